"""What the MLP + Memcodes tokenizer tests and their fixture generator (tests/golden/make_golden_memcodes.py) share: two small
configurations (a BottleneckMLP and a StandardMLP tokenizer with a multi-head Memcodes quantizer), their seeded state dicts in upstream's
layout and seeded inputs.  Everything is regenerated from seeds on both sides; the fixture keeps upstream's outputs only.

The keys are spelled out here, not read off either model: the fixture's key list (upstream's) and the package's state_dict() are both
compared with them."""
import math

import torch

from oracle.fourm_oracle import seeded_tensor

U = 2.0 ** -24

CASES = {
    # BottleneckMLP/B_2-Wi_64 both ways, 24 input channels, latent 64 in 4 heads of 16, 50 codes per head
    "bmlp_small": dict(mlp="BottleneckMLP/B_2-Wi_64", channels=24, latent=64, heads=4, codebook=50, width=64, depth=2, expansion=4, seed=11),
    # MLP/B_3-Wi_64 both ways (two inner layers), 2 heads of 32, 37 codes per head
    "mlp_small": dict(mlp="MLP/B_3-Wi_64", channels=24, latent=64, heads=2, codebook=37, width=64, depth=3, expansion=None, seed=12),
}
# (name, batch, h, w): one vector per sample (upstream's real use; decoded too) and a 1 x 3 grid (encode only)
INPUTS = [("g1", 5, 1, 1), ("g3", 2, 1, 3)]


def kwargs(c):
    """Constructor arguments of the case, identical for upstream's VQVAE and this package's."""
    return dict(enc_type=c["mlp"], dec_type=c["mlp"], n_channels=c["channels"], latent_dim=c["latent"], num_codebooks=c["heads"],
                codebook_size=c["codebook"], quant_type="memcodes", patch_proj=False, sync_codebook=False)


def _linear(sd, name, n_out, n_in, seed):
    sd[name + ".weight"] = seeded_tensor(name + ".weight", (n_out, n_in), 1.0 / math.sqrt(n_in), seed)
    sd[name + ".bias"] = seeded_tensor(name + ".bias", (n_out,), 0.2, seed)


def _norm(sd, name, n, seed):
    sd[name + ".weight"] = 1.0 + seeded_tensor(name + ".weight", (n,), 0.2, seed)
    sd[name + ".bias"] = seeded_tensor(name + ".bias", (n,), 0.3, seed)


def mlp_state(prefix, c, dim_in, dim_out):
    """One BottleneckMLP / StandardMLP in upstream's names.  LayerNorm affines and every bias non-trivial."""
    sd, W, seed = {}, c["width"], c["seed"]
    _linear(sd, f"{prefix}.linear_in", W, dim_in, seed)
    _linear(sd, f"{prefix}.linear_out", dim_out, W, seed)
    if c["expansion"] is not None:
        for i in range(c["depth"]):
            _linear(sd, f"{prefix}.blocks.{i}.block.0", c["expansion"] * W, W, seed)
            _linear(sd, f"{prefix}.blocks.{i}.block.2", W, c["expansion"] * W, seed)
            _norm(sd, f"{prefix}.layernorms.{i}", W, seed)
    else:
        for i in range(c["depth"] - 1):
            _linear(sd, f"{prefix}.layers.{i}", W, W, seed)
            _norm(sd, f"{prefix}.layernorms.{i}", W, seed)
    return sd


def state_dict(c):
    """The whole VQVAE: encoder, quant_proj, quantize.{codes, to_k.weight, to_v.weight}, decoder, post_quant_proj."""
    W, Ld, H, K, seed = c["width"], c["latent"], c["heads"], c["codebook"], c["seed"]
    d = Ld // H
    sd = mlp_state("encoder", c, c["channels"], W)
    sd["quant_proj.weight"] = seeded_tensor("quant_proj.weight", (Ld, W, 1, 1), 1.0 / math.sqrt(W), seed)
    sd["quant_proj.bias"] = seeded_tensor("quant_proj.bias", (Ld,), 0.2, seed)
    sd["quantize.codes"] = seeded_tensor("quantize.codes", (H, K, d), 1.0, seed)
    sd["quantize.to_k.weight"] = seeded_tensor("quantize.to_k.weight", (H, d, d), 1.0 / math.sqrt(d), seed)
    sd["quantize.to_v.weight"] = seeded_tensor("quantize.to_v.weight", (H, d, d), 1.0 / math.sqrt(d), seed)
    sd.update(mlp_state("decoder", c, W, c["channels"]))
    sd["post_quant_proj.weight"] = seeded_tensor("post_quant_proj.weight", (W, Ld, 1, 1), 1.0 / math.sqrt(Ld), seed)
    sd["post_quant_proj.bias"] = seeded_tensor("post_quant_proj.bias", (W,), 0.2, seed)
    return sd


def inputs(name, c):
    """{input name: (B, channels, h, w) f32}."""
    return {tag: seeded_tensor(f"memcodes.{name}.{tag}", (B, c["channels"], h, w), 1.0, c["seed"]) for tag, B, h, w in INPUTS}


def checksum(tensors):
    return sum(float(v.double().abs().sum()) for v in tensors)


def keys64(sd):
    """Float64 keys and values (H, K, d) from the fp32 parameters: codes[h] @ to_k.weight[h], codes[h] @ to_v.weight[h]."""
    codes = sd["quantize.codes"].double()
    return torch.einsum("hnd,hdc->hnc", codes, sd["quantize.to_k.weight"].double()), torch.einsum("hnd,hdc->hnc", codes, sd["quantize.to_v.weight"].double())


def head_scores64(z, k64):
    """z (R, H d) any float dtype, k64 (H, K, d) -> float64 scores (R, H, K) = <z_h, k_hj> (no d^-0.5: the search leaves the scale out)."""
    H, K, d = k64.shape
    return torch.einsum("rhd,hjd->rhj", z.double().reshape(z.shape[0], H, d), k64.to(z.device))


def margins64(s64):
    """(float64 arg-max (lowest index), top-2 margin) of scores (R, H, K); the margin of a single key is +inf."""
    if s64.shape[-1] == 1:
        return s64.argmax(-1), torch.full(s64.shape[:-1], float("inf"), dtype=torch.float64, device=s64.device)
    top = s64.topk(2, dim=-1).values
    return s64.argmax(-1), top[..., 0] - top[..., 1]


def score_bound(z, k64):
    """d u |z_h| max_j |k_hj| per (row, head): Cauchy-Schwarz bound of one any-order fp32 chain, u = 2^-24."""
    H, K, d = k64.shape
    zn = z.double().reshape(z.shape[0], H, d).norm(dim=-1)
    return d * U * zn * k64.to(z.device).norm(dim=-1).max(dim=-1).values[None, :]


def rows_of(t):
    """(B, C, h, w) -> (B h w, C)."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def tokens_rows(tokens):
    """tokens (B, H, h, w) -> (B h w, H)."""
    return tokens.permute(0, 2, 3, 1).reshape(-1, tokens.shape[1])
