"""Shared pieces of the CLIP text-tower tests: the two micro towers, a seeded filler for their weights and token ids, and ``text_forward`` - a
plain-torch restatement of ``CLIP.encode_text`` that runs in any float type (float64 is the yardstick of the GPU tests; upstream's class is
absent where the GPU tests run).

tests/golden/make_golden_clip_text.py pins the restatement to upstream's class: tests/test_clip_text_cpu.py checks that it reproduces upstream's
float64 and fp32 outputs stored in tests/golden/clip_text_micro.npz.

Case A: width 128, 2 heads, 2 layers, 12 tokens, vocabulary 50, embed_dim 40 (not a multiple of 16 or 64: the projection's padded columns),
        3 samples.
Case B: width 64, 1 head, 1 layer, 77 tokens (an odd key count past one 64-key tile of the attention kernel), vocabulary 300, embed_dim 64,
        2 samples.
The end-of-text token (the largest id of a row, vocab - 1) sits at position 1, in the middle and at Lc - 1; the "middle" row carries it a
second time further on, so that only the FIRST maximum gives the right row."""
import os

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "clip_text_micro.npz")

CASES = {
    "text_a": dict(embed_dim=40, context_length=12, vocab_size=50, width=128, heads=2, layers=2),
    "text_b": dict(embed_dim=64, context_length=77, vocab_size=300, width=64, heads=1, layers=1),
}
BATCH = {"text_a": 3, "text_b": 2}
# per row: (position of the end-of-text id, position of its second occurrence or None)
EOT = {
    "text_a": [(1, None), (6, 9), (11, None)],
    "text_b": [(38, 60), (76, None)],
}
FLAGS = ["default", "return_all_tokens", "return_patch_tokens"]
LN_EPS = 1e-5


def flag_kwargs(flag):
    return {} if flag == "default" else {flag: True}


def expected_shapes(case):
    """(key, shape) of the text tower's state dict in upstream's order (CLIP's own parameters first, then its modules; the ``visual.*`` keys and
    ``logit_scale`` left out)."""
    c = CASES[case]
    w = c["width"]
    out = [("positional_embedding", (c["context_length"], w)), ("text_projection", (w, c["embed_dim"]))]
    for i in range(c["layers"]):
        b = f"transformer.resblocks.{i}."
        out += [(b + "attn.in_proj_weight", (3 * w, w)), (b + "attn.in_proj_bias", (3 * w,)), (b + "attn.out_proj.weight", (w, w)),
                (b + "attn.out_proj.bias", (w,)), (b + "ln_1.weight", (w,)), (b + "ln_1.bias", (w,)), (b + "mlp.c_fc.weight", (4 * w, w)),
                (b + "mlp.c_fc.bias", (4 * w,)), (b + "mlp.c_proj.weight", (w, 4 * w)), (b + "mlp.c_proj.bias", (w,)), (b + "ln_2.weight", (w,)),
                (b + "ln_2.bias", (w,))]
    return out + [("token_embedding.weight", (c["vocab_size"], w)), ("ln_final.weight", (w,)), ("ln_final.bias", (w,))]


def seeded_state_dict(case):
    """fp32 weights from a seed (not stored anywhere): matrices at fan-in scale, every bias nonzero (c_fc: std 0.5, so that QuickGELU sees both
    tails), LayerNorm weights 1 +- 0.2 with biases of std 0.1, token and position rows of std 0.5."""
    g = torch.Generator().manual_seed(3000 + sorted(CASES).index(case))
    sd = {}
    for key, shape in expected_shapes(case):
        r = torch.randn(*shape, generator=g)
        if ".ln_" in key or key.startswith("ln_"):
            v = 1.0 + 0.2 * r if key.endswith("weight") else 0.1 * r
        elif key.endswith("c_fc.bias"):
            v = 0.5 * r
        elif key.endswith("bias"):
            v = 0.2 * r
        elif key in ("positional_embedding", "token_embedding.weight"):
            v = 0.5 * r
        elif key == "text_projection":
            v = r * shape[0] ** -0.5
        else:
            v = r * shape[1] ** -0.5
        sd[key] = v.float().contiguous()
    return sd


def token_ids(case, batch=None):
    """int64 (B, Lc): ids below vocab - 1 everywhere, vocab - 1 at the row's end-of-text position(s).  ``batch`` above the case's own size
    repeats the position pattern (one draw of 64 rows is sliced, so the first rows are the case's rows whatever the batch)."""
    c = CASES[case]
    B = BATCH[case] if batch is None else batch
    assert 0 < B <= 64
    g = torch.Generator().manual_seed(4000 + sorted(CASES).index(case))
    ids = torch.randint(0, c["vocab_size"] - 1, (64, c["context_length"]), generator=g)[:B].contiguous()
    for b in range(B):
        first, second = EOT[case][b % len(EOT[case])]
        ids[b, first] = c["vocab_size"] - 1
        if second is not None:
            ids[b, second] = c["vocab_size"] - 1
    return ids


def eot_positions(case, batch=None):
    B = BATCH[case] if batch is None else batch
    return [EOT[case][b % len(EOT[case])][0] for b in range(B)]


def checksum(case):
    """Order-independent integer checksum of the regenerated inputs: the fp32 bit patterns of every weight and the ids, summed as int64."""
    total = int(token_ids(case).sum())
    for v in seeded_state_dict(case).values():
        total += int(v.view(torch.int32).to(torch.int64).sum())
    return total


def text_forward(sd, ids, flag="default", dtype=torch.float64):
    """``CLIP.encode_text`` as plain tensor algebra in ``dtype``: token rows + position rows, pre-LN blocks (causal softmax attention with 64-wide
    heads, QuickGELU MLP), ln_final, and per ``flag``: the normalised tokens, every token projected, or the projected row at the first maximum
    of each sample's ids."""
    p = {k: v.to(dtype) for k, v in sd.items()}
    D = p["ln_final.weight"].shape[0]
    B, Lc = ids.shape
    heads = D // 64

    def ln(t, name):
        return F.layer_norm(t, (D,), p[name + ".weight"], p[name + ".bias"], LN_EPS)

    t = p["token_embedding.weight"][ids] + p["positional_embedding"]
    blocked = torch.ones(Lc, Lc, dtype=torch.bool).triu(1)
    i = 0
    while f"transformer.resblocks.{i}.ln_1.weight" in p:
        b = f"transformer.resblocks.{i}."
        h = ln(t, b + "ln_1")
        q, k, v = (h @ p[b + "attn.in_proj_weight"].t() + p[b + "attn.in_proj_bias"]).reshape(B, Lc, 3, heads, 64).permute(2, 0, 3, 1, 4)
        s = (q @ k.transpose(-1, -2) * 64 ** -0.5).masked_fill(blocked, float("-inf"))
        a = torch.softmax(s, -1) @ v
        t = t + a.permute(0, 2, 1, 3).reshape(B, Lc, D) @ p[b + "attn.out_proj.weight"].t() + p[b + "attn.out_proj.bias"]
        u = ln(t, b + "ln_2") @ p[b + "mlp.c_fc.weight"].t() + p[b + "mlp.c_fc.bias"]
        u = u * torch.sigmoid(1.702 * u)
        t = t + u @ p[b + "mlp.c_proj.weight"].t() + p[b + "mlp.c_proj.bias"]
        i += 1
    t = ln(t, "ln_final")
    if flag == "return_patch_tokens":
        return t
    if flag == "return_all_tokens":
        return t @ p["text_projection"]
    assert flag == "default", flag
    return t[torch.arange(B), ids.argmax(dim=-1)] @ p["text_projection"]


def rel_max(a, ref):
    """max |a - ref| / max |ref| in float64: the distance the fixture stores and the tests bound."""
    ref = ref.double()
    return float((a.double().cpu() - ref.cpu()).abs().max() / ref.abs().max())


def load_golden():
    return np.load(GOLDEN)


def autocast_output(gold, case, flag):
    """Upstream's result under CPU bf16 autocast as fp32: the fixture keeps a bf16 result as its 16-bit patterns."""
    a = torch.from_numpy(gold[f"{case}/{flag}/out_ac"])
    return a.view(torch.bfloat16).float() if a.dtype == torch.int16 else a
