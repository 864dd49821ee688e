"""compute_precision = "fp32" of the ViT tokenizer on the GPU: f32 patch rows, the 12 blocks on the trunk's fp32 kernels, fm_gemm_f32 for the patch
projection / tanh post-MLP / quant_proj, against upstream's fp32 latents and tokens (the fixtures of tests/test_vq.py)."""
import numpy as np
import pytest
import torch

from tests.golden.cases import VQ_CASES
from tests.parity_log import record
from tests.test_vq import build, case

pytestmark = pytest.mark.gpu

NEAR_TIE = 1e-4          # reference rows whose top-1 / top-2 cosine similarities are closer than this may fall on either of the two codes


@pytest.mark.parametrize("name", list(VQ_CASES))
def test_tokenize_in_fp32_reproduces_upstream(name):
    """Latents within 2e-5 x max |latents| of upstream's (the tolerance the CPU oracle is held to, tests/test_vq.py); tokens identical on every
    row whose reference similarities are >= 1e-4 apart, first or second choice of the reference on the (at most four) others."""
    c, cfg, sd, x, g = case(name)
    model = build(c, cfg)
    model.load_state_dict(sd)
    model = model.cuda().eval()
    model.compute_precision = "fp32"
    quant, loss, tokens = model.encode(x.cuda())
    assert tokens.dtype == torch.int64 and tuple(tokens.shape) == (c["batch"], cfg.grid, cfg.grid) and quant.dtype == torch.float32 and float(loss) == 0.0
    eng = model.encoder._hip_engine
    assert eng.fp32 and not eng.shadows and all(t.dtype != torch.bfloat16 for t in eng.ws.bufs.values())
    # latents
    z = model._last_latents.float().cpu()
    ref = torch.from_numpy(g["latents"])
    err, scale = float((z - ref).abs().max()), float(ref.abs().max())
    # tokens
    en = torch.nn.functional.normalize(sd["quantize._codebook.embed"].double(), dim=-1)
    top = (torch.nn.functional.normalize(ref.double().reshape(-1, cfg.latent), dim=-1) @ en.t()).topk(2, dim=-1)
    gap = top.values[:, 0] - top.values[:, 1]
    want, mine = torch.from_numpy(g["tokens"]).long().reshape(-1), tokens.cpu().reshape(-1)
    assert torch.equal(top.indices[:, 0], want)                               # (the fixture's tokens are the reference's first choice)
    clear = gap >= NEAR_TIE
    agree = float((mine == want).float().mean())
    print(f"{name}: latents max abs err {err:.3e} = {err / scale:.3e} of max |latents| (bound 2e-5); min reference gap {float(gap.min()):.3e} over {gap.numel()} rows, "
          f"{int((~clear).sum())} below {NEAR_TIE:g}; token agreement {agree:.4f}")
    record("vq.tokenize.fp32", case=name, latent_max_abs_err=err, latent_err_over_max=err / scale, token_agreement=agree, rows=gap.numel(),
           near_tie_rows=int((~clear).sum()), min_reference_gap=float(gap.min()))
    assert err <= 2e-5 * scale, (err, scale)
    assert int((~clear).sum()) <= 4
    assert torch.equal(mine[clear], want[clear]), int((mine[clear] != want[clear]).sum())
    near = ~clear
    assert bool(((mine[near] == top.indices[near, 0]) | (mine[near] == top.indices[near, 1])).all())
    if name == "vq_small":
        assert bool(clear.all()) and np.array_equal(tokens.cpu().numpy(), g["tokens"])
    # the default mode is still there after flipping back, and flips again
    model.compute_precision = "bf16"
    t_bf = model.tokenize(x.cuda())
    assert model.encoder._hip_engine.adt == torch.bfloat16 and float((t_bf.cpu().reshape(-1) == want).float().mean()) > 0.9
    model.compute_precision = "fp32"
    assert torch.equal(model.tokenize(x.cuda()), tokens)


def test_tokenize_sub_batches_on_two_streams_in_fp32():
    """fourm.vq.tokenize_sub_batches with two sub-batches in flight in fp32 mode: the tokens of one call after the other, bit for bit."""
    from fourm.vq import VQ, tokenize_sub_batches
    torch.manual_seed(3)
    model = VQ(image_size=64, enc_type="vit_s_enc", patch_size=16, post_mlp=True, codebook_size=256, latent_dim=32, norm_codes=True, sync_codebook=False).cuda().eval()
    model.compute_precision = "fp32"
    subs = [torch.rand(n, 3, 64, 64, device="cuda") * 2 - 1 for n in (5, 8, 3)]        # ragged sub-batch sizes
    want = [model.tokenize(x).clone() for x in subs]
    for n in (2, 1):
        got = tokenize_sub_batches(model, subs, n_streams=n)
        torch.cuda.synchronize()
        assert len(got) == len(want) and all(torch.equal(g, w) for g, w in zip(got, want)), n
    assert model.encoder._hip_engine.fp32


def test_fp32_input_preparation_is_upstreams():
    """undo_std and n_labels in fp32 mode: the model fed raw inputs gives what the plain model gives on upstream's prepare_input (vqvae.py:282-285:
    2 * denormalize(x) - 1 with denormalize = (x + m / s) / (1 / s); cls_emb(x) as 'b h w c -> b c h w'), computed here on the CPU."""
    from fourm.vq import VQ
    kw = dict(image_size=64, enc_type="vit_s_enc", patch_size=16, post_mlp=True, codebook_size=256, latent_dim=32, norm_codes=True, sync_codebook=False)

    def pair(n_channels, **extra):
        torch.manual_seed(4)
        plain = VQ(n_channels=n_channels, **kw)
        other = VQ(n_channels=n_channels, **extra, **kw)
        other.load_state_dict(plain.state_dict(), strict=False)
        plain, other = plain.cuda().eval(), other.cuda().eval()
        plain.compute_precision = other.compute_precision = "fp32"
        return plain, other

    def same(plain, prepared, other, raw):
        t_other = other.tokenize(raw.cuda())
        z_other = other._last_latents.clone()
        t_plain = plain.tokenize(prepared.cuda())
        z_plain = plain._last_latents
        assert float((z_other - z_plain).abs().max()) <= 2e-5 * float(z_plain.abs().max()) and torch.equal(t_other, t_plain)

    g = torch.Generator().manual_seed(8)
    plain, std_model = pair(3, undo_std=True)
    x = torch.randn(2, 3, 64, 64, generator=g)
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    m2 = torch.tensor([-m / s for m, s in zip(mean, std)]).view(1, 3, 1, 1)
    s2 = torch.tensor([1 / s for s in std]).view(1, 3, 1, 1)
    same(plain, 2.0 * ((x - m2) / s2) - 1.0, std_model, x)
    plain, lab_model = pair(4, n_labels=7)
    labels = torch.randint(0, 7, (2, 64, 64), generator=g)
    same(plain, lab_model.cls_emb.weight.detach().cpu()[labels].permute(0, 3, 1, 2).contiguous(), lab_model, labels)
