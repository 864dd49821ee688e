"""SAM-instance tokenizer on a real MI355X: VQVAE(one-channel 64 x 64 masks, patch 16, latent_dim 1024, 1024 codes, out_conv) end to end
against the fixture of the unmodified upstream model (tests/golden/make_golden_sam_instance.py), the refusals that stay, and upstream's
full geometry (vit_b, batch 384)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import vq_oracle as V
from tests import sam_instance_util as S
from tests.parity_log import record

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
U = 2.0 ** -24


def _rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


@pytest.fixture(scope="module")
def small():
    from fourm.vq import VQVAE
    c = S.SAM_SMALL
    sd = S.sam_state_dict(c)
    m = VQVAE(**S.sam_kwargs(c))
    m.load_state_dict(sd, strict=True)
    x = S.synthetic_masks(c["batch"], c["image"], seed=c["seed"])
    return c, S.sam_cfg(c), sd, m.cuda().eval(), x, np.load(os.path.join(GOLD, "sam_instance_small.npz"))


def test_tokenize_matches_upstream_fixture(small):
    c, cfg, sd, m, x, g = small
    quant, loss, tokens = m.encode(x.cuda())
    assert tokens.dtype == torch.int64 and tuple(tokens.shape) == (c["batch"], 4, 4) and tuple(quant.shape) == (c["batch"], 1024, 4, 4) and float(loss) == 0.0
    ref_tok = torch.from_numpy(g["tokens"]).long()
    z = m._last_latents.float().cpu()
    ref_z = torch.from_numpy(g["latents"])
    rel = _rel(z, ref_z)
    # the yardstick: the reference's own autocast-vs-fp32 agreement on this very case (as tests/test_vq.py obtains oracle_self)
    _, tok_fp, _ = V.vq_encode(sd, cfg, x)
    assert torch.equal(tok_fp, ref_tok)                                       # the oracle restates upstream for this configuration
    _, tok_bf, _ = V.vq_encode(sd, cfg, x, emulate_bf16=True)
    oracle_self = float((tok_bf == ref_tok).float().mean())
    agree = float((tokens.cpu() == ref_tok).float().mean())
    agree_bf = float((tokens.cpu() == tok_bf).float().mean())
    print(f"sam_small: latent rel err {rel:.3e}, token agreement vs fp32 {agree:.4f}, vs autocast oracle {agree_bf:.4f}, oracle autocast-vs-fp32 {oracle_self:.4f}")
    record("sam_instance.tokenize", latent_rel_vs_fp32=rel, token_agreement_vs_fp32=agree, token_agreement_vs_autocast_oracle=agree_bf, oracle_autocast_vs_fp32=oracle_self)
    assert rel < 3e-2, rel
    assert agree >= 0.95 * oracle_self, (agree, oracle_self)
    # every disagreeing row is a near tie in upstream's fp32 scores
    en = F.normalize(sd["quantize._codebook.embed"], dim=-1)
    sims = F.normalize(ref_z.reshape(-1, 1024), dim=-1) @ en.t()
    mine = tokens.cpu().reshape(-1)
    for r in (mine != ref_tok.reshape(-1)).nonzero().flatten().tolist():
        assert float(sims[r].max() - sims[r, mine[r]]) < 2e-2, r
    assert torch.equal(quant, m.tokens_to_embedding(tokens))


def test_search_alone_on_upstream_latents(small):
    """Given upstream's fp32 latents the search must meet the two conditions of tests/test_vq_wide_gpu.py against the fixture's tokens and
    float64 margins: the score of the chosen code within 2 bound of the float64 maximum on every row, the fixture's token on every row whose
    margin exceeds 2 bound."""
    from fourm.vq import engine as E
    c, cfg, sd, m, x, g = small
    D = 1024
    bound = (D + 8) * U
    z = torch.from_numpy(g["latents"]).reshape(-1, D).cuda().contiguous()
    B = c["batch"]
    tok = E._assign(m, E._engine(m.encoder), z, z.shape[0], 16, B, 4, 4, False).reshape(-1)
    s64 = F.normalize(z.double(), dim=-1) @ F.normalize(m.quantize._codebook.embed.double(), dim=-1).t()
    gap = s64.max(1).values - s64.gather(1, tok[:, None])[:, 0]
    margin = torch.from_numpy(g["margin64"]).cuda()
    ref_tok = torch.from_numpy(g["tokens"]).long().reshape(-1).cuda()
    clear = margin > 2 * bound
    print(f"sam_small search: worst gap / (2 bound) {float(gap.max() / (2 * bound)):.3g}, rows above the margin {int(clear.sum())} of {len(tok)}")
    assert bool((gap <= 2 * bound).all())
    assert torch.equal(tok[clear], ref_tok[clear]) and int(clear.sum()) >= 0.98 * len(tok)


def test_decode_tokens_matches_upstream_fixture(small):
    c, cfg, sd, m, x, g = small
    tok = torch.from_numpy(g["tokens"]).long().cuda()
    dec = m.decode_tokens(tok)
    ref = torch.from_numpy(g["dec_tokens"])
    assert tuple(dec.shape) == (c["batch"], 1, 64, 64) and dec.dtype == torch.float32
    rel = _rel(dec.cpu(), ref)
    err = float((dec.cpu() - ref).abs().max())
    # sigmoid(dec) > 0.5 is dec > 0 (decode_sam_instances, plotting_utils.py:628-630): every pixel whose upstream logit is farther from 0 than the error
    far = ref.abs() > err
    same = ((dec.cpu() > 0) == (ref > 0))[far]
    print(f"sam_small decode_tokens: rel Frobenius {rel:.3e} (bound 1.5e-2), max abs err {err:.3e}, pixels beyond it {int(far.sum())} of {ref.numel()}")
    record("sam_instance.decode_tokens", rel_fro=rel, max_abs_err=err, pixels_beyond_err=int(far.sum()), pixels=ref.numel())
    assert rel < 1.5e-2, rel
    assert bool(same.all()) and int(far.sum()) > 0
    assert torch.equal((torch.sigmoid(dec.cpu()) > 0.5)[far], (torch.sigmoid(ref) > 0.5)[far])
    # bit-reproducible across calls and batch splits; the two entry points share one path
    assert torch.equal(m.decode_tokens(tok), dec)
    assert torch.equal(torch.cat([m.decode_tokens(tok[:2]), m.decode_tokens(tok[2:])]), dec)
    assert torch.equal(m.decode_quant(m.tokens_to_embedding(tok)), dec)
    # autoencode = tokenize + decode_tokens
    with torch.no_grad():
        ae = m.autoencode(x.cuda())
    assert torch.equal(ae, m.decode_tokens(m.tokenize(x.cuda())))


def test_out_conv_branch_reaches_the_output(small):
    """The ConvNeXt tail is computed, not skipped: zeroing both layer scales changes the reconstruction by the branch upstream's fixture contains."""
    c, cfg, sd, m, x, g = small
    tok = torch.from_numpy(g["tokens"]).long().cuda()
    dec = m.decode_tokens(tok)
    keep = [b.gamma.detach().clone() for b in m.decoder.out_conv]
    try:
        with torch.no_grad():
            for b in m.decoder.out_conv:
                b.gamma.zero_()
        plain = m.decode_tokens(tok)
    finally:
        with torch.no_grad():
            for b, k in zip(m.decoder.out_conv, keep):
                b.gamma.copy_(k)
    # (with one channel each block adds the constant gamma (w2 . GELU(w1 beta + b1) + b2): +0.050 and -0.351 for the seeded weights, 8.5 % of the fixture's RMS)
    assert _rel(plain.cpu(), torch.from_numpy(g["dec_tokens"])) > 0.05
    assert torch.equal(m.decode_tokens(tok), dec)


def _untouched(model):
    """No engine was ever built for the model's encoder / decoder: no workspace, no kernel."""
    return getattr(model.encoder, "_hip_engine", None) is None and getattr(getattr(model, "decoder", None), "_hip_engine", None) is None


def test_refusals_stay_loud_and_launch_nothing():
    from fourm.hip import _lib as L
    from fourm.vq import VQ, VQVAE
    before = L.lib.fm_last_error()
    x = S.synthetic_masks(2, 64).cuda()
    wide = VQVAE(**S.sam_kwargs()).cuda()
    # training mode with gradients
    wide.train()
    with pytest.raises(NotImplementedError, match="latent_dim=1024 is inference only"):
        wide(x)
    # eval mode, gradients enabled and trainable parameters: still the differentiable forward
    wide.eval()
    with pytest.raises(NotImplementedError, match="inference only"):
        wide(x)
    # training-mode quantizer without gradients (EMA codebook update)
    wide.train()
    with torch.no_grad():
        with pytest.raises(NotImplementedError, match="fm_vq_ema_update"):
            wide(x)
    for p in wide.parameters():
        p.requires_grad = False
    with pytest.raises(NotImplementedError, match="training-mode quantizer"):
        wide.encode(x)
    assert _untouched(wide)
    # a narrow latent with out_conv: the ConvNeXt blocks have no backward
    kw = dict(S.sam_kwargs(), latent_dim=32, codebook_size=64)
    narrow = VQVAE(**kw).cuda().train()
    with pytest.raises(NotImplementedError, match="ConvNeXt blocks .* have no backward"):
        narrow(x)
    assert _untouched(narrow)
    with torch.no_grad():
        assert tuple(narrow.eval().autoencode(x).shape) == (2, 1, 64, 64)      # inference runs
    # Euclidean codebook at another width; out_conv with more than 4 channels
    eu = VQ(image_size=32, enc_type="vit_s_enc", patch_size=8, post_mlp=True, codebook_size=64, latent_dim=64, norm_codes=False, sync_codebook=False).cuda().eval()
    with pytest.raises(NotImplementedError, match="Euclidean codebook .* latent_dim=64"):
        eu.tokenize(torch.rand(2, 3, 32, 32, device="cuda"))
    assert _untouched(eu)
    with pytest.raises(NotImplementedError, match="at most 4 channels"):
        VQVAE(image_size=32, n_channels=8, n_labels=20, enc_type="vit_s_enc", dec_type="vit_s_dec", patch_size=8, codebook_size=64, latent_dim=8, out_conv=True)
    assert L.lib.fm_last_error() == before


def test_full_size_geometry():
    """Upstream's SAM-instance tokenizer as configured (vit_b_enc / vit_b_dec, batch 384 instances, seeded weights, no fixture)."""
    from fourm.vq import VQVAE
    torch.manual_seed(0)
    m = VQVAE(enc_type="vit_b_enc", dec_type="vit_b_dec", image_size=64, n_channels=1, patch_size=16, latent_dim=1024, codebook_size=1024, norm_codes=True,
              out_conv=True, post_mlp=True, sync_codebook=False)
    with torch.no_grad():
        for b in m.decoder.out_conv:
            b.gamma.fill_(0.7)
    m = m.cuda().eval()
    x = S.synthetic_masks(384, 64, seed=1).cuda()
    tok = m.tokenize(x)
    dec = m.decode_tokens(tok)
    assert tuple(tok.shape) == (384, 4, 4) and tuple(dec.shape) == (384, 1, 64, 64)
    assert bool(torch.isfinite(dec).all()) and int(tok.min()) >= 0 and int(tok.max()) < 1024
    assert torch.equal(m.tokenize(x), tok) and torch.equal(m.decode_tokens(tok), dec)
    tok6 = m.tokenize(x[:6])
    assert torch.equal(tok6, tok[:6])
    assert torch.equal(m.decode_tokens(tok6), dec[:6])
