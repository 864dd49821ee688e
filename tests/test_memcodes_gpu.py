"""MLP + Memcodes tokenizers on a real MI355X, end to end against the fixture of the unmodified upstream model
(tests/golden/make_golden_memcodes.py): latents and reconstruction against upstream's float64 run, tokens against upstream's wherever the
float64 margin decides them, the token -> embedding -> reconstruction identities, batch invariance, the refresh of the cached keys, and
upstream's full geometry (BottleneckMLP/B_6-Wi_1024, 8 x 8192 codes, batch 64).

Tolerances.  Latents / reconstruction: relative Frobenius error against float64 at most 8 x upstream's OWN fp32-vs-float64 error stored in
the fixture (a sequential fmaf chain and a blocked BLAS sum differ in typical error).  Tokens: b = d u |z_h| max_j |k_hj| bounds the error
of one fp32 score (Cauchy-Schwarz, u = 2^-24); a (row, head) pair is decided wherever the float64 top-2 margin exceeds 2 b (given the
fixture's latents) or 2 (d u |z_h| + |z_h - z64_h|) max_j |k_hj| (end to end, z the latents measured here)."""
import os

import numpy as np
import pytest
import torch

from tests import memcodes_util as M
from tests.parity_log import record

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
_MODELS = {}


def _rel(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


def build(name):
    from fourm.vq import VQVAE
    c = M.CASES[name]
    m = VQVAE(**M.kwargs(c))
    m.load_state_dict(M.state_dict(c), strict=True)
    return m.cuda().eval()


def case(name):
    """(case, state dict, shared model, inputs, fixture view): built once per case, left unchanged by the tests that share it."""
    if name not in _MODELS:
        c = M.CASES[name]
        g = np.load(os.path.join(GOLD, "memcodes_small.npz"))
        _MODELS[name] = (c, M.state_dict(c), build(name), M.inputs(name, c), {k[len(name) + 1:]: g[k] for k in g.files if k.startswith(name + "/")})
    return _MODELS[name]


NAMES = list(M.CASES)


@pytest.mark.parametrize("name", NAMES)
def test_latents_and_reconstruction_against_float64(name):
    c, sd, m, xs, g = case(name)
    worst = 0.0
    for tag, B, h, w in M.INPUTS:
        quant, loss, tokens = m.encode(xs[tag].cuda())
        assert tokens.dtype == torch.int64 and tuple(tokens.shape) == (B, c["heads"], h, w) and tuple(quant.shape) == (B, c["latent"], h, w)
        assert float(loss) == 0.0 and tuple(loss.shape) == (1,)
        z = m._last_latents.reshape(B * h * w, c["latent"]).cpu()
        rel, ref = _rel(z, torch.from_numpy(g[f"{tag}/latents64"])), float(g[f"{tag}/latents_rel"])
        print(f"{name} {tag}: latents vs float64 {rel:.3e}, upstream's own {ref:.3e}, ratio {rel / ref:.3g} (bound 8)")
        record("memcodes.latents", case=name, grid=tag, rel_vs_float64=rel, upstream_rel_vs_float64=ref, ratio=rel / ref)
        worst = max(worst, rel / ref)
        assert rel <= 8 * ref, (rel, ref)
    tok = torch.from_numpy(g["g1/tokens"]).long().cuda()
    dec = m.decode_tokens(tok)
    assert tuple(dec.shape) == (5, c["channels"], 1, 1) and dec.dtype == torch.float32
    rel, ref = _rel(dec.cpu(), torch.from_numpy(g["g1/dec_tokens64"])), float(g["g1/dec_rel"])
    print(f"{name}: decode_tokens vs float64 {rel:.3e}, upstream's own {ref:.3e}, ratio {rel / ref:.3g} (bound 8)")
    record("memcodes.decode_tokens", case=name, rel_vs_float64=rel, upstream_rel_vs_float64=ref, ratio=rel / ref)
    assert rel <= 8 * ref, (rel, ref)
    assert _rel(dec.cpu(), torch.from_numpy(g["g1/dec_tokens"])) < 1e-5         # and upstream's fp32 run, loosely: the same function


@pytest.mark.parametrize("name", NAMES)
def test_search_alone_on_upstream_latents(name):
    """Given upstream's fp32 latents: upstream's token on every (row, head) whose stored float64 margin exceeds 2 b."""
    from fourm.vq import engine as E
    c, sd, m, xs, g = case(name)
    k64, v64 = M.keys64(sd)
    keys, values = E.memcodes_tables(m.quantize)
    assert _rel(keys.cpu(), k64) < 1e-6 and _rel(values.cpu(), v64) < 1e-6
    for tag, B, h, w in M.INPUTS:
        z = torch.from_numpy(g[f"{tag}/latents"]).cuda().contiguous()
        tok, quant = E._memcodes_assign(m.quantize, z, B, h, w)
        clear = torch.from_numpy(g[f"{tag}/margin64"]) > 2 * M.score_bound(z.cpu(), k64)
        mine, ref = M.tokens_rows(tok.cpu()), M.tokens_rows(torch.from_numpy(g[f"{tag}/tokens"]).long())
        print(f"{name} {tag} search: pairs above the margin {int(clear.sum())} of {clear.numel()}, mismatches {int((mine != ref).sum())}")
        assert torch.equal(mine[clear], ref[clear]) and int(clear.sum()) >= 0.98 * clear.numel()
        assert _rel(quant.cpu(), torch.from_numpy(g[f"{tag}/quant"])) < 1e-5


@pytest.mark.parametrize("name", NAMES)
def test_tokens_end_to_end(name):
    c, sd, m, xs, g = case(name)
    k64, _ = M.keys64(sd)
    H, d = c["heads"], c["latent"] // c["heads"]
    kmax = k64.norm(dim=-1).max(dim=-1).values
    n_clear = n_all = 0
    for tag, B, h, w in M.INPUTS:
        tokens = m.tokenize(xs[tag].cuda())
        z = m._last_latents.reshape(B * h * w, c["latent"]).cpu().double()
        z64 = torch.from_numpy(g[f"{tag}/latents64"])
        dz = (z - z64).reshape(-1, H, d).norm(dim=-1)
        bound = (M.score_bound(z, k64) / kmax[None, :] + dz) * kmax[None, :]    # (d u |z_h| + |z_h - z64_h|) max_j |k_hj|
        clear = torch.from_numpy(g[f"{tag}/margin64_z64"]) > 2 * bound
        mine = M.tokens_rows(tokens.cpu())
        assert torch.equal(mine[clear], torch.from_numpy(g[f"{tag}/argmax64_z64"]).long()[clear])
        both = clear & (torch.from_numpy(g[f"{tag}/margin64"]) > 2 * M.score_bound(torch.from_numpy(g[f"{tag}/latents"]), k64))
        assert torch.equal(mine[both], M.tokens_rows(torch.from_numpy(g[f"{tag}/tokens"]).long())[both])          # upstream's fp32 tokens
        n_clear += int(clear.sum())
        n_all += clear.numel()
    print(f"{name}: {n_clear} of {n_all} (row, head) pairs decided by the margin")
    record("memcodes.tokens", case=name, decided=n_clear, pairs=n_all)
    assert n_clear >= 0.95 * n_all


@pytest.mark.parametrize("name", NAMES)
def test_embedding_and_reconstruction_are_consistent(name):
    from fourm.vq import engine as E
    c, sd, m, xs, g = case(name)
    H, d = c["heads"], c["latent"] // c["heads"]
    _, values = E.memcodes_tables(m.quantize)
    for tag, B, h, w in M.INPUTS:
        x = xs[tag].cuda()
        quant, _, tokens = m.encode(x)
        want = torch.stack([values[hh][tokens[:, hh]] for hh in range(H)], dim=1)           # (B, H, h, w, d)
        assert torch.equal(quant, want.permute(0, 1, 4, 2, 3).reshape(B, H * d, h, w))       # quant == values[token], bit for bit
        q2, _, t2 = m.quantize(m._last_latents.reshape(B, h, w, -1).permute(0, 3, 1, 2))     # the quantizer called on its own
        assert torch.equal(q2, quant) and torch.equal(t2, tokens)
        with torch.no_grad():
            full, ae = m(x)[0], m.autoencode(x)
        assert torch.equal(full, m.decode_quant(quant)) and torch.equal(ae, full) and tuple(full.shape) == (B, c["channels"], h, w)
        if (h, w) == (1, 1):
            assert torch.equal(m.tokens_to_embedding(tokens), quant)
            assert torch.equal(m.decode_tokens(tokens), full)
        else:
            with pytest.raises(NotImplementedError, match="not an image-shaped latent"):
                m.tokens_to_embedding(tokens)


@pytest.mark.parametrize("name", NAMES)
def test_a_sample_is_the_same_bits_in_any_batch(name):
    c, sd, m, xs, g = case(name)
    x = xs["g1"].cuda()
    quant, _, tokens = m.encode(x)
    dec = m.decode_tokens(tokens)
    q1, _, t1 = m.encode(x[3:4])
    assert torch.equal(t1, tokens[3:4]) and torch.equal(q1, quant[3:4])
    assert torch.equal(m.decode_tokens(t1), dec[3:4]) and torch.equal(m.decode_quant(q1), dec[3:4])
    q2, _, t2 = m.encode(x[3:4].clone())
    assert torch.equal(t2, t1) and torch.equal(q2, q1)


def test_cached_keys_follow_the_parameters():
    """An in-place edit of to_k.weight (version counter) and an edit behind the counters followed by a bump of the engine's weight epoch
    (what FusedAdamW does): the next encode searches the new keys."""
    from fourm.hip import engine as hip_engine
    from fourm.vq import engine as E
    name = "bmlp_small"
    c, sd, _, xs, g = case(name)
    m = build(name)
    x = xs["g1"].cuda()
    t0 = m.tokenize(x)
    z = m._last_latents.reshape(5, c["latent"]).cpu()

    def expect(sign):
        k64, _ = M.keys64(dict(sd, **{"quantize.to_k.weight": sign * sd["quantize.to_k.weight"]}))
        best, margin = M.margins64(M.head_scores64(z, k64))
        assert bool((margin > 2 * M.score_bound(z, k64)).all())
        return best.reshape(5, c["heads"], 1, 1)

    assert torch.equal(t0.cpu(), expect(1.0))
    with torch.no_grad():
        m.quantize.to_k.weight.mul_(-1.0)                                       # the arg-max becomes the arg-min
    t1 = m.tokenize(x)
    assert torch.equal(t1.cpu(), expect(-1.0)) and not torch.equal(t1, t0)
    m.quantize.to_k.weight.data.mul_(-1.0)                                      # behind the version counter: stale until the epoch moves
    hip_engine.bump_weight_epoch()
    t2 = m.tokenize(x)
    assert torch.equal(t2, t0)
    k, _ = E.memcodes_tables(m.quantize)
    assert E.memcodes_tables(m.quantize)[0] is k                                # and the tables are built once per stamp


def test_full_size_geometry():
    """Upstream's global-feature tokenizer as configured (BottleneckMLP/B_6-Wi_1024 both ways, latent 1024 in 8 heads, 8192 codes per
    head, 768 input channels, batch 64; default-initialised weights, no fixture)."""
    from fourm.vq import VQVAE
    torch.manual_seed(0)
    m = VQVAE(enc_type="BottleneckMLP/B_6-Wi_1024", dec_type="BottleneckMLP/B_6-Wi_1024", n_channels=768, latent_dim=1024, num_codebooks=8,
              codebook_size=8192, quant_type="memcodes", patch_proj=False, sync_codebook=False).cuda().eval()
    x = torch.randn(64, 768, 1, 1, device="cuda")
    quant, _, tok = m.encode(x)
    dec = m.decode_tokens(tok)
    assert tuple(tok.shape) == (64, 8, 1, 1) and tuple(quant.shape) == (64, 1024, 1, 1) and tuple(dec.shape) == (64, 768, 1, 1)
    assert int(tok.min()) >= 0 and int(tok.max()) < 8192 and bool(torch.isfinite(dec).all())
    assert torch.equal(m.tokenize(x), tok) and torch.equal(m.decode_tokens(tok), dec)
    assert torch.equal(m.tokenize(x[:6]), tok[:6]) and torch.equal(m.decode_tokens(tok[:6]), dec[:6])
    assert len(tok.reshape(64, 8).unique(dim=0)) > 1                             # the samples do not all share one token tuple
