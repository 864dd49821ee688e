"""fm_vq_assign_wide (cosine code search for any latent width, csrc/vq.hip) on a real MI355X against float64, every row.

Bound.  The kernel's score of (row r, code k) is an fp32 fmaf chain over d of l2norm(z_r)[d] * En[k][d] (v_mfma_f32_32x32x2_f32 is
exact fp32, one rounding per term).  For unit vectors an any-order fp32 dot product is within gamma_D * sum_d |a_d b_d| <= D u of the exact
one (Cauchy-Schwarz), u = 2^-24; the two normalisations (sum of squares, square root, division, one multiply per element, on each side)
add at most 8 u:      bound = (D + 8) u.
Two scores enter every comparison, so with s64 the float64 cosine scores:
  (1) value: s64[r, tok[r]] >= max_k s64[r, k] - 2 bound                    for EVERY row;
  (2) index: tok[r] == argmax64[r] (lowest index)                            for every row whose float64 top-2 margin exceeds 2 bound.
Rows under that margin are exempt from (2) only, and their share is capped: at most 2 % of the rows on unit-variance random latents, none
on latents 0.7 e_j + noise."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests.parity_log import record

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -24
SENT = 7.0
TILE = 128


def _ops():
    from fourm.hip import ops, _lib
    return ops, _lib


def randn(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def normalized_codes(embed):
    """The image the engine caches: fm_l2norm_rows of the codebook."""
    ops, L = _ops()
    en = torch.empty_like(embed)
    L.check(L.l2norm_rows(ops._p(embed), embed.stride(0), ops._p(en), en.stride(0), embed.shape[0], embed.shape[1], ops._stream()))
    return en


def assign_wide(z, ldz, en, embed, G, want_quant=True):
    """z (R, D) copied into a (R, ldz) buffer whose pad columns hold NaN; returns tokens (R), quant (nb, D, G) or None, ws_val, ws_idx."""
    ops, L = _ops()
    R, D = z.shape
    K = embed.shape[0]
    buf = torch.full((R, ldz), float("nan"), device=DEV)
    buf[:, :D] = z
    tiles = -(-K // TILE)
    wv, wi = torch.full((R, tiles), SENT, device=DEV), torch.full((R, tiles), -7, dtype=torch.int32, device=DEV)
    tok = torch.full((R + 1,), -7, dtype=torch.int64, device=DEV)
    nb = (R + G - 1) // G
    quant = torch.full((nb, D, G), SENT, device=DEV) if want_quant else None
    L.check(L.vq_assign_wide(ops._p(buf), ldz, ops._p(en), ops._p(embed), K, D, R, G, ops._p(wv), ops._p(wi), tiles, ops._p(tok), ops._p(quant),
                             ops._stream()))
    torch.cuda.synchronize()
    assert int(tok[R]) == -7
    return tok[:R], quant, wv, wi


def scores64(z, embed):
    z64, e64 = F.normalize(z.double(), dim=-1), F.normalize(embed.double(), dim=-1)
    out = torch.empty(z.shape[0], embed.shape[0], dtype=torch.float64, device=DEV)
    for i in range(0, z.shape[0], 1024):
        out[i:i + 1024] = z64[i:i + 1024] @ e64.t()
    return out


def check_rows(name, tok, s64, D, cap):
    """Conditions (1) and (2) of the module docstring; returns (exempt rows, worst value gap / (2 bound), smallest margin)."""
    R, K = s64.shape
    bound = (D + 8) * U
    assert bool(((tok >= 0) & (tok < K)).all()), name
    top = s64.topk(min(2, K), dim=1)
    best = s64.argmax(1)                                                      # (torch.argmax: the lowest index of equal maxima)
    margin = top.values[:, 0] - top.values[:, 1] if K > 1 else torch.full((R,), float("inf"), dtype=torch.float64, device=DEV)
    gap = top.values[:, 0] - s64.gather(1, tok[:, None])[:, 0]
    worst = float(gap.max() / (2 * bound))
    exempt = margin <= 2 * bound
    n_ex = int(exempt.sum())
    print(f"{name}: worst value gap / (2 bound) {worst:.3g}, rows under the margin {n_ex} of {R}, smallest margin {float(margin.min()):.3g}, "
          f"index mismatches {int((tok != best).sum())}")
    assert bool((gap <= 2 * bound).all()), f"{name}: {int((gap > 2 * bound).sum())} rows with a score below the maximum by more than 2 bound, worst ratio {worst:.3g}"
    wrong = (tok != best) & ~exempt
    assert not bool(wrong.any()), f"{name}: {int(wrong.sum())} rows off the float64 arg-max at a margin above 2 bound"
    assert n_ex <= cap * R, f"{name}: {n_ex} of {R} rows are near ties (cap {cap})"
    return n_ex, worst, float(margin.min())


SHAPES = [(1024, 1024), (128, 8192), (64, 300), (8, 37), (1024, 1)]
ROWS = [1, 6144, 777]


@pytest.mark.parametrize("R", ROWS)
@pytest.mark.parametrize("D,K", SHAPES)
@pytest.mark.parametrize("kind", ["random", "near_code"])
def test_assign_wide_against_float64(kind, D, K, R):
    embed = randn(K, D, seed=100 + D + K)
    en = normalized_codes(embed)
    if kind == "random":
        z = randn(R, D, seed=3 + R)
        cap = 0.02
    else:                                                                       # 0.7 e_j + noise of length ~0.3
        g = torch.Generator().manual_seed(5 + R)
        j = torch.randint(0, K, (R,), generator=g).to(DEV)
        z = 0.7 * en[j] + randn(R, D, scale=0.3 / math.sqrt(D), seed=4 + R)
        cap = 0.0
    ldz = D + 4 if R == 777 else D                                              # a padded row stride, NaN in the pad columns
    G = 16 if R % 16 == 0 else R
    tok, quant, _, _ = assign_wide(z, ldz, en, embed, G)
    s64 = scores64(z, embed)
    n_ex, worst, mmin = check_rows(f"wide {kind} D={D} K={K} R={R}", tok, s64, D, cap)
    q = quant.permute(0, 2, 1).reshape(-1, D)
    assert torch.equal(q[:R], embed[tok])                                       # the gathered table rows, exactly
    assert bool((q[R:] == SENT).all())
    if kind == "near_code" and K > 1 and D >= 64:
        assert float((tok == j).float().mean()) > 0.99
    record("vq_wide.assign", kind=kind, D=D, K=K, R=R, near_tie_rows=n_ex, worst_gap_over_2bound=worst, smallest_margin=mmin)


def test_assign_wide_without_quant_and_zero_row():
    D, K, R = 1024, 1024, 300
    embed = randn(K, D, seed=1)
    en = normalized_codes(embed)
    z = randn(R, D, seed=2)
    z[1] = 0.0                                                                  # zero latent: every score 0, code 0 wins
    tok, quant, _, _ = assign_wide(z, D, en, embed, R, want_quant=False)
    assert quant is None and int(tok[1]) == 0
    tok2, _, _, _ = assign_wide(z, D, en, embed, R)
    assert torch.equal(tok, tok2)


def test_assign_wide_duplicate_codes_lowest_index_wins():
    """Exact duplicates at i < j: i wins with bit-identical scores.  The pairs sit in one lane's registers (8, 9), in the two lane halves of
    one 32-code tile (10, 20), in the two 32-code tiles of a wave (3, 40), in the two wave pairs of a block (50, 100), in two blocks
    (200, 700) and at the last, partial tile (130, 999)."""
    D, K = 1024, 1000
    embed = randn(K, D, seed=80)
    pairs = [(8, 9), (10, 20), (3, 40), (50, 100), (200, 700), (130, 999)]
    for i, j in pairs:
        embed[j] = embed[i]
    en = normalized_codes(embed)
    z = torch.cat([torch.stack([embed[j] * 2.5 for _, j in pairs]), torch.stack([embed[i] for i, _ in pairs]), randn(20, D, seed=81)]).contiguous()
    tok, quant, wv, wi = assign_wide(z, D, en, embed, z.shape[0])
    want = [i for i, _ in pairs] * 2
    assert tok[:12].tolist() == want
    for r, (i, j) in enumerate(pairs):
        if i // TILE != j // TILE:                                              # both tiles report the same score, bit for bit
            assert float(wv[r, i // TILE]) == float(wv[r, j // TILE]) and int(wi[r, i // TILE]) == i and int(wi[r, j // TILE]) == j
    s64 = scores64(z, embed)
    check_rows("wide duplicates", tok, s64, D, 13 / z.shape[0])                 # the 12 duplicate rows are exact float64 ties by construction (+ at most one of the 20 random rows)


def test_assign_wide_is_bit_reproducible():
    D, K, R = 1024, 1024, 6144
    embed, z = randn(K, D, seed=7), randn(R, D, seed=8)
    en = normalized_codes(embed)
    a = assign_wide(z, D, en, embed, 16)
    b = assign_wide(z, D, en, embed, 16)
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3]) and torch.equal(a[1], b[1])


def test_assign_wide_refuses_bad_arguments():
    ops, L = _ops()
    D, K, R = 64, 300, 10
    embed, z = randn(K, D, seed=1), randn(R, 72, seed=2)
    en = normalized_codes(embed)
    tiles = -(-K // TILE)
    wv, wi = torch.empty(R, tiles, device=DEV), torch.empty(R, tiles, dtype=torch.int32, device=DEV)
    tok = torch.full((R,), -7, dtype=torch.int64, device=DEV)

    def call(z_=z, ldz=72, en_=en, K_=K, D_=D, R_=R, G=R, tiles_=tiles):
        return L.vq_assign_wide(ops._p(z_), ldz, ops._p(en_), ops._p(embed), K_, D_, R_, G, ops._p(wv), ops._p(wi), tiles_, ops._p(tok), None, ops._stream())

    def refused(rc, text):
        assert rc != 0, "the launcher accepted a bad argument"
        msg = L.lib.fm_last_error().decode()
        assert text in msg, msg

    refused(call(D_=6), "latent_dim=6 unsupported")
    refused(call(D_=4), "latent_dim=4 unsupported")
    refused(call(D_=4100, ldz=4100), "latent_dim=4100 unsupported")
    refused(call(D_=66), "latent_dim=66 unsupported")
    refused(call(K_=0), "bad shape")
    refused(call(R_=0), "bad shape")
    refused(call(ldz=70), "bad shape")
    refused(call(ldz=60), "bad shape")
    refused(call(G=0), "bad shape")
    refused(call(tiles_=tiles + 1), "code_tiles")
    refused(call(z_=None), "null pointer")
    refused(call(z_=z.reshape(-1)[1:]), "16-byte aligned")
    torch.cuda.synchronize()
    assert bool((tok == -7).all())                                              # nothing was launched
    L.check(call())
    torch.cuda.synchronize()
    assert bool(((tok >= 0) & (tok < K)).all())
    # the 32-wide entry point keeps refusing other widths
    refused(L.vq_assign(ops._p(z), 72, ops._p(en), ops._p(embed), K, D, R, R, 1, ops._p(wv), ops._p(wi), 1, ops._p(tok), None, ops._stream()),
            "latent_dim=64 unsupported (this build handles 32)")


def test_engine_dispatch_by_latent_width(monkeypatch):
    """_assign: latent_dim == 32 keeps calling fm_vq_assign (tokens of the vq_small fixture unchanged), any other width with the cosine
    codebook calls fm_vq_assign_wide."""
    import numpy as np
    from fourm.vq import engine as E
    from tests.test_vq import build, case
    calls = []
    real_narrow, real_wide = E.L.vq_assign, E.L.vq_assign_wide
    monkeypatch.setattr(E.L, "vq_assign", lambda *a: (calls.append("narrow"), real_narrow(*a))[1])
    monkeypatch.setattr(E.L, "vq_assign_wide", lambda *a: (calls.append("wide"), real_wide(*a))[1])
    c, cfg, sd, x, g = case("vq_small")
    m = build(c, cfg)
    m.load_state_dict(sd)
    m = m.cuda().eval()
    tokens = m.tokenize(x.cuda())
    assert calls == ["narrow"]
    agree = float((tokens.cpu() == torch.from_numpy(g["tokens"]).long()).float().mean())
    assert agree > 0.9, agree
    z = torch.from_numpy(g["latents"]).reshape(-1, cfg.latent).cuda().contiguous()          # upstream's latents: upstream's tokens exactly
    eng = E._engine(m.encoder)
    B = c["batch"]
    tok = E._assign(m, eng, z, z.shape[0], cfg.grid ** 2, B, cfg.grid, cfg.grid, False)
    assert np.array_equal(tok.cpu().numpy(), g["tokens"]) and calls == ["narrow", "narrow"]
    from fourm.vq import VQ
    w = VQ(image_size=32, enc_type="vit_s_enc", patch_size=8, post_mlp=True, codebook_size=300, latent_dim=64, norm_codes=True, sync_codebook=False).cuda().eval()
    calls.clear()
    t = w.tokenize(torch.rand(3, 3, 32, 32, device=DEV) * 2 - 1)
    assert calls == ["wide"] and tuple(t.shape) == (3, 4, 4) and int(t.max()) < 300
