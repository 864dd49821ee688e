"""fm_memcodes_assign (multi-head inner-product code search, csrc/vq.hip) on a real MI355X against float64, every (row, head).

Bound.  The kernel's score of (row r, head h, key j) is one fp32 fmaf chain over d of z[r, h d + c] * keys[h][j][c] (v_mfma_f32_32x32x2_f32
is exact fp32, one rounding per term; nothing is normalised and upstream's d^-0.5 is left out).  An any-order fp32 dot product is within
gamma_d * sum_c |a_c b_c| <= d u |a| |b| of the exact one (Cauchy-Schwarz), u = 2^-24:      b(r, h, j) = d u |z_h| |k_hj|.
Two scores enter every comparison, so with s64 the float64 scores:
  (1) value: s64[r, h, tok] >= max_j s64[r, h, j] - (b(tok) + b(argmax))  [<= 2 max_j b]   for EVERY (row, head);
  (2) index: tok == argmax64 (lowest index)         for every (row, head) whose float64 top-2 margin exceeds 2 max_j b(r, h, j).
Pairs under that margin are exempt from (2) only, and their share is capped: at most 2 % on unit-variance random data, none on
z_h = 0.7 k_hj + noise.  The float64 scores are computed head by head."""
import pytest
import torch

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


def assign(z, ldz, keys, values, G, want_quant=True):
    """z (R, H d) copied into a (R, ldz) buffer whose pad columns hold NaN; R % G == 0.  Returns tokens (B, H, G), quant (B, H d, G) or
    None, ws_val, ws_idx (H, R, tiles).  One spare element behind tokens and quant must keep its sentinel."""
    ops, L = _ops()
    H, K, d = keys.shape
    R = z.shape[0]
    assert z.shape[1] == H * d and R % G == 0
    B = R // G
    buf = torch.full((R, ldz), float("nan"), device=DEV)
    buf[:, :H * d] = z
    tiles = -(-K // TILE)
    wv, wi = torch.full((H, R, tiles), SENT, device=DEV), torch.full((H, R, tiles), -7, dtype=torch.int32, device=DEV)
    tok = torch.full((B * H * G + 1,), -7, dtype=torch.int64, device=DEV)
    quant = torch.full((B * H * d * G + 1,), SENT, device=DEV) if want_quant else None
    L.check(L.memcodes_assign(ops._p(buf), ldz, ops._p(keys), ops._p(values), K, d, H, R, G, ops._p(wv), ops._p(wi), tiles, ops._p(tok),
                              ops._p(quant), ops._stream()))
    torch.cuda.synchronize()
    assert int(tok[-1]) == -7 and (quant is None or float(quant[-1]) == SENT)
    return tok[:-1].view(B, H, G), (quant[:-1].view(B, H * d, G) if want_quant else None), wv, wi


def check_pairs(name, tok, z, keys, cap):
    """Conditions (1) and (2) of the module docstring for tokens (B, H, G); returns (exempt pairs, worst gap / bound, smallest margin)."""
    H, K, d = keys.shape
    B, _, G = tok.shape
    R = B * G
    assert bool(((tok >= 0) & (tok < K)).all()), name
    n_ex, worst, mmin, mism = 0, 0.0, float("inf"), 0
    for h in range(H):
        zh, kh = z[:, h * d:(h + 1) * d].double(), keys[h].double()
        s64 = zh @ kh.t()                                                       # (R, K)
        t = tok[:, h, :].reshape(R)
        zn, kn = zh.norm(dim=1), kh.norm(dim=1)
        best = s64.argmax(1)                                                    # (torch.argmax: the lowest index of equal maxima)
        top = s64.topk(min(2, K), dim=1).values
        margin = top[:, 0] - top[:, 1] if K > 1 else torch.full((R,), float("inf"), dtype=torch.float64, device=DEV)
        gap = top[:, 0] - s64.gather(1, t[:, None])[:, 0]
        bound1 = d * U * zn * (kn[t] + kn[best])
        bound2 = 2 * d * U * zn * kn.max()
        ok1 = gap <= bound1
        assert bool(ok1.all()), f"{name} head {h}: {int((~ok1).sum())} rows with a score below the maximum by more than the bound, worst {float((gap / bound1.clamp_min(1e-300)).max()):.3g}"
        exempt = margin <= bound2
        wrong = (t != best) & ~exempt
        assert not bool(wrong.any()), f"{name} head {h}: {int(wrong.sum())} rows off the float64 arg-max at a margin above 2 b"
        nz = bound1 > 0
        if bool(nz.any()):
            worst = max(worst, float((gap[nz] / bound1[nz]).max()))
        n_ex += int(exempt.sum())
        mmin = min(mmin, float(margin.min()))
        mism += int((t != best).sum())
    print(f"{name}: worst value gap / bound {worst:.3g}, pairs under the margin {n_ex} of {R * H}, smallest margin {mmin:.3g}, index mismatches {mism}")
    assert n_ex <= cap * R * H, f"{name}: {n_ex} of {R * H} (row, head) pairs are near ties (cap {cap})"
    return n_ex, worst, mmin


def expected_quant(tok, values):
    """quant[b][h d + c][g] = values[h][tok[b, h, g]][c]."""
    H, K, d = values.shape
    B, _, G = tok.shape
    picked = torch.stack([values[h][tok[:, h, :]] for h in range(H)], dim=1)    # (B, H, G, d)
    return picked.permute(0, 1, 3, 2).reshape(B, H * d, G)


# (H, d, K): the pose shape, the global-feature shape (R = 129 only), d below one 32-wide staging step with a partial code tile, d no multiple
# of 32, one code past a tile, a single key
SHAPES = [(8, 128, 1024), (8, 128, 8192), (4, 16, 50), (3, 36, 300), (2, 64, 129), (1, 8, 1)]
CASES = [(s, R) for s in SHAPES for R in (1, 129, 777) if s != (8, 128, 8192) or R == 129]


@pytest.mark.parametrize("shape,R", CASES, ids=[f"H{s[0]}-d{s[1]}-K{s[2]}-R{R}" for s, R in CASES])
@pytest.mark.parametrize("kind", ["random", "near_key"])
def test_memcodes_assign_against_float64(kind, shape, R):
    H, d, K = shape
    keys, values = randn(H, K, d, seed=100 + d + K), randn(H, K, d, seed=200 + d + K)
    if kind == "random":
        z = randn(R, H * d, seed=3 + R)
        cap = 0.02
    else:                                                                       # z_h = 0.7 k_hj + noise of length ~0.3 |k|
        g = torch.Generator().manual_seed(5 + R)
        j = torch.randint(0, K, (R, H), generator=g).to(DEV)
        z = 0.7 * torch.stack([keys[h][j[:, h]] for h in range(H)], dim=1).reshape(R, H * d) + randn(R, H * d, scale=0.3, seed=4 + R)
        cap = 0.0
    ldz = H * d + 4 if R == 777 else H * d                                      # a padded row stride, NaN in the pad columns
    G = 3 if R % 3 == 0 else 1                                                  # several tokens per image: the head-major layouts
    want_quant = kind == "random" or R == 129                                   # quant given in some calls, NULL in others
    tok, quant, _, _ = assign(z, ldz, keys, values, G, want_quant)
    n_ex, worst, mmin = check_pairs(f"memcodes {kind} H={H} d={d} K={K} R={R}", tok, z, keys, cap)
    if want_quant:
        assert torch.equal(quant, expected_quant(tok, values))                  # the gathered value rows, exactly
    else:
        assert quant is None
    record("memcodes.assign", kind=kind, H=H, d=d, K=K, R=R, near_tie_pairs=n_ex, worst_gap_over_bound=worst, smallest_margin=mmin)


def test_memcodes_assign_duplicate_keys_lowest_index_wins():
    """Exact duplicates at i < j, searched with the key itself (|k|^2 ~ d = 64 against ~ 3.3 sqrt(d) for the best other key): i wins with
    bit-identical scores.  The pairs sit in one lane's registers (8, 9), in the two lane halves of one 32-key tile (10, 20), in the two 32-key tiles of a wave (3, 40), in the two wave pairs of
    a block (50, 100), in two blocks (200, 700) and at the last, partial tile (130, 999); the second head holds them shifted by one."""
    H, d, K = 2, 64, 1000
    keys, values = randn(H, K, d, seed=80), randn(H, K, d, seed=82)
    pairs = [(8, 9), (10, 20), (3, 40), (50, 100), (200, 700), (130, 998)]
    for h in range(H):
        for i, j in pairs:
            keys[h, j + h] = keys[h, i + h]
    z = torch.cat([torch.stack([torch.cat([keys[h, j + h] for h in range(H)]) for _, j in pairs]), randn(20, H * d, seed=81)]).contiguous()
    tok, quant, wv, wi = assign(z, H * d, keys, values, 1)
    for h in range(H):
        assert tok[:6, h, 0].tolist() == [i + h for i, _ in pairs]
        for r, (i, j) in enumerate(pairs):
            if (i + h) // TILE != (j + h) // TILE:                              # both tiles report the same score, bit for bit
                assert float(wv[h, r, (i + h) // TILE]) == float(wv[h, r, (j + h) // TILE])
                assert int(wi[h, r, (i + h) // TILE]) == i + h and int(wi[h, r, (j + h) // TILE]) == j + h
    assert torch.equal(quant, expected_quant(tok, values))
    check_pairs("memcodes duplicates", tok, z, keys, 13 / (z.shape[0] * H))     # the 12 duplicate pairs are exact float64 ties by construction (+ at most one random pair)


def test_memcodes_assign_zero_row_negative_scores_and_reproducibility():
    H, d, K, R = 4, 16, 300, 200
    keys, values = randn(H, K, d, seed=1).abs() + 0.1, randn(H, K, d, seed=2)   # positive keys, negative latents: every score is negative
    z = -(randn(R, H * d, seed=3).abs() + 0.1)
    z[1] = 0.0                                                                  # zero latent: every score 0, key 0 wins in every head
    tok, quant, wv, wi = assign(z, H * d, keys, values, 1)
    assert tok[1, :, 0].tolist() == [0] * H
    assert bool((wv[:, [0] + list(range(2, R))] < 0).all())
    check_pairs("memcodes negative scores", tok, z, keys, 0.02)
    tok2, quant2, wv2, wi2 = assign(z, H * d, keys, values, 1)
    assert torch.equal(tok, tok2) and torch.equal(quant, quant2) and torch.equal(wv, wv2) and torch.equal(wi, wi2)
    tok3, none, _, _ = assign(z, H * d, keys, values, 1, want_quant=False)
    assert none is None and torch.equal(tok, tok3)


def test_memcodes_assign_heads_do_not_leak():
    """The middle head between neighbours whose columns (and keys) hold huge values: its tokens are those of the same columns searched
    alone, and its quant slice the middle value table's rows."""
    H, d, K, R = 3, 16, 50, 150
    keys, values = randn(H, K, d, seed=5), randn(H, K, d, seed=6)
    z = randn(R, H * d, seed=7)
    z[:, :d] = 1e30
    z[:, 2 * d:] = -1e30
    keys[0] *= 1e6
    keys[2] *= 1e6
    tok, quant, _, _ = assign(z, H * d + 4, keys, values, 3)
    alone, q_alone, _, _ = assign(z[:, d:2 * d].contiguous(), d, keys[1:2].contiguous(), values[1:2].contiguous(), 3)
    assert torch.equal(tok[:, 1], alone[:, 0]) and torch.equal(quant[:, d:2 * d], q_alone)
    check_pairs("memcodes middle head", alone, z[:, d:2 * d], keys[1:2], 0.02)
    assert bool(torch.isfinite(quant).all())


def test_memcodes_assign_refuses_bad_arguments():
    ops, L = _ops()
    H, d, K, R = 2, 32, 300, 10
    keys, values, z = randn(H, K, d, seed=1), randn(H, K, d, seed=2), randn(R, 72, seed=3)
    tiles = -(-K // TILE)
    wv, wi = torch.empty(H, R, tiles, device=DEV), torch.empty(H, R, tiles, dtype=torch.int32, device=DEV)
    tok = torch.full((R * H,), -7, dtype=torch.int64, device=DEV)

    def call(z_=z, ldz=72, keys_=keys, values_=values, K_=K, d_=d, H_=H, R_=R, G=R, tiles_=tiles, wv_=wv, wi_=wi, tok_=tok):
        return L.memcodes_assign(ops._p(z_), ldz, ops._p(keys_), ops._p(values_), K_, d_, H_, R_, G, ops._p(wv_), ops._p(wi_), tiles_, ops._p(tok_), None,
                                 ops._stream())

    def refused(rc, text):
        assert rc != 0, "the launcher accepted a bad argument"
        msg = L.lib.fm_last_error().decode()
        assert text in msg, msg

    for bad in ("z_", "keys_", "values_", "wv_", "wi_", "tok_"):
        refused(call(**{bad: None}), "null pointer")
    refused(call(d_=6), "d=6 unsupported")
    refused(call(d_=4), "d=4 unsupported")
    refused(call(d_=34), "d=34 unsupported")
    refused(call(d_=4100, H_=1, ldz=4100), "d=4100 unsupported")
    refused(call(H_=0), "bad shape")
    refused(call(K_=0), "bad shape")
    refused(call(R_=0), "bad shape")
    refused(call(G=0), "bad shape")
    refused(call(ldz=70), "bad row stride")
    refused(call(ldz=60), "bad row stride")                                     # ldz < H d
    refused(call(z_=z.reshape(-1)[1:]), "16-byte aligned")
    refused(call(keys_=keys.reshape(-1)[1:]), "16-byte aligned")
    refused(call(tiles_=tiles + 1), "code_tiles")
    refused(call(R_=65536 * TILE), "grid too large")
    refused(call(H_=65536, d_=8, ldz=65536 * 8), "grid too large")
    torch.cuda.synchronize()
    assert bool((tok == -7).all())                                              # nothing was launched
    L.check(call())
    torch.cuda.synchronize()
    assert bool(((tok >= 0) & (tok < K)).all())
