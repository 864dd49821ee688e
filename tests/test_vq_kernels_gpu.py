"""Per-kernel numerics of the VQ tokenizer on a real MI355X: every entry point of csrc/vq.hip against a float64 (or exact) restatement of
the upstream operation it replaces, on the same fp32 inputs.  The end-to-end VQ-VAE fixtures (tests/test_vqvae.py) bound whole-model
outputs at the 1e-2 level; here each kernel is held, element by element, to a bound derived from the fp32 unit roundoff u = 2^-24 and
written next to its check, so a lost gradient term, a missing projection, a leaking pad column or a wrong index fails by orders of
magnitude.  Pad columns of every output start as a sentinel and must stay so; pad columns the kernel must not read hold NaN.  Also: the
split3 GEMM (fm_split3_bf16 + one bf16 NT GEMM over 3 K columns, the tokenizer's fp32 tail at inference) measured against its stated
accuracy."""
import pytest
import torch
import torch.nn.functional as F

from tests.parity_log import record

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -24           # fp32 unit roundoff
FN = 2.0 ** -20          # a few ulps of tanhf / sqrtf / division
ETA = 2.0 ** -126        # smallest normal fp32: results below it may be flushed to zero
SENT = 7.0


def _ops():
    from fourm.hip import ops, _lib
    return ops, _lib


def randn(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def randint(lo, hi, shape, seed=0):
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    return torch.randint(lo, hi, shape, generator=g).to(DEV)


def check(name, got, ref, tol):
    """|got - ref| <= tol element-wise (float64); returns the worst err / tol."""
    err = (got.double() - ref).abs()
    bad = ~(err <= tol)
    ratio = float((err / (tol + 1e-300)).max()) if err.numel() else 0.0
    assert not bool(bad.any()), f"{name}: {int(bad.sum())} of {err.numel()} outside the bound, worst err/tol {ratio:.3g}"
    return ratio


def padded(src, ld, offset=0, fill=0.0):
    """src (rows, cols) copied into a (rows, ld) buffer at column ``offset``; returns the (rows, cols) view."""
    buf = torch.full((src.shape[0], ld), fill, device=DEV, dtype=src.dtype)
    buf[:, offset:offset + src.shape[1]] = src
    return buf[:, offset:offset + src.shape[1]]


def sentinel_rows(rows, cols, ld, dtype=torch.float32):
    """(rows + 1, ld) buffer full of the sentinel and its (rows, cols) view."""
    buf = torch.full((rows + 1, ld), SENT, device=DEV, dtype=dtype)
    return buf, buf[:rows, :cols]


def untouched(buf, rows, cols):
    mask = torch.ones(buf.shape, dtype=torch.bool, device=buf.device)
    mask[:rows, :cols] = False
    return bool((buf[mask] == SENT).all())


def refused(rc, text):
    _, L = _ops()
    assert rc != 0, "the launcher accepted a bad argument"
    msg = L.lib.fm_last_error().decode()
    assert text in msg, msg


def patchify64(img, P):
    """rearrange(img, 'b c (h p) (w q) -> (b h w) (c p q)')   (vit_models.py:402-405: Conv2d(k = s = P) as a GEMM)"""
    B, C, H, W = img.shape
    return img.reshape(B, C, H // P, P, W // P, P).permute(0, 2, 4, 1, 3, 5).reshape(B * (H // P) * (W // P), C * P * P)


def unpatchify64(rows, B, C, H, W, P):
    """rearrange(rows, '(b nh nw) (c ph pw) -> b c (nh ph) (nw pw)')   (vit_models.py:640-643)"""
    return rows.reshape(B, H // P, W // P, C, P, P).permute(0, 3, 1, 4, 2, 5).reshape(B, C, H, W)


# ------------------------------------------------------------------------------------------------
# fm_vq_patchify / fm_vq_patchify_ex / fm_vq_unpatchify
# ------------------------------------------------------------------------------------------------
PATCH_SHAPES = [  # B, C, H, W, P, extra pad columns
    (2, 3, 32, 48, 8, 5), (1, 19, 16, 12, 4, 3), (3, 1, 32, 16, 16, 64), (2, 3, 5, 7, 1, 1), (1, 19, 32, 32, 16, 0),
    (5, 1, 224, 224, 1, 1),          # 250880 rows > 8192 blocks x 4 waves: the grid-stride loop runs
]


@pytest.mark.parametrize("B,C,H,W,P,extra", PATCH_SHAPES)
def test_patchify_bitwise(B, C, H, W, P, extra):
    """fm_vq_patchify == rearrange(...).bfloat16() bit for bit; columns [C P P, ld_out) exactly 0; the row past the end untouched."""
    ops, L = _ops()
    img = randn(B, C, H, W, seed=B * 7 + C + H + W + P)
    Fc, R = C * P * P, B * (H // P) * (W // P)
    buf, out = sentinel_rows(R, Fc + extra, Fc + extra, torch.bfloat16)
    L.check(L.vq_patchify(ops._p(img), ops._p(buf), buf.stride(0), B, C, H, W, P, ops._stream()))
    assert torch.equal(out[:, :Fc], patchify64(img, P).bfloat16())
    assert bool((out[:, Fc:] == 0).all())
    assert untouched(buf, R, Fc + extra)


def test_patchify_ex_pixels_scale_shift():
    """undo_std form (vqvae.py:269-286 folded into the gather): s[c] v + h[c], possibly contracted to one FMA (2 u of the terms), then one
    bf16 rounding (2^-8 of the fp32 value, which itself is within 2 u of the terms of ref):
        |out - ref| <= 2^-8 |ref| + 3 u (|s v| + |h|)."""
    ops, L = _ops()
    B, C, H, W, P, ld = 2, 3, 32, 48, 8, 3 * 64 + 6
    img = randn(B, C, H, W, seed=11)
    scale, shift = randn(C, seed=12).abs() + 0.5, randn(C, seed=13)
    R, Fc = B * (H // P) * (W // P), C * P * P
    buf, out = sentinel_rows(R, ld, ld, torch.bfloat16)
    L.check(L.vq_patchify_ex(ops._p(img), None, None, ops._p(scale), ops._p(shift), ops._p(buf), ld, B, C, H, W, P, ops._stream()))
    sv = scale.double().view(1, C, 1, 1) * img.double()
    h = shift.double().view(1, C, 1, 1).expand_as(sv)
    ref = patchify64(sv + h, P)
    r = check("patchify_ex scale/shift", out[:, :Fc], ref, 2.0 ** -8 * ref.abs() + 3 * U * (patchify64(sv.abs(), P) + patchify64(h.abs(), P)))
    assert bool((out[:, Fc:] == 0).all()) and untouched(buf, R, ld)
    record("vq_kernels.patchify_ex", worst_err_over_tol=r)


@pytest.mark.parametrize("with_affine", [False, True])
@pytest.mark.parametrize("P", [1, 4, 8])
def test_patchify_ex_labels(P, with_affine):
    """Semantic-segmentation input (vqvae.py:141-146, :281-284): cls_emb[labels] gathered per pixel; bitwise without the affine map."""
    ops, L = _ops()
    B, C, H, W, n_labels = 2, 5, 16, 24, 7
    labels = randint(0, n_labels, (B, H, W), seed=20 + P)
    labels[0, 0, 0], labels[1, H - 1, W - 1] = 0, n_labels - 1
    emb = randn(n_labels, C, seed=21)
    scale, shift = (randn(C, seed=22).abs() + 0.5, randn(C, seed=23)) if with_affine else (None, None)
    R, Fc = B * (H // P) * (W // P), C * P * P
    ld = Fc + 9
    buf, out = sentinel_rows(R, ld, ld, torch.bfloat16)
    L.check(L.vq_patchify_ex(None, ops._p(labels), ops._p(emb), ops._p(scale), ops._p(shift), ops._p(buf), ld, B, C, H, W, P, ops._stream()))
    v = emb.double()[labels].permute(0, 3, 1, 2)                             # (B, C, H, W)
    if not with_affine:
        assert torch.equal(out[:, :Fc], patchify64(v, P).bfloat16())
    else:
        sv = scale.double().view(1, C, 1, 1) * v
        h = shift.double().view(1, C, 1, 1).expand_as(sv)
        ref = patchify64(sv + h, P)
        check("patchify_ex labels+affine", out[:, :Fc], ref, 2.0 ** -8 * ref.abs() + 3 * U * (patchify64(sv.abs(), P) + patchify64(h.abs(), P)))
    assert bool((out[:, Fc:] == 0).all()) and untouched(buf, R, ld)


def test_patchify_ex_refusals():
    ops, L = _ops()
    B, C, H, W, P = 1, 3, 8, 8, 4
    img, labels, emb, s = randn(B, C, H, W), randint(0, 3, (B, H, W)), randn(3, C), randn(C)
    out = torch.zeros(4, C * P * P, dtype=torch.bfloat16, device=DEV)
    args = (ops._p(out), C * P * P, B, C, H, W, P, ops._stream())
    refused(L.vq_patchify_ex(None, ops._p(labels), None, None, None, *args), "pass pixels (img) or class ids")
    refused(L.vq_patchify_ex(None, None, None, None, None, *args), "pass pixels (img) or class ids")
    refused(L.vq_patchify_ex(ops._p(img), None, None, ops._p(s), None, *args), "scale and shift go together")
    refused(L.vq_patchify_ex(ops._p(img), None, None, None, ops._p(s), *args), "scale and shift go together")
    assert bool((out == 0).all())


@pytest.mark.parametrize("B,C,H,W,P,extra", [(2, 3, 32, 48, 8, 5), (1, 19, 16, 12, 4, 3), (2, 3, 5, 7, 1, 2),
                                             (2, 3, 896, 896, 16, 4)])       # 4.8 M pixels > 256 x 16384: the grid clamp is hit
def test_unpatchify_bitwise_and_round_trip(B, C, H, W, P, extra):
    """fm_vq_unpatchify is the exact inverse rearrange; NaN in the row pad columns never reaches the image; unpatchify(patchify(x)) == x
    for bf16-representable x."""
    ops, L = _ops()
    Fc, R = C * P * P, B * (H // P) * (W // P)
    rows = padded(randn(R, Fc, seed=30 + C + P), Fc + extra, fill=float("nan"))
    n = B * C * H * W
    ibuf = torch.full((n + 64,), SENT, device=DEV)
    img = ibuf[:n].view(B, C, H, W)
    L.check(L.vq_unpatchify(ops._p(rows), rows.stride(0), ops._p(img), B, C, H, W, P, ops._stream()))
    assert torch.equal(img, unpatchify64(rows, B, C, H, W, P))
    assert bool((ibuf[n:] == SENT).all())
    # round trip through the bf16 patch rows
    x = randn(B, C, H, W, seed=31).bfloat16().float()
    pr = torch.zeros(R, Fc + extra, dtype=torch.bfloat16, device=DEV)
    L.check(L.vq_patchify(ops._p(x), ops._p(pr), pr.stride(0), B, C, H, W, P, ops._stream()))
    prf = pr.float()
    back = torch.empty_like(x)
    L.check(L.vq_unpatchify(ops._p(prf), prf.stride(0), ops._p(back), B, C, H, W, P, ops._stream()))
    assert torch.equal(back, x)


# ------------------------------------------------------------------------------------------------
# fm_l2norm_rows, fm_vq_code_bias
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,D", [(1000, 8), (1000, 32), (1000, 33), (40000, 64), (300, 384)])
def test_l2norm_rows(R, D):
    """F.normalize(x, dim=-1) = x / max(|x|, 1e-12).  sum of squares: gamma_D relative; sqrt, reciprocal, product: u each:
        |y - ref| <= (D + 4) u |ref| + ETA.
    A zero row gives exact zeros; a row of norm ~1e-15 takes the eps branch (y = x / 1e-12), as torch does."""
    ops, L = _ops()
    x0 = randn(R, D, seed=40 + D)
    x0[0] = 0.0
    x0[1] = x0[1] / x0[1].norm() * 1e-15
    x = padded(x0, D + 3, fill=float("nan"))
    buf, y = sentinel_rows(R, D, D + 5)
    L.check(L.l2norm_rows(ops._p(x), x.stride(0), ops._p(y), buf.stride(0), R, D, ops._stream()))
    x64 = x0.double()
    ref = x64 / x64.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    r = check(f"l2norm D={D}", y, ref, (D + 4) * U * ref.abs() + ETA)
    assert bool((y[0] == 0).all())
    assert float(y[1].double().norm()) < 1e-2                              # the eps branch: |y| = 1e-15 / 1e-12
    assert untouched(buf, R, D)
    record("vq_kernels.l2norm_rows", D=D, worst_err_over_tol=r)


@pytest.mark.parametrize("K", [1, 255, 256, 16385])
@pytest.mark.parametrize("D", [8, 32])
def test_code_bias(K, D):
    """bias[k] = -|e_k|^2 / 2 (EuclideanCodebook distance, quantize_lucid.py:272-278): a D-term FMA chain, then an exact halving:
        |bias - ref| <= gamma_D |ref| <= (D + 1) u |ref|."""
    ops, L = _ops()
    e = randn(K, D, seed=50 + K + D)
    bbuf = torch.full((K + 4,), SENT, device=DEV)
    L.check(L.vq_code_bias(ops._p(e), K, D, ops._p(bbuf), ops._stream()))
    ref = -0.5 * e.double().pow(2).sum(1)
    r = check(f"code_bias K={K} D={D}", bbuf[:K], ref, (D + 1) * U * ref.abs())
    assert bool((bbuf[K:] == SENT).all())
    record("vq_kernels.code_bias", K=K, D=D, worst_err_over_tol=r)


# ------------------------------------------------------------------------------------------------
# fm_vq_assign / fm_vq_assign_bias
# ------------------------------------------------------------------------------------------------
ASSIGN_CASES = [  # R, K, splits, ldz, normalize
    (1, 1, 1, 32, 1), (1, 1, 4, 36, 0), (255, 3, 3, 32, 1), (257, 64, 64, 36, 1),      # K = 64, splits = 64: splits 16-63 scan nothing
    (257, 64, 16, 32, 0), (255, 255, 3, 36, 1), (12547, 1000, 16, 32, 1), (12547, 16384, 16, 36, 1),
    (257, 16384, 64, 32, 0), (12547, 255, 1, 36, 0), (255, 1000, 3, 32, 0),
]


def _assign(z, ldz, codes, bias, embed, K, R, G, normalize, splits):
    ops, L = _ops()
    D = 32
    zb = padded(z, ldz, fill=float("nan"))
    wv, wi = torch.empty(R, splits, device=DEV), torch.empty(R, splits, dtype=torch.int32, device=DEV)
    tok = torch.full((R + 1,), -7, dtype=torch.int64, device=DEV)
    nb = (R + G - 1) // G
    quant = torch.full((nb, D, G), SENT, device=DEV)
    L.check(L.vq_assign_bias(ops._p(zb), ldz, ops._p(codes), ops._p(bias), ops._p(embed), K, D, R, G, normalize, ops._p(wv), ops._p(wi), splits,
                             ops._p(tok), ops._p(quant), ops._stream()))
    assert int(tok[R]) == -7
    return tok[:R], quant


def _scores64(x64, codes64, bias64, R):
    out = torch.empty(R, codes64.shape[0], dtype=torch.float64, device=DEV)
    for i in range(0, R, 2048):
        out[i:i + 2048] = x64[i:i + 2048] @ codes64.t()
    return out + bias64 if bias64 is not None else out


def _check_assignment(name, tok, quant, scores, tau, embed, R, G):
    """token == float64 argmax unless the float64 score gap to the argmax is <= tau (near ties: < 1e-3 of the rows);
    quant (B, D, G) == embed[tokens] exactly; the entries of rows past R keep the sentinel."""
    K = scores.shape[1]
    assert bool(((tok >= 0) & (tok < K)).all()), name
    best = scores.argmax(1)
    gap = scores.gather(1, best[:, None])[:, 0] - scores.gather(1, tok[:, None])[:, 0]
    diff = tok != best
    assert bool((gap[diff] <= tau[diff]).all()), f"{name}: a token off the arg-max by more than the score-error bound"
    assert int(diff.sum()) <= 1e-3 * R, f"{name}: {int(diff.sum())} near-tie exceptions of {R} rows"
    q = quant.permute(0, 2, 1).reshape(-1, embed.shape[1])
    assert torch.equal(q[:R], embed[tok])
    assert bool((q[R:] == SENT).all())
    return int(diff.sum())


@pytest.mark.parametrize("R,K,splits,ldz,normalize", ASSIGN_CASES)
def test_assign_cosine(R, K, splits, ldz, normalize):
    """CosineSimCodebook search (quantize_lucid.py:394-407): argmax_c <x, En_c>, x = l2norm(z) when normalize, first maximum wins.
    fp32 score: a 32-term FMA chain, gamma_33 |x| |En_c|; normalisation in-kernel adds (D/2 + 3) u relative to x.  Per row
        tau = 2 (33 + 19) u |x| max_c |En_c|   (Cauchy-Schwarz for sum |x_d| |e_cd|; two scores enter a gap)."""
    D, G = 32, 196 if R > 1000 else R
    z = randn(R, D, seed=60 + R + K)
    if R > 1:
        z[1] = 0.0                                                          # zero latent: every score 0, code 0 wins
    embed = randn(K, D, seed=61 + K)
    En = F.normalize(embed, dim=-1)
    tok, quant = _assign(z, ldz, En, None, embed, K, R, G, normalize, splits)
    x64 = F.normalize(z.double(), dim=-1) if normalize else z.double()
    scores = _scores64(x64, En.double(), None, R)
    tau = 2 * (33 + 19) * U * x64.norm(dim=1) * float(En.double().norm(dim=1).max())
    n = _check_assignment(f"cosine R={R} K={K} splits={splits}", tok, quant, scores, tau, embed, R, G)
    if R > 1:
        assert int(tok[1]) == 0 or not normalize
    record("vq_kernels.assign", R=R, K=K, splits=splits, near_ties=n)


@pytest.mark.parametrize("R,K,splits,ldz,normalize", ASSIGN_CASES)
def test_assign_euclidean(R, K, splits, ldz, normalize):
    """EuclideanCodebook search (quantize_lucid.py:272-280) as fm_vq_assign_bias on the raw codes with the fm_vq_code_bias scores:
    argmax_c <x, e_c> - |e_c|^2 / 2 == the nearest code.  Reference: float64 -|x - e_c|^2 / 2 + |x|^2 / 2 (the same ordering).
    Score error: the chain starts at the fp32 bias (itself within gamma_32 |e|^2 / 2), then 32 FMAs:
        tau = 2 ((33 + 19) u (|x| max|e| + max|e|^2 / 2) + 33 u max|e|^2 / 2)."""
    ops, L = _ops()
    D, G = 32, 196 if R > 1000 else R
    z = randn(R, D, seed=70 + R + K)
    if R > 1:
        z[1] = 0.0
    embed = randn(K, D, scale=0.7, seed=71 + K)
    bias = torch.empty(K, device=DEV)
    L.check(L.vq_code_bias(ops._p(embed), K, D, ops._p(bias), ops._stream()))
    tok, quant = _assign(z, ldz, embed, bias, embed, K, R, G, normalize, splits)
    x64 = F.normalize(z.double(), dim=-1) if normalize else z.double()
    e64 = embed.double()
    scores = _scores64(x64, e64, -0.5 * e64.pow(2).sum(1), R)
    e_max = float(e64.norm(dim=1).max())
    tau = 2 * ((33 + 19) * U * (x64.norm(dim=1) * e_max + 0.5 * e_max ** 2) + 33 * U * 0.5 * e_max ** 2)
    n = _check_assignment(f"euclid R={R} K={K} splits={splits}", tok, quant, scores, tau, embed, R, G)
    # the float64 nearest-distance view of the same rule
    if R <= 300:
        d = torch.cdist(x64, e64)
        near = d.argmin(1)
        assert bool((tok == near).all()) or n > 0
    record("vq_kernels.assign_bias", R=R, K=K, splits=splits, near_ties=n)


@pytest.mark.parametrize("euclid", [False, True])
def test_assign_duplicate_codes_first_index_wins(euclid):
    """Exact duplicates at i < j: i wins (torch.argmax).  K = 1000, splits = 3: per = 336, so the pairs sit in one chunk of one split
    (10, 20), across the VQ_CHUNK = 256 boundary of split 0 (100, 300) and across splits (200, 700)."""
    ops, L = _ops()
    K, D = 1000, 32
    embed = randn(K, D, seed=80)
    pairs = [(10, 20), (100, 300), (200, 700)]
    for i, j in pairs:
        embed[j] = embed[i]
    z = torch.stack([embed[j] * 2.5 if not euclid else embed[j] for _, j in pairs] + [embed[i] for i, _ in pairs])
    R = z.shape[0]
    if euclid:
        codes, bias = embed, torch.empty(K, device=DEV)
        L.check(L.vq_code_bias(ops._p(embed), K, D, ops._p(bias), ops._stream()))
    else:
        codes, bias = F.normalize(embed, dim=-1), None
    for splits in (1, 3, 16):
        tok, _ = _assign(z, 32, codes, bias, embed, K, R, R, 0 if euclid else 1, splits)
        assert tok.tolist() == [i for i, _ in pairs] * 2, (euclid, splits, tok.tolist())


def test_assign_refuses_other_latent_dims():
    ops, L = _ops()
    z, e = randn(4, 16), randn(8, 16)
    wv, wi = torch.empty(4, 1, device=DEV), torch.empty(4, 1, dtype=torch.int32, device=DEV)
    tok = torch.zeros(4, dtype=torch.int64, device=DEV)
    refused(L.vq_assign(ops._p(z), 16, ops._p(e), ops._p(e), 8, 16, 4, 4, 1, ops._p(wv), ops._p(wi), 1, ops._p(tok), None, ops._stream()),
            "latent_dim=16 unsupported")


# ------------------------------------------------------------------------------------------------
# fm_vq_code_stats / _raw, fm_vq_ema_update / _euclid
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("raw", [False, True])
@pytest.mark.parametrize("R,K,D,one_code", [(5000, 37, 8, False), (5000, 300, 32, False), (20000, 40, 64, True), (20000, 1000, 64, False)])
def test_code_stats(R, K, D, one_code, raw):
    """bins == bincount(tokens) exactly; sums[k] = sum of l2norm(z_r) (raw: z_r) over the rows of code k (quantize_lucid.py:409-419,
    :283-289).  Each term carries (D/2 + 3) u relative from the normalisation; n_k fp32 atomics add gamma_{n_k}:
        |sums - ref| <= ((n_k + 1) + D / 2 + 3) u sum_{r in k} |x_rd| + ETA.
    Unused codes give exactly 0 although the buffers start as NaN; one_code: all rows on code 3 (maximum atomic contention)."""
    ops, L = _ops()
    z = padded(randn(R, D, seed=90 + R + D), D + 5, fill=float("nan"))
    tok = torch.full((R,), 3, dtype=torch.int64, device=DEV) if one_code else randint(0, K // 2, (R,), seed=91) * 2    # odd codes unused
    bbuf = torch.full((K + 4,), float("nan"), device=DEV)
    sbuf = torch.full((K * D + 8,), float("nan"), device=DEV)
    bbuf[K:], sbuf[K * D:] = SENT, SENT
    fn = L.vq_code_stats_raw if raw else L.vq_code_stats
    L.check(fn(ops._p(z), z.stride(0), ops._p(tok), R, D, K, ops._p(bbuf), ops._p(sbuf), ops._stream()))
    bins, sums = bbuf[:K], sbuf[:K * D].view(K, D)
    cnt = torch.bincount(tok, minlength=K)
    assert torch.equal(bins.double(), cnt.double())
    x64 = z.double() if raw else F.normalize(z.double(), dim=-1)
    ref = torch.zeros(K, D, dtype=torch.float64, device=DEV).index_add_(0, tok, x64)
    mag = torch.zeros(K, D, dtype=torch.float64, device=DEV).index_add_(0, tok, x64.abs())
    r = check(f"code_stats raw={raw} D={D}", sums, ref, ((cnt.double() + 1)[:, None] + D / 2 + 3) * U * mag + ETA)
    assert bool((sums[cnt == 0] == 0).all())
    assert bool((bbuf[K:] == SENT).all()) and bool((sbuf[K * D:] == SENT).all())
    record("vq_kernels.code_stats", raw=raw, R=R, K=K, D=D, worst_err_over_tol=r)


def _f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


@pytest.mark.parametrize("decay", [0.0, 0.99, 1.0])
@pytest.mark.parametrize("K,D", [(37, 8), (37, 32), (130, 64)])
def test_ema_update_cosine(K, D, decay):
    """quantize_lucid.py:413, :421-425 (embed = l2norm(embed) inside forward, so an unused code's target is l2norm(embed)):
        cluster_size <- cluster_size d + bins (1 - d);  embed <- embed d + target (1 - d),  target = l2norm(sums / bins) or l2norm(embed).
    target: division u, normalisation (D/2 + 3) u; then two products and an FMA:
        |embed - ref| <= (D/2 + 7) u (|target (1 - d)| + |embed d|) + ETA;   |cluster - ref| <= 3 u (|bins (1 - d)| + |cs d|)."""
    ops, L = _ops()
    d = _f32(decay)
    bins = randint(0, 5, (K,), seed=100 + K).float()
    bins[:3] = 0.0
    sums = randn(K, D, seed=101) * bins[:, None].clamp_min(1.0)
    sums[bins == 0] = float("nan")                                        # never read for unused codes (upstream masks them)
    ebuf = torch.full((K * D + 8,), SENT, device=DEV)
    embed0 = randn(K, D, seed=102)
    ebuf[:K * D] = embed0.reshape(-1)
    cs0 = randn(K, seed=103).abs() * 3
    cbuf = torch.full((K + 4,), SENT, device=DEV)
    cbuf[:K] = cs0
    L.check(L.vq_ema_update(ops._p(bins), ops._p(sums), ops._p(ebuf), ops._p(cbuf), K, D, d, ops._stream()))
    e64, b64 = embed0.double(), bins.double()
    a = 1.0 - d
    tgt = torch.where((b64 == 0)[:, None], F.normalize(e64, dim=-1), F.normalize(torch.nan_to_num(sums.double()) / b64.clamp_min(1)[:, None], dim=-1))
    ref = e64 * d + tgt * a
    r = check(f"ema K={K} D={D} d={decay}", ebuf[:K * D].view(K, D), ref, (D / 2 + 7) * U * ((tgt * a).abs() + (e64 * d).abs()) + ETA)
    rc = check("ema cluster", cbuf[:K], cs0.double() * d + b64 * a, 3 * U * ((b64 * a).abs() + (cs0.double() * d).abs()))
    assert bool((ebuf[K * D:] == SENT).all()) and bool((cbuf[K:] == SENT).all())
    record("vq_kernels.ema_update", K=K, D=D, decay=decay, worst_err_over_tol=max(r, rc))


@pytest.mark.parametrize("decay", [0.0, 0.99, 1.0])
@pytest.mark.parametrize("K,D", [(37, 8), (37, 32), (130, 64)])
def test_ema_update_euclid(K, D, decay):
    """quantize_lucid.py:286-296: cluster_size and embed_avg EMAs, S = sum_k cluster_size, smoothed = (cs + eps) / (S + K eps) S,
    embed = embed_avg / smoothed.  S: gamma_K on positive terms; smoothed collects (2 K + 12) u relative; the embed_avg FMA 2 u of its
    terms, the division u:
        |embed - ref| <= (2 K + 14) u |ref| + 2 u (|s (1 - d)| + |avg d|) / smoothed + ETA."""
    ops, L = _ops()
    d, eps = _f32(decay), _f32(1e-5)
    bins = randint(0, 5, (K,), seed=110 + K).float()
    bins[:3] = 0.0
    sums = randn(K, D, seed=111)
    avg0, cs0 = randn(K, D, seed=112), randn(K, seed=113).abs() + 0.5
    ebuf = torch.full((K * D + 8,), SENT, device=DEV)
    abuf, cbuf = ebuf.clone(), torch.full((K + 4,), SENT, device=DEV)
    abuf[:K * D], cbuf[:K] = avg0.reshape(-1), cs0
    total = torch.full((1,), float("nan"), device=DEV)
    L.check(L.vq_ema_update_euclid(ops._p(bins), ops._p(sums), ops._p(ebuf), ops._p(abuf), ops._p(cbuf), ops._p(total), K, D, d, eps, ops._stream()))
    a = 1.0 - d
    cs = cs0.double() * d + bins.double() * a
    avg = avg0.double() * d + sums.double() * a
    S = cs.sum()
    sm = (cs + eps) / (S + K * eps) * S
    ref = avg / sm[:, None]
    tol = (2 * K + 14) * U * ref.abs() + 2 * U * ((sums.double() * a).abs() + (avg0.double() * d).abs()) / sm[:, None] + ETA
    r = check(f"ema_euclid K={K} D={D} d={decay}", ebuf[:K * D].view(K, D), ref, tol)
    check("ema_euclid avg", abuf[:K * D].view(K, D), avg, 2 * U * ((sums.double() * a).abs() + (avg0.double() * d).abs()))
    check("ema_euclid cluster", cbuf[:K], cs, 2 * U * cs.abs())
    assert bool((ebuf[K * D:] == SENT).all()) and bool((abuf[K * D:] == SENT).all()) and bool((cbuf[K:] == SENT).all())
    record("vq_kernels.ema_update_euclid", K=K, D=D, decay=decay, worst_err_over_tol=r)


# ------------------------------------------------------------------------------------------------
# fm_vq_latent_grad / _normalized
# ------------------------------------------------------------------------------------------------
def _latent_grad_ref(z, embed, tok, dq, gl, w, normalized):
    """float64 autograd of the upstream training branch (quantize_lucid.py:525-527, :533-541):
        x = z or l2norm(z);  quantize = x + (q - x).detach();  objective = <dq, quantize> + g w mse(q.detach(), x)."""
    z64 = z.double().requires_grad_(True)
    x = F.normalize(z64, dim=-1) if normalized else z64
    q = embed.double()[tok]
    quantize = x + (q - x).detach()
    commit = w * F.mse_loss(q, x)
    obj = (quantize * (dq.double() if dq is not None else 0.0)).sum() + (gl if gl is not None else 0.0) * commit
    obj.backward()
    return z64.grad.detach(), float(commit.detach()), x.detach(), q


def _commit_tol(x, q, w, R, D, total):
    """w mean((q - x)^2): per-lane sums over ceil(R / 32768) rows, a 64-lane tree, one fp32 atomic per wave (at most min(R, 32768)
    waves) on positive terms; each difference within (D/2 + 4) u |x| (+ u |x - q|), the scaling 3 u:
        |commit - ref| <= (ceil(R / 32768) + 6 + min(R, 32768) + 3) u ref + (D + 10) u w sum |x| |x - q| / (R D) + u |total|."""
    ref = w * float((x - q).pow(2).mean())
    cross = w * float((x.abs() * (x - q).abs()).sum()) / (R * D)
    return (-(-R // 32768) + 6 + min(R, 32768) + 3) * U * ref + (D + 10) * U * cross + U * abs(total)


def _latent_grad_tol(x, q, dq, coef, D, normalized, znorm):
    """dz = dq + c (x - q), c = g w 2 / (R D) (coefficient: 3 roundings; difference and FMA: u each):
        |dz - ref| <= 2 u |dq| + 6 u |c| (|x| + |q|) + ETA.
    normalized: dz = (dx - x <x, dx>) / |z|, x carrying (D/2 + 3) u, the D-term dot gamma_D; with M_d = |dq_d| + |c| (|x_d| + |q_d|):
        |dz - ref| <= (D + 12) u (M_d + |x_d| sum_e |x_e| M_e) / |z| + ETA."""
    M = (dq.double().abs() if dq is not None else 0.0) + abs(coef) * (x.abs() + q.abs())
    if not normalized:
        return (2 * U * dq.double().abs() if dq is not None else 0.0) + 6 * U * abs(coef) * (x.abs() + q.abs()) + ETA
    S = (x.abs() * M).sum(1, keepdim=True)
    return (D + 12) * U * (M + x.abs() * S) / znorm + ETA


@pytest.mark.parametrize("normalized", [False, True])
@pytest.mark.parametrize("R,D", [(1, 8), (3, 63), (4097, 32), (40000, 64)])     # 40000 rows > 8192 x 4 waves: lanes accumulate several rows
def test_latent_grad(R, D, normalized):
    """dz and the commitment value w mean((q - x)^2) against float64 autograd; strided operands, sentinels in dz's pad columns, the
    commitment value added onto a nonzero pre-filled scalar (bound: _commit_tol)."""
    ops, L = _ops()
    K, w, g = 50, 0.25, 1.7
    z = randn(R, D, seed=120 + R + D)
    embed = randn(K, D, scale=0.3, seed=121) if normalized else randn(K, D, seed=121)
    tok = randint(0, K, (R,), seed=122)
    dq = randn(R, D, scale=1e-3, seed=123)
    zb, dqb = padded(z, D + 3, fill=float("nan")), padded(dq, D + 5, fill=float("nan"))
    gl = torch.tensor([g], device=DEV)
    buf, dz = sentinel_rows(R, D, D + 7)
    pre = 0.75
    commit = torch.full((1,), pre, device=DEV)
    fn = L.vq_latent_grad_normalized if normalized else L.vq_latent_grad
    L.check(fn(ops._p(zb), zb.stride(0), ops._p(embed), ops._p(tok), ops._p(dqb), dqb.stride(0), ops._p(gl), w, ops._p(buf), buf.stride(0),
               ops._p(commit), R, D, ops._stream()))
    ref, cval, x, q = _latent_grad_ref(z, embed, tok, dq, g, w, normalized)
    coef = g * w * 2 / (R * D)
    r = check(f"latent_grad R={R} D={D} norm={normalized}", dz, ref,
              _latent_grad_tol(x, q, dq, coef, D, normalized, z.double().norm(dim=1, keepdim=True)))
    assert untouched(buf, R, D)
    ctol = _commit_tol(x, q, w, R, D, pre + cval)
    rc = check("commit", commit, torch.tensor([pre + cval], dtype=torch.float64, device=DEV), ctol)
    record("vq_kernels.latent_grad", normalized=normalized, R=R, D=D, worst_err_over_tol=r, commit_err_over_tol=rc)


@pytest.mark.parametrize("normalized", [False, True])
def test_latent_grad_optional_operands(normalized):
    """Each of dquant, grad_loss, dz, commit set to NULL in turn; dz and commit both NULL is refused."""
    ops, L = _ops()
    R, D, K, w, g = 1000, 32, 50, 0.25, 1.7
    z = randn(R, D, seed=130)
    embed = randn(K, D, scale=0.3, seed=131)
    tok = randint(0, K, (R,), seed=132)
    dq = randn(R, D, scale=1e-3, seed=133)
    gl = torch.tensor([g], device=DEV)
    fn = L.vq_latent_grad_normalized if normalized else L.vq_latent_grad
    zn = z.double().norm(dim=1, keepdim=True)
    for drop in ("dquant", "grad_loss", "dz", "commit"):
        dz = torch.full((R, D), SENT, device=DEV)
        commit = torch.zeros(1, device=DEV)
        a_dq, a_gl = (None if drop == "dquant" else dq), (None if drop == "grad_loss" else gl)
        L.check(fn(ops._p(z), D, ops._p(embed), ops._p(tok), ops._p(a_dq), D, ops._p(a_gl), w, None if drop == "dz" else ops._p(dz), D,
                   None if drop == "commit" else ops._p(commit), R, D, ops._stream()))
        ref, cval, x, q = _latent_grad_ref(z, embed, tok, a_dq, g if a_gl is not None else None, w, normalized)
        if drop == "dz":
            assert bool((dz == SENT).all())
        else:
            coef = (g if a_gl is not None else 0.0) * w * 2 / (R * D)
            check(f"latent_grad without {drop}", dz, ref, _latent_grad_tol(x, q, a_dq, coef, D, normalized, zn))
        if drop == "commit":
            assert float(commit) == 0.0
        else:
            check(f"commit without {drop}", commit, torch.tensor([cval], dtype=torch.float64, device=DEV), _commit_tol(x, q, w, R, D, cval))
    refused(fn(ops._p(z), D, ops._p(embed), ops._p(tok), ops._p(dq), D, ops._p(gl), w, None, 0, None, R, D, ops._stream()), "bad argument")


# ------------------------------------------------------------------------------------------------
# fm_vq_cls_emb_bwd, fm_tanh_bwd_f32, fm_embed_rows_f32
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("single_label", [False, True])
@pytest.mark.parametrize("P", [1, 8, 16])
def test_cls_emb_bwd(P, single_label):
    """d cls_emb[label(b, y, x)][c] += d patches[(b, y/P, x/P)][(c, y%P, x%P)] (the backward of cls_emb[labels] before the patch
    gather), fp32 atomics onto a nonzero pre-filled table.  n_k atomics per entry:
        |d_emb - ref| <= (n_k + 1) u (sum_{pixels of k} |g| + |d0|) + ETA."""
    ops, L = _ops()
    B, C, H, W, n_labels = 2, 5, 32, 48, 9
    labels = torch.full((B, H, W), 4, dtype=torch.int64, device=DEV) if single_label else randint(0, n_labels, (B, H, W), seed=140 + P)
    R, Fc = B * (H // P) * (W // P), C * P * P
    g = randn(R, Fc, seed=141).bfloat16()
    gp = padded(g, Fc + 6, fill=float("nan"))
    d0 = randn(n_labels, C, seed=142)
    ebuf = torch.full((n_labels * C + 4,), SENT, device=DEV)
    ebuf[:n_labels * C] = d0.reshape(-1)
    L.check(L.vq_cls_emb_bwd(ops._p(gp), gp.stride(0), ops._p(labels), ops._p(ebuf), B, C, H, W, P, ops._stream()))
    per_pix = unpatchify64(g.double(), B, C, H, W, P).permute(0, 2, 3, 1).reshape(-1, C)
    lab = labels.reshape(-1)
    ref = d0.double().index_add(0, lab, per_pix)
    mag = d0.double().abs().index_add(0, lab, per_pix.abs())
    n = torch.bincount(lab, minlength=n_labels).double()
    r = check(f"cls_emb_bwd P={P}", ebuf[:n_labels * C].view(n_labels, C), ref, (n[:, None] + 1) * U * mag + ETA)
    assert bool((ebuf[n_labels * C:] == SENT).all())
    record("vq_kernels.cls_emb_bwd", P=P, single_label=single_label, worst_err_over_tol=r)


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("R,N", [(100, 1536), (2100, 2048)])      # 2100 x 2048 > 256 x 16384: the grid clamp is hit
def test_tanh_bwd(R, N, in_place):
    """dx = dy (1 - t^2) (the Tanh of the post MLP, vit_models.py:494-496): three roundings:
        |dx - ref| <= 3 u |dy| (1 + t^2) + ETA.   In place (dx is dy) as vq/engine.py's _post_mlp_bwd calls it; pad columns untouched."""
    ops, L = _ops()
    ld = N + 4
    dy = padded(randn(R, N, seed=150), ld, fill=SENT)
    t = padded(torch.tanh(randn(R, N, seed=151)), ld, fill=float("nan"))
    ref = dy.double() * (1 - t.double() ** 2)
    tol = 3 * U * dy.double().abs() * (1 + t.double() ** 2) + ETA
    if in_place:
        L.check(L.tanh_bwd_f32(ops._p(dy), ops._p(t), ops._p(dy), R, N, ld, ops._stream()))
        out, base = dy, dy
    else:
        out = padded(torch.zeros(R, N, device=DEV), ld, fill=SENT)
        L.check(L.tanh_bwd_f32(ops._p(dy), ops._p(t), ops._p(out), R, N, ld, ops._stream()))
        base = out
    r = check(f"tanh_bwd R={R} N={N}", out, ref, tol)
    full = base.as_strided((R, ld), (ld, 1))
    assert bool((full[:, N:] == SENT).all())
    record("vq_kernels.tanh_bwd", R=R, N=N, in_place=in_place, worst_err_over_tol=r)


@pytest.mark.parametrize("R,D", [(1, 32), (40000, 32), (3000, 100)])
def test_embed_rows(R, D):
    """out[r] = table[idx[r]] exactly (F.embedding); repeated indices; pad columns and the row past the end untouched."""
    ops, L = _ops()
    K = 77
    table = randn(K, D, seed=160 + D)
    idx = randint(0, K, (R,), seed=161)
    idx[: min(R, 5)] = 7
    buf, out = sentinel_rows(R, D, D + 3)
    L.check(L.embed_rows_f32(ops._p(table), ops._p(idx), ops._p(buf), buf.stride(0), R, D, ops._stream()))
    assert torch.equal(out, table[idx])
    assert untouched(buf, R, D)


# ------------------------------------------------------------------------------------------------
# fm_split3_bf16 and the split3 GEMM
# ------------------------------------------------------------------------------------------------
def _split3(x, K, R, weight_order, apply_tanh, rows=None, extra=8):
    ops, L = _ops()
    rows = rows or R
    buf = torch.full((rows + 1, 3 * K + extra), SENT, dtype=torch.bfloat16, device=DEV)
    L.check(L.split3_bf16(ops._p(x), x.stride(0), ops._p(buf), buf.stride(0), R, K, weight_order, apply_tanh, ops._stream()))
    return buf


@pytest.mark.parametrize("R,K", [(3, 4), (257, 100), (16400, 4096)])     # 16400 x 1024 float4 > 256 x 65535: the grid clamp is hit
def test_split3_bitwise(R, K):
    """hi = bf16(x), lo = bf16(x - hi) (x - hi is exact in fp32); blocks [hi | hi | lo] (weight_order 0) and [hi | lo | hi] (1);
    ldx > K with NaN pad, ldo > 3 K with the pad and the row past the end untouched."""
    x = padded(randn(R, K, seed=170 + K), K + 4, fill=float("nan"))
    hi = x.bfloat16()
    lo = (x - hi.float()).bfloat16()
    for order, blocks in ((0, (hi, hi, lo)), (1, (hi, lo, hi))):
        buf = _split3(x, K, R, order, 0)
        for i, b in enumerate(blocks):
            assert torch.equal(buf[:R, i * K:(i + 1) * K], b), (order, i)
        assert untouched(buf.float(), R, 3 * K)
        del buf


def test_split3_tanh_and_refusal():
    """apply_tanh: hi + lo within FN |tanh| (tanhf) + 2^-16 |tanh| (the bf16 rounding of lo leaves <= 2^-18) of float64 tanh."""
    ops, L = _ops()
    R, K = 300, 512
    x = padded(randn(R, K, scale=2.0, seed=180), K + 4, fill=float("nan"))
    t64 = torch.tanh(x.double())
    for order in (0, 1):
        buf = _split3(x, K, R, order, 1)
        hi = buf[:R, :K]
        lo = buf[:R, 2 * K:3 * K] if order == 0 else buf[:R, K:2 * K]
        assert torch.equal(buf[:R, K:2 * K] if order == 0 else buf[:R, 2 * K:3 * K], hi)
        r = check("split3 tanh", hi.double() + lo.double(), t64, (FN + 2.0 ** -16) * t64.abs())
        assert untouched(buf.float(), R, 3 * K)
    record("vq_kernels.split3_tanh", worst_err_over_tol=r)
    out = torch.zeros(4, 3 * 8, dtype=torch.bfloat16, device=DEV)
    refused(L.split3_bf16(ops._p(x), x.stride(0), ops._p(out), 24, 4, 6, 0, 0, ops._stream()), "K % 4 == 0")


def _ru(v, m):
    return (v + m - 1) // m * m


@pytest.mark.parametrize("R", [1, 100, 1568, 12544])
@pytest.mark.parametrize("D", [384, 768])
def test_split3_gemm_accuracy(D, R):
    """The tokenizer's fp32 tail at inference (vq/engine.py _post_mlp_fwd): X' = split3(x) [hi | hi | lo], W' = split3(w) [hi | lo | hi],
    one bf16 NT GEMM over 3 K with EPI_F32 (+ bias, + res).  Against float64 x w^T + b (+ res):
        |err| <= (3 2^-16 (1 + 2^-7) + (3 K + 3) u) sum_k |x_k| |w_k| + 2 u (|b| + |res|)
    (dropped lo lo product and the two bf16 roundings of lo; fp32 accumulation of exact bf16 products).  fc2 reads tanh(pre): + FN for
    tanhf.  Shapes (R, 4D, D) for fc1 and (R, D, 4D) for fc2.  The worst normwise error must be >= 30 x below that of the same GEMM on
    the hi halves only (a plain bf16 GEMM): the lo blocks contribute."""
    ops, L = _ops()
    Rp = _ru(R, 128)
    out_stats = {}
    for layer, (N, K, tanh) in (("fc1", (4 * D, D, 0)), ("fc2", (D, 4 * D, 1))):
        x = torch.zeros(Rp, K, device=DEV)
        x[:R] = randn(R, K, seed=190 + K + R)
        w = randn(N, K, scale=K ** -0.5, seed=191 + N)
        b = randn(N, scale=0.1, seed=192 + N)
        res = randn(Rp, N, seed=193 + N)
        xs = torch.zeros(Rp, 3 * K, dtype=torch.bfloat16, device=DEV)
        L.check(L.split3_bf16(ops._p(x), K, ops._p(xs), 3 * K, R, K, 0, tanh, ops._stream()))
        ws = torch.empty(N, 3 * K, dtype=torch.bfloat16, device=DEV)
        L.check(L.split3_bf16(ops._p(w), K, ops._p(ws), 3 * K, N, K, 1, 0, ops._stream()))
        x64 = torch.tanh(x[:R].double()) if tanh else x[:R].double()
        w64 = w.double()
        acc = x64 @ w64.t()
        S = x64.abs() @ w64.abs().t()
        coef = 3 * 2.0 ** -16 * (1 + 2.0 ** -7) + (3 * K + 3) * U + (FN if tanh else 0.0)
        for with_res in (False, True):
            out = torch.full((Rp, N), SENT, device=DEV)
            ops.gemm_nt(xs, ws, out, epilogue=L.EPI_F32, bias=b, res=res if with_res else None, M=R, N=N, K=3 * K)
            ref = acc + b.double() + (res[:R].double() if with_res else 0.0)
            tol = coef * S + 2 * U * (b.double().abs() + (res[:R].double().abs() if with_res else 0.0))
            r = check(f"split3 gemm {layer} D={D} R={R} res={with_res}", out[:R], ref, tol)
            rel = float(((out[:R].double() - ref).abs() / S).max())
            out_stats[f"{layer}{'_res' if with_res else ''}"] = (r, rel)
        # plain bf16 GEMM on the hi halves only
        xh = torch.zeros(Rp, K, dtype=torch.bfloat16, device=DEV)
        xh[:R] = xs[:R, :K]
        wh = ws[:, :K].contiguous()
        outh = torch.empty(Rp, N, device=DEV)
        ops.gemm_nt(xh, wh, outh, epilogue=L.EPI_F32, bias=b, M=R, N=N, K=K)
        rel_bf16 = float(((outh[:R].double() - acc - b.double()).abs() / S).max())
        rel_split = out_stats[layer][1]
        assert rel_split * 30 <= rel_bf16, (layer, rel_split, rel_bf16)
        record("vq_kernels.split3_gemm", layer=layer, D=D, R=R, worst_err_over_tol=max(out_stats[layer][0], out_stats[layer + "_res"][0]),
               rel_err_split3=rel_split, rel_err_bf16=rel_bf16)
