"""The two entry points of csrc/lpips_metric.hip against float64 (tests/lpips_metric_util.py has the bounds): the stem convolution element by
element on every case of the contract, with its clamp, affine, bias, ReLU and output-stride variants, its batch invariance and refusals; the
per-layer distance per sample, with its bit properties (symmetry, exact zero, zero rows) and refusals.  Outputs sit in sentinel buffers."""
import ctypes
import itertools
import math

import pytest
import torch
import torch.nn.functional as F

from tests import lpips_metric_util as MU
from tests import parity_log
from tests.vq_metrics_util import sentinel_view, sentinels_intact

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = MU.U
SENT = -7777.0

# (B, Cin, H, W, Cout, K, stride, pad)
STEM_CASES = [(2, 3, 31, 31, 64, 11, 4, 2), (1, 3, 33, 46, 64, 11, 4, 2), (3, 3, 64, 64, 64, 11, 4, 2), (2, 1, 9, 12, 5, 3, 1, 1), (1, 4, 20, 17, 128, 7, 2, 3),
              (2, 2, 15, 15, 33, 5, 3, 0)]
# (clamp, affine, bias, relu, ldo_extra)
FULL = (True, True, True, True, 9)
BARE = (False, False, False, False, 0)


def _stem_inputs(case, seed=0):
    B, Cin, H, W, Cout, K, stride, pad = case
    g = MU.gen(4000 + seed + 7 * H + W + Cout)
    img = 0.8 * torch.randn(B, Cin, H, W, generator=g)                 # a fifth of the pixels lies outside [-1, 1]: the clamp bites
    w = torch.randn(Cout, Cin, K, K, generator=g) / math.sqrt(K * K * Cin)
    bias = torch.randn(Cout, generator=g)
    mul = 1.5 + torch.rand(Cin, generator=g)
    add = torch.randn(Cin, generator=g)
    return img, w, bias, mul, add


def _stem_ref(img, w, bias, mul, add, stride, pad, variant):
    """-> (ref rows, bound rows) float64.  s is formed in float64 from the fp32 mul / add; the zero padding applies to s."""
    clamp, affine, use_bias, relu, _ = variant
    Cout, Cin, K, _ = w.shape
    s = img.double()
    if clamp:
        s = s.clamp(-1.0, 1.0)
    if affine:
        s = s * mul.double().view(1, -1, 1, 1) + add.double().view(1, -1, 1, 1)
    b64 = bias.double() if use_bias else None
    ref = F.conv2d(s, w.double(), b64, stride=stride, padding=pad)
    mag = F.conv2d(s.abs(), w.double().abs(), None if b64 is None else b64.abs(), stride=stride, padding=pad)
    if relu:
        ref = F.relu(ref)
    return MU.to_rows(ref), (K * K * Cin + 4) * U * MU.to_rows(mag)


def _run_stem(img, w, bias, mul, add, stride, pad, variant, c0=3):
    """-> (out view (rows, Cout), the sentinel buffer, the full-width view)."""
    from fourm.utils.inception import ops
    from fourm.vq.percept_losses.lpips_alex import conv2d_stem
    clamp, affine, use_bias, relu, ldo_extra = variant
    B, Cin, H, W = img.shape
    Cout, _, K, _ = w.shape
    Ho, Wo = ops.conv_out_size(H, K, stride, pad), ops.conv_out_size(W, K, stride, pad)
    c0 = c0 if ldo_extra else 0
    buf, view = sentinel_view((B * Ho * Wo, c0 + Cout + ldo_extra), torch.float32, DEV, SENT)
    out = view[:, c0:c0 + Cout]
    wr = w.permute(0, 2, 3, 1).reshape(Cout, -1).contiguous().to(DEV)
    conv2d_stem(img.to(DEV), wr, bias.to(DEV) if use_bias else None, K, K, stride, pad, mul.to(DEV) if affine else None, add.to(DEV) if affine else None,
                (-1.0, 1.0) if clamp else None, relu, out)
    return out, buf, view, c0


def _untouched(buf, view, c0, C):
    return sentinels_intact(buf, view.numel(), SENT) and bool((view[:, :c0] == SENT).all()) and bool((view[:, c0 + C:] == SENT).all())


def _check_stem(case, variant):
    B, Cin, H, W, Cout, K, stride, pad = case
    img, w, bias, mul, add = _stem_inputs(case)
    out, buf, view, c0 = _run_stem(img, w, bias, mul, add, stride, pad, variant)
    ref, bound = _stem_ref(img, w, bias, mul, add, stride, pad, variant)
    got = out.cpu().double()
    assert tuple(got.shape) == tuple(ref.shape)
    assert not torch.isnan(got).any()
    err = (got - ref).abs()
    ratio = float((err / bound.clamp(min=1e-300)).max())
    print(f"stem {case} {variant}: max err / bound {ratio:.3f}, max err {float(err.max()):.3e}")
    assert bool((err <= bound).all()), (ratio, float(err.max()))
    assert float(got.abs().max()) > 0.1
    assert _untouched(buf, view, c0, Cout)
    again, _, _, _ = _run_stem(img, w, bias, mul, add, stride, pad, variant)
    assert torch.equal(again, out)                                     # two calls, the same bits
    return ratio


@pytest.mark.parametrize("variant", [FULL, BARE], ids=["full", "bare"])
@pytest.mark.parametrize("case", STEM_CASES, ids=lambda c: "b%d_c%d_%dx%d_n%d_k%d_s%d_p%d" % c)
def test_stem_matches_float64_per_element(case, variant):
    ratio = _check_stem(case, variant)
    parity_log.record("test_stem_matches_float64_per_element", case=list(case), variant=list(variant), err_over_bound=ratio)


@pytest.mark.parametrize("case", [STEM_CASES[3], STEM_CASES[5]], ids=["narrow_tile", "wide_tile"])
def test_stem_every_switch_alone_and_together(case):
    """clamp, affine, bias and ReLU in all 16 combinations on the two small cases (one per tile shape), inside a wider output buffer."""
    for clamp, affine, use_bias, relu in itertools.product((False, True), repeat=4):
        _check_stem(case, (clamp, affine, use_bias, relu, 5))


def test_stem_padding_applies_after_the_affine():
    """A constant image with add != 0: an output next to the border must see zeros there, not add[c]."""
    img = torch.zeros(1, 3, 31, 31)
    w = torch.ones(4, 3, 11, 11)
    mul, add = torch.ones(3), torch.tensor([1.0, 2.0, 3.0])
    out, _, _, _ = _run_stem(img, w, torch.zeros(4), mul, add, 4, 2, (False, True, False, False, 0))
    got = out.cpu().reshape(7, 7, 4)                                   # (31 + 4 - 11) / 4 + 1 = 7
    assert float(got[2, 2, 0]) == 6.0 * 121                           # interior: all 121 taps see s = add[c]
    assert float(got[0, 0, 0]) == 6.0 * 81                            # corner: 9 x 9 taps inside the image
    assert float(got[0, 3, 1]) == 6.0 * 99                            # top edge


@pytest.mark.parametrize("case", [STEM_CASES[2], (3, 1, 9, 12, 5, 3, 1, 1)], ids=["alex_64", "narrow_tile"])
def test_stem_is_batch_invariant(case):
    """An image alone against the same image as element 2 of a batch of 3 (225 rows per image at 64 x 64: it starts in the middle of a tile)."""
    B, Cin, H, W, Cout, K, stride, pad = case
    assert B == 3
    img, w, bias, mul, add = _stem_inputs(case, seed=1)
    three, _, _, _ = _run_stem(img, w, bias, mul, add, stride, pad, FULL)
    one, _, _, _ = _run_stem(img[2:3].contiguous(), w, bias, mul, add, stride, pad, FULL)
    n = one.shape[0]
    assert three.shape[0] == 3 * n
    assert torch.equal(three[2 * n:], one)


def test_stem_refusals_leave_the_output_untouched():
    from fourm.hip import _lib as L
    B, Cin, H, W, Cout, K, stride, pad = 1, 3, 31, 31, 8, 11, 4, 2
    img = torch.zeros(B * Cin * H * W + 4, device=DEV)
    w = torch.zeros(Cout * K * K * Cin + 4, device=DEV)
    vec = torch.zeros(16, device=DEV)
    buf, view = sentinel_view((7 * 7, Cout), torch.float32, DEV, SENT)      # Ho = Wo = (31 + 4 - 11) / 4 + 1 = 7
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)

    def args(**kw):
        d = dict(img=p(img), w=p(w), bias=p(vec), mul=p(vec), add=p(vec), out=p(view), B=B, Cin=Cin, H=H, W=W, Cout=Cout, KH=K, KW=K, stride=stride, pad=pad,
                 ldw=K * K * Cin, ldo=Cout, relu=1, clamp=1, reserved=0, lo=-1.0, hi=1.0)
        d.update(kw)
        return L.Conv2dStemArgs(**d)

    bad = [dict(Cin=5, ldw=K * K * 5), dict(Cin=0), dict(Cout=129, ldo=129), dict(Cout=0), dict(KH=12), dict(KW=12), dict(KH=0), dict(stride=5), dict(stride=0),
           dict(pad=6), dict(pad=-1), dict(H=6, pad=2, KH=11), dict(W=3, pad=3, KW=11), dict(B=0), dict(img=None), dict(w=None), dict(out=None),
           dict(mul=None), dict(add=None), dict(ldo=Cout - 1), dict(ldw=K * K * Cin - 1), dict(img=p(img, 2)), dict(w=p(w, 1)), dict(out=p(view, 2)),
           dict(bias=p(vec, 2)), dict(mul=p(vec, 2)), dict(B=1 << 30, H=200, W=200)]
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for kw in bad:
        a = args(**kw)
        assert L.conv2d_stem_f32(ctypes.byref(a), stream) == -1, kw
        assert L.lib.fm_last_error().startswith(b"fm_conv2d_stem_f32"), kw
    torch.cuda.synchronize()
    assert bool((view == SENT).all()) and sentinels_intact(buf, view.numel(), SENT)
    a = args()                                                         # the same arguments, unmodified, are accepted
    assert L.conv2d_stem_f32(ctypes.byref(a), stream) == 0
    torch.cuda.synchronize()
    assert bool((view != SENT).all()) and sentinels_intact(buf, view.numel(), SENT)


# ---- fm_lpips_score ------------------------------------------------------------------------------------------------------------------
SCORE_CASES = [(2, 1, 64), (3, 49, 192), (1, 225, 384), (2, 65, 256)]


def _features(B, P, C, seed):
    """Post-ReLU-like rows: half the entries zero; on sample 0 one pixel all zero on both sides and one on either side only (where P allows)."""
    g = MU.gen(seed)
    a = F.relu(torch.randn(B * P, C, generator=g))
    b = F.relu(a + 0.5 * torch.randn(B * P, C, generator=g))
    if P >= 4:
        a[1] = 0
        b[1] = 0
        a[2] = 0
        b[3] = 0
    w = torch.rand(C, generator=g)
    return a, b, w


def _padded(t, ld):
    buf = torch.full((t.shape[0], ld), float("nan"), dtype=torch.float32, device=DEV)
    buf[:, :t.shape[1]] = t.to(DEV)
    return buf[:, :t.shape[1]]


@pytest.mark.parametrize("B,P,C", SCORE_CASES)
def test_score_matches_float64_per_sample(B, P, C):
    from fourm.vq.percept_losses.lpips_alex import lpips_score
    a, b, w = _features(B, P, C, 900 + P + C)
    ref64 = MU.rows_score(a, b, w, B, P, torch.float64)
    ref32 = MU.rows_score(a, b, w, B, P, torch.float32)
    tol, base = MU.tol(ref64, ref32)
    ad, bd, wd = _padded(a, C + 4), _padded(b, C + 8), w.to(DEV)     # strided lda, ldb
    buf, score = sentinel_view((B,), torch.float32, DEV, SENT, pad=64)
    score.zero_()
    lpips_score(ad, bd, wd, B, P, score)
    got = score.cpu().double()
    assert bool(torch.isfinite(got).all())
    err = (got - ref64).abs()
    print(f"score B{B} P{P} C{C}: err {float(err.max()):.3e}, fp32 restatement {base:.3e}, bound {tol:.3e}, values {ref64.tolist()}")
    parity_log.record("test_score_matches_float64_per_sample", shape=[B, P, C], err=float(err.max()), fp32_restatement=base, bound=tol,
                      ratio=float(err.max()) / base if base else None)
    assert bool((err <= tol).all()), (err.tolist(), base, tol)
    assert float(ref64.min()) > 1e-3
    assert sentinels_intact(buf, B, SENT)
    first = score.clone()
    # contiguous rows give the same bits as strided ones; the call accumulates
    lpips_score(a.to(DEV), b.to(DEV), wd, B, P, score)
    assert torch.equal(score, first + first)
    # swapped arguments: equal bits
    swapped = torch.zeros(B, device=DEV)
    lpips_score(bd, ad, wd, B, P, swapped)
    assert torch.equal(swapped, first)
    # a against itself: exactly 0, added onto what is there
    same = torch.full((B,), 0.25, device=DEV)
    lpips_score(ad, ad, wd, B, P, same)
    assert bool((same == 0.25).all())


def test_score_zero_rows_are_finite_and_exact():
    from fourm.vq.percept_losses.lpips_alex import lpips_score
    C, P = 64, 3
    z = torch.zeros(P, C, device=DEV)
    one = torch.zeros(P, C, device=DEV)
    one[:, 0] = 2.0                                                    # unit vector e_0 after the normalisation (eps is far below fp32 resolution of 4)
    w = torch.full((C,), 0.5, device=DEV)
    s = torch.zeros(1, device=DEV)
    lpips_score(z, z, w, 1, P, s)
    assert float(s) == 0.0
    lpips_score(z, one, w, 1, P, s)
    assert float(s) == 0.5                                             # (0 - 1)^2 * 0.5 on every pixel, mean over the pixels
    lpips_score(one, z, w, 1, P, s)
    assert float(s) == 1.0


def test_score_refusals_leave_the_score_untouched():
    from fourm.hip import _lib as L
    B, P, C = 2, 5, 64
    a = torch.zeros(B * P * (C + 8) + 8, device=DEV)
    w = torch.zeros(512 + 8, device=DEV)
    scratch = torch.zeros(64, device=DEV)
    buf, score = sentinel_view((B,), torch.float32, DEV, SENT)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    good = dict(a=p(a), lda=C, b=p(a), ldb=C, w=p(w), B=B, P=P, C=C, eps=1e-8, score=p(score), scratch=p(scratch))
    order = ("a", "lda", "b", "ldb", "w", "B", "P", "C", "eps", "score", "scratch")
    bad = [dict(C=62, lda=64), dict(C=516, lda=516, ldb=516), dict(C=0), dict(lda=C + 2), dict(ldb=C - 4), dict(lda=C - 4), dict(a=p(a, 4)), dict(b=p(a, 8)),
           dict(w=p(w, 4)), dict(score=p(score, 4)), dict(scratch=p(scratch, 4)), dict(P=0), dict(B=0), dict(a=None), dict(b=None), dict(w=None),
           dict(score=None), dict(scratch=None), dict(eps=-1.0)]
    for kw in bad:
        d = dict(good)
        d.update(kw)
        assert L.lpips_score(*[d[k] for k in order], stream) == -1, kw
        assert L.lib.fm_last_error().startswith(b"fm_lpips_score"), kw
    torch.cuda.synchronize()
    assert bool((score == SENT).all()) and sentinels_intact(buf, B, SENT)
    assert L.lpips_score(*[good[k] for k in order], stream) == 0
    torch.cuda.synchronize()
    assert bool((score == SENT).all())                                 # zeros against zeros: + 0
