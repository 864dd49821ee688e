"""The four entry points of csrc/inception.hip, element by element against float64 (tests/inception_util.py has the bounds): the fp32
implicit-GEMM convolution on every (kernel, stride, padding) class of the InceptionV3 graph, the pools, the preprocess and the float64 moment
accumulator.  Inputs sit in NaN-padded rows (ld > C) and outputs in channel slices of sentinel buffers."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import inception_util as IU
from tests.vq_metrics_util import sentinel_view, sentinels_intact

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = IU.U
SENT = -7777.0

# (KH, KW, stride, pad_h, pad_w): every class of the graph
CLASSES = [(3, 3, 2, 0, 0), (3, 3, 1, 0, 0), (3, 3, 1, 1, 1), (1, 1, 1, 0, 0), (5, 5, 1, 2, 2), (1, 7, 1, 0, 3), (7, 1, 1, 3, 0), (1, 3, 1, 0, 1), (3, 1, 1, 1, 0)]
CINS, COUTS = (3, 48, 80, 448), (32, 80, 192, 1008)


def _conv_cases():
    cases = []
    for i, cls in enumerate(CLASSES):                                  # every class on both shapes; the channel counts rotate through all values
        for j, (B, H, W) in enumerate(((2, 9, 7), (2, 17, 17))):
            cases.append(cls + (CINS[(i + j) % 4], COUTS[(i + 2 * j + 1) % 4], B, H, W, 4 + (i + j) % 2))
    for H, W in ((10, 8), (16, 16)):                                   # stride 2 on even sizes (the odd ones are above)
        cases.append((3, 3, 2, 0, 0, 48, 80, 2, H, W, 4))
    for cin in CINS:                                                   # every (Cin, Cout) pair on the 1 x 1 class
        for cout in COUTS:
            cases.append((1, 1, 1, 0, 0, cin, cout, 2, 9, 7, 4 if cin % 4 == 0 and cout % 2 == 0 else 5))
    return cases


def _padded_rows(data, ld, fill=float("nan")):
    """data (rows, C) fp32 CPU -> a device view (rows, C) with row stride ld whose padding columns hold ``fill``."""
    buf = torch.full((data.shape[0], ld), fill, dtype=torch.float32, device=DEV)
    buf[:, :data.shape[1]] = data.to(DEV)
    return buf[:, :data.shape[1]]


def _run_conv(x_nchw, w, bias, stride, pad, relu, ldx_extra, c0=3, ldo_extra=9, ldw_extra=0):
    """-> (out view (rows, Cout) on the device, the sentinel buffer, its element count).  x_nchw, w (Cout, Cin, KH, KW), bias: fp32 CPU."""
    from fourm.utils.inception import ops
    B, Cin, H, W = x_nchw.shape
    Cout, _, KH, KW = w.shape
    xr = _padded_rows(IU.to_rows(x_nchw), Cin + ldx_extra)
    K = KH * KW * Cin
    wr = _padded_rows(w.permute(0, 2, 3, 1).reshape(Cout, K), K + ldw_extra)
    Ho, Wo = ops.conv_out_size(H, KH, stride, pad[0]), ops.conv_out_size(W, KW, stride, pad[1])
    ldo = c0 + Cout + ldo_extra
    buf, view = sentinel_view((B * Ho * Wo, ldo), torch.float32, DEV, SENT)
    out = view[:, c0:c0 + Cout]
    ops.conv2d_nhwc(xr, B, H, W, wr, None if bias is None else bias.to(DEV), KH, KW, stride, pad, relu, out)
    return out, buf, view


def _slice_untouched(buf, view, c0, C):
    return sentinels_intact(buf, view.numel(), SENT) and bool((view[:, :c0] == SENT).all()) and bool((view[:, c0 + C:] == SENT).all())


@pytest.mark.parametrize("case", _conv_cases(), ids=lambda c: "k%dx%d_s%d_p%d%d_c%d_n%d_b%d_%dx%d_ld%d" % c)
def test_conv_matches_float64_per_element(case):
    KH, KW, stride, ph, pw, Cin, Cout, B, H, W, ldx_extra = case
    g = IU.gen(1000 + KH * 131 + KW * 17 + Cin + Cout + H)
    x = torch.randn(B, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, KH, KW, generator=g) / math.sqrt(KH * KW * Cin)
    bias = torch.randn(Cout, generator=g)
    relu = (Cin + Cout + H) % 2 == 0
    out, buf, view = _run_conv(x, w, bias, stride, (ph, pw), relu, ldx_extra, ldw_extra=4 if KH == 5 or Cin == 80 else 0)
    ref = F.conv2d(x.double(), w.double(), bias.double(), stride=stride, padding=(ph, pw))
    mag = F.conv2d(x.double().abs(), w.double().abs(), bias.double().abs(), stride=stride, padding=(ph, pw))
    bound = (KH * KW * Cin + 2) * U * IU.to_rows(mag)
    if relu:
        ref = F.relu(ref)
    got = out.cpu().double()
    assert tuple(got.shape) == tuple(bound.shape)
    assert not torch.isnan(got).any()
    err = (got - IU.to_rows(ref)).abs()
    assert bool((err <= bound).all()), (float((err / bound).max()), float(err.max()))
    assert float(got.abs().max()) > 0.1
    assert _slice_untouched(buf, view, 3, Cout)
    again, _, _ = _run_conv(x, w, bias, stride, (ph, pw), relu, ldx_extra, ldw_extra=4 if KH == 5 or Cin == 80 else 0)
    assert torch.equal(again, out)                                     # two calls, the same bits
    if ldx_extra == 4 and Cin % 4 == 0:                                # the 16-byte-load form and the scalar form stage the same values
        other, _, _ = _run_conv(x, w, bias, stride, (ph, pw), relu, 5, ldw_extra=1)
        assert torch.equal(other, out)


@pytest.mark.parametrize("cls,Cin,Cout,H,W", [((3, 3, 1, 1, 1), 48, 80, 17, 17), ((7, 1, 1, 3, 0), 80, 192, 17, 17), ((3, 3, 2, 0, 0), 3, 32, 17, 17),
                                              ((1, 1, 1, 0, 0), 448, 1008, 9, 7), ((5, 5, 1, 2, 2), 48, 32, 9, 7)])
def test_conv_is_batch_invariant(cls, Cin, Cout, H, W):
    """An image's rows from a B = 1 call against its rows inside a B = 3 call at position 2 (289 rows per image at 17 x 17: the image starts in
    the middle of a tile)."""
    KH, KW, stride, ph, pw = cls
    g = IU.gen(77 + Cin + Cout)
    x = torch.randn(3, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, KH, KW, generator=g) / math.sqrt(KH * KW * Cin)
    bias = torch.randn(Cout, generator=g)
    three, _, _ = _run_conv(x, w, bias, stride, (ph, pw), True, 4)
    one, _, _ = _run_conv(x[2:3], w, bias, stride, (ph, pw), True, 4)
    n = one.shape[0]
    assert three.shape[0] == 3 * n
    assert torch.equal(three[2 * n:], one)


def test_conv_without_bias_is_the_plain_product():
    """The fc head: H = W = 1, no bias, no ReLU."""
    g = IU.gen(5)
    x = torch.randn(5, 2048, 1, 1, generator=g)
    w = torch.randn(1008, 2048, 1, 1, generator=g) / math.sqrt(2048)
    out, buf, view = _run_conv(x, w, None, 1, (0, 0), False, 0, c0=0, ldo_extra=0)
    ref = x.double().reshape(5, 2048) @ w.double().reshape(1008, 2048).t()
    mag = x.double().abs().reshape(5, 2048) @ w.double().abs().reshape(1008, 2048).t()
    assert bool(((out.cpu().double() - ref).abs() <= (2048 + 2) * U * mag).all())
    assert sentinels_intact(buf, view.numel(), SENT)


# ---- pools ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(9, 7), (35, 35)])
@pytest.mark.parametrize("C", [5, 288])
@pytest.mark.parametrize("mode", ["max_s2", "max_s1p1", "avg_s1p1", "global_avg"])
def test_pools_match_float64(mode, C, H, W):
    from fourm.utils.inception import ops
    B, c0 = 2, 7
    g = IU.gen(300 + C + H)
    x = torch.randn(B, C, H, W, generator=g)
    xr = _padded_rows(IU.to_rows(x), C + 3)
    Ho, Wo = ops.pool_out_size(mode, H, W)
    buf, view = sentinel_view((B * Ho * Wo, c0 + C + 6), torch.float32, DEV, SENT)
    out = view[:, c0:c0 + C]
    ops.pool2d_nhwc(xr, B, H, W, mode, out)
    got = out.cpu().double()
    x64 = x.double()
    if mode == "max_s2":
        assert torch.equal(got, IU.to_rows(F.max_pool2d(x64, 3, 2)))
    elif mode == "max_s1p1":
        assert torch.equal(got, IU.to_rows(F.max_pool2d(x64, 3, 1, 1)))
    elif mode == "avg_s1p1":
        ref = F.avg_pool2d(x64, 3, 1, 1, count_include_pad=False)
        assert float((got - IU.to_rows(ref)).abs().max()) <= 10 * U * float(x64.abs().max())
        img = IU.from_rows(got, B, H, W)
        corner = x64[:, :, 0:2, 0:2].sum(dim=(2, 3)) / 4.0             # 4 valid taps
        edge = x64[:, :, 0:2, 0:3].sum(dim=(2, 3)) / 6.0               # 6 valid taps
        assert float((img[:, :, 0, 0] - corner).abs().max()) <= 10 * U * float(x64.abs().max())
        assert float((img[:, :, 0, 1] - edge).abs().max()) <= 10 * U * float(x64.abs().max())
    else:
        ref = x64.mean(dim=(2, 3))
        bound = (H * W + 1) * U * x64.abs().mean(dim=(2, 3))
        assert bool(((got - ref).abs() <= bound).all()), float(((got - ref).abs() / bound).max())
    assert _slice_untouched(buf, view, c0, C)
    again_buf, again_view = sentinel_view((B * Ho * Wo, c0 + C + 6), torch.float32, DEV, SENT)
    ops.pool2d_nhwc(xr, B, H, W, mode, again_view[:, c0:c0 + C])
    assert torch.equal(again_view, view)


# ---- preprocess ----------------------------------------------------------------------------------------------------------------------
def _bytes_scale(rows, B):
    """rows (B*299*299, 3) in (v - 128) / 128 -> (B, 3, 299, 299) float64 on the 0..255 scale (exact: a power-of-two scale and a small integer)."""
    return IU.from_rows(rows.cpu().double(), B, IU.SIZE, IU.SIZE) * 128.0 + 128.0


@pytest.mark.parametrize("H,W", [(64, 48), (299, 299), (448, 448)])
def test_preprocess_uint8(H, W):
    from fourm.utils.inception import ops
    imgs = torch.randint(0, 256, (2, 3, H, W), generator=IU.gen(H + W), dtype=torch.uint8)
    got = _bytes_scale(ops.inception_preprocess(imgs.to(DEV)), 2)
    ref = IU.tf1_resize(IU.to_bytes(imgs, False))
    assert float((got - ref).abs().max()) <= 8 * U * 255
    if H == 299:
        assert torch.equal(got, imgs.double())                         # identity weights: every output is its byte
    again = _bytes_scale(ops.inception_preprocess(imgs.to(DEV)), 2)
    assert torch.equal(again, got)


@pytest.mark.parametrize("H,W", [(64, 48), (299, 299)])
def test_preprocess_normalized_fp32(H, W):
    from fourm.utils.inception import ops
    g = IU.gen(9 + H)
    imgs = torch.rand(2, 3, H, W, generator=g)
    flat = imgs.view(-1)
    special = torch.tensor([1.0, 0.0, 0.999, 0.5, 1.5, -0.2, 254.5 / 255.0, 127.0 / 255.0, 1.0 / 255.0, 0.99999994, 200.0 / 255.0, 3.0 / 255.0])
    flat[:special.numel()] = special
    flat[-special.numel():] = special
    got = _bytes_scale(ops.inception_preprocess(imgs.to(DEV), normalize=True), 2)
    by = IU.to_bytes(imgs, True)
    assert float(by.max()) == 255.0 and float(by.min()) == 0.0 and bool((by == by.round()).all())
    ref = IU.tf1_resize(by)
    assert float((got - ref).abs().max()) <= 8 * U * 255
    if H == 299:
        assert torch.equal(got, by)                                    # one tap of weight 1 per output: the byte conversion, exactly


def test_preprocess_refuses_wrong_dtypes():
    from fourm.utils.inception import ops
    with pytest.raises(TypeError):
        ops.inception_preprocess(torch.zeros(1, 3, 8, 8, device=DEV), normalize=False)
    with pytest.raises(TypeError):
        ops.inception_preprocess(torch.zeros(1, 3, 8, 8, dtype=torch.uint8, device=DEV), normalize=True)
    with pytest.raises(ValueError):
        ops.inception_preprocess(torch.zeros(1, 1, 8, 8, dtype=torch.uint8, device=DEV))


# ---- moments -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,d", [(1, 4), (37, 20), (50, 2048)])
def test_feature_moments_are_the_sequential_float64_sums(n, d):
    from fourm.utils.inception import ops
    g = IU.gen(n + d)
    a, b = torch.randn(n, d, generator=g) * 3.0, torch.randn(n, d, generator=g) + 0.5
    sbuf, s = sentinel_view((d,), torch.float64, DEV, SENT)
    obuf, o = sentinel_view((d, d), torch.float64, DEV, SENT)
    cbuf, c = sentinel_view((1,), torch.int64, DEV, -7777)
    s.zero_(), o.zero_(), c.zero_()
    for part in (a, b):                                                # accumulated over two calls
        ops.feature_moments(_padded_rows(part, d + 3), s, o, c)
    rs, ro, rn = IU.moments(torch.cat([a, b]))
    assert int(c.item()) == rn == 2 * n
    assert np.array_equal(s.cpu().numpy(), rs)                         # bit for bit
    assert np.array_equal(o.cpu().numpy(), ro)
    assert sentinels_intact(sbuf, d, SENT) and sentinels_intact(obuf, d * d, SENT) and sentinels_intact(cbuf, 1, -7777)
