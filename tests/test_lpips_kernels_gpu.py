"""Per-kernel numerics of the LPIPS loss on a real MI355X: the five entry points of csrc/lpips.hip and the two ReLU epilogues of the implicit
convolution (fm_gemm_nt) / FM_EPI_RELU of fm_gemm_f32, each element against float64 of the same, already rounded operands.

Bounds come from the formats: U = 2^-24 is the fp32 unit roundoff, a chain of n fp32 multiply-adds errs by at most n U sum |a_i b_i| (to first
order), a bf16 store by at most 2^-8 |value| (half an ulp at the bottom of a binade).  Where the operands of a bf16-mode kernel are chosen
bf16-representable its own operand rounding is the identity, and a second check shows that it does round operands that are not."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -24
BF = 2.0 ** -8
SENT = 7.0


def _ops():
    from fourm.hip import _lib, ops
    return ops, _lib


def gen(seed):
    return torch.Generator().manual_seed(seed)


def bf_vals(t):
    """f32 tensor whose values are bf16-representable."""
    return t.to(torch.bfloat16).float()


def within(name, got, ref, tol):
    err = (got.double().cpu() - ref.double().cpu()).abs()
    tol = tol.double().cpu().expand_as(err)
    bad = ~(err <= tol)
    assert not bool(bad.any()), f"{name}: {int(bad.sum())} of {err.numel()} outside the bound, worst err/tol {float((err / (tol + 1e-300)).max()):.3g}"


def rows_to_nchw(rows, B, H, W):
    return rows.reshape(B, H, W, -1).permute(0, 3, 1, 2)


def nchw_to_rows(x):
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1])


def padded_rows(src, ld, fill=float("nan")):
    buf = torch.full((src.shape[0], ld), fill, dtype=src.dtype, device=DEV)
    buf[:, :src.shape[1]] = src.to(DEV)
    return buf, buf[:, :src.shape[1]]


# ---- stem -----------------------------------------------------------------------------------------------------------------------------------
MUL = torch.tensor([2.0, 1.0, 0.5])
ADD = torch.tensor([0.25, -0.5, 0.125])          # non-zero: padding applied before the affine would put ADD on the border


def stem_operands(B, H, W, seed):
    """img on a grid of sixteenths: fma(img, MUL, ADD) is exact in fp32 and representable in bf16; w and bias bf16-representable."""
    g = gen(seed)
    img = torch.randint(-16, 17, (B, 3, H, W), generator=g).float() / 16
    w = bf_vals(torch.randn(64, 3, 3, 3, generator=g) * (2.0 / 27) ** 0.5)
    bias = bf_vals(0.1 * torch.randn(64, generator=g))
    return img, w, bias


@pytest.mark.parametrize("B,H,W", [(2, 16, 32), (1, 16, 16)])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
def test_stem_forward(B, H, W, dt):
    ops, _ = _ops()
    img, w, bias = stem_operands(B, H, W, 11)
    s = img.double() * MUL.double()[None, :, None, None] + ADD.double()[None, :, None, None]
    pre = F.conv2d(s, w.double(), bias.double(), padding=1)                               # zero padding of the SCALED image
    mag = F.conv2d(s.abs(), w.double().abs(), bias.double().abs(), padding=1)
    ref = nchw_to_rows(pre.clamp(min=0))
    tol = nchw_to_rows(28 * U * mag) + (BF * nchw_to_rows(pre.abs()) if dt == torch.bfloat16 else 0)
    buf, out = padded_rows(torch.full((B * H * W, 64), SENT, dtype=dt), 72, fill=SENT)
    ops.lpips_stem(img.to(DEV), MUL.to(DEV), ADD.to(DEV), w.reshape(64, 27).contiguous().to(DEV), bias.to(DEV), out, B, H, W)
    within(f"stem {dt}", out, ref, tol)
    assert bool((buf[:, 64:] == SENT).all())
    border_wrong = nchw_to_rows(F.conv2d(F.pad(img.double(), (1, 1, 1, 1)) * MUL.double()[None, :, None, None] + ADD.double()[None, :, None, None], w.double(), bias.double()).clamp(min=0))
    assert float((border_wrong - ref).abs().max()) > 0.05                                # the test would see padding in the wrong space
    if dt == torch.bfloat16:                                                             # operands that are not bf16 values ARE rounded by the kernel
        g = gen(12)
        w2, b2 = torch.randn(64, 27, generator=g) * 0.3, 0.1 * torch.randn(64, generator=g)
        a = torch.empty(B * H * W, 64, dtype=dt, device=DEV)
        b = torch.empty_like(a)
        ops.lpips_stem(img.to(DEV), MUL.to(DEV), ADD.to(DEV), w2.to(DEV), b2.to(DEV), a, B, H, W)
        ops.lpips_stem(img.to(DEV), MUL.to(DEV), ADD.to(DEV), bf_vals(w2).to(DEV), bf_vals(b2).to(DEV), b, B, H, W)
        assert torch.equal(a, b)


@pytest.mark.parametrize("B,H,W", [(2, 16, 32), (1, 16, 16)])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
def test_stem_backward(B, H, W, dt):
    ops, _ = _ops()
    g = gen(21)
    w = torch.randn(64, 3, 3, 3, generator=g) * (2.0 / 27) ** 0.5
    if dt == torch.bfloat16:
        w = bf_vals(w)
    d = (torch.randn(B * H * W, 64, generator=g) * (torch.rand(B * H * W, 64, generator=g) > 0.4)).to(dt)       # masked rows: many zeros
    mul = torch.tensor([1.0 / 0.458, 1.0 / 0.448, 1.0 / 0.450])
    rs = torch.tensor([0.75, -1.5, 0.3])[:B].contiguous()
    x = torch.zeros(B, 3, H, W, dtype=torch.float64, requires_grad=True)
    gx, = torch.autograd.grad(F.conv2d(x, w.double(), padding=1), x, rows_to_nchw(d.double(), B, H, W))
    x2 = torch.zeros(B, 3, H, W, dtype=torch.float64, requires_grad=True)
    gm, = torch.autograd.grad(F.conv2d(x2, w.double().abs(), padding=1), x2, rows_to_nchw(d.double().abs(), B, H, W))
    k = mul.double()[None, :, None, None] * rs.double()[:, None, None, None]
    ref, tol = gx * k, (577 * U * gm + 2 * U * gx.abs()) * k.abs()
    _, dv = padded_rows(d, 72)
    dimg = torch.full((B, 3, H, W), SENT, dtype=torch.float32, device=DEV)
    ops.lpips_stem_bwd(dv, w.reshape(64, 27).contiguous().to(DEV), mul.to(DEV), rs.to(DEV), dimg, B, H, W)
    within(f"stem_bwd {dt}", dimg, ref, tol)
    one = torch.empty_like(dimg)
    ops.lpips_stem_bwd(dv, w.reshape(64, 27).contiguous().to(DEV), mul.to(DEV), None, one, B, H, W)            # row_scale = NULL: 1
    within(f"stem_bwd {dt} unscaled", one, gx * mul.double()[None, :, None, None], (577 * U * gm + U * gx.abs()) * mul.double()[None, :, None, None])


# ---- max-pool -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,Cc", [(2, 4, 6, 64), (1, 2, 2, 128)])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
def test_maxpool_is_exact(B, H, W, Cc, dt):
    ops, _ = _ops()
    x = torch.randn(B * H * W, Cc, generator=gen(31)).clamp(min=0).to(dt)
    ref = nchw_to_rows(F.max_pool2d(rows_to_nchw(x.float(), B, H, W), 2)).to(dt)
    _, xv = padded_rows(x, Cc + 8)
    buf, y = padded_rows(torch.full((B * (H // 2) * (W // 2), Cc), SENT, dtype=dt), Cc + 16, fill=SENT)
    ops.maxpool2x2_nhwc(xv, y, B, H, W, Cc)
    assert torch.equal(y.cpu(), ref) and bool((buf[:, Cc:] == SENT).all())


# ---- tap layer backward ---------------------------------------------------------------------------------------------------------------------
def tap_case(dt, seed=41):
    B, H, W, Cc = 2, 4, 6, 8
    g = gen(seed)
    levels = torch.tensor([0.0, 0.0, 0.5, 1.0, 1.0, 2.0])
    act = levels[torch.randint(0, 6, (B, Cc, H, W), generator=g)]                         # ties among positive values, many zeros
    act[0, :, 0:2, 0:2] = 0.0                                                             # an all-zero window
    act[1, :, 2:4, 4:6] = 1.0                                                             # a window of four equal positive values
    a = act.double().requires_grad_()
    first, = torch.autograd.grad(F.max_pool2d(a, 2).sum(), a)                             # 1 at torch's selected position of each window
    assert float(first[1, 0, 2, 4]) == 1.0 and float(first[1, 0, 2:4, 4:6].sum()) == 1.0   # the first in scan order wins
    rows = lambda t: nchw_to_rows(t).contiguous()
    din = (torch.randn(B * H * W, Cc, generator=g)).to(dt)
    dtap = torch.randn(B * H * W, Cc, generator=g)
    dpool = torch.randn(B * (H // 2) * (W // 2), Cc, generator=g).to(dt)
    up = rows(F.interpolate(rows_to_nchw(dpool.float(), B, H // 2, W // 2), scale_factor=2, mode="nearest")) * rows(first.float())
    return (B, H, W, Cc), rows(act).to(dt), din, dtap, dpool, up


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("use_din,use_tap,use_pool", [(False, False, True), (False, True, False), (False, True, True), (True, True, True), (False, False, False)])
def test_tap_bwd(dt, use_din, use_tap, use_pool):
    ops, _ = _ops()
    (B, H, W, Cc), act, din, dtap, dpool, up = tap_case(dt)
    v = torch.zeros(B * H * W, Cc)
    if use_din:
        v = v + din.float()
    if use_tap:
        v = v + dtap
    if use_pool:
        v = v + up
    ref = torch.where(act.float() > 0, v, torch.zeros_like(v)).to(dt)                     # fp32 sum in the kernel's order, one rounding
    _, av = padded_rows(act, 12)
    buf, d = padded_rows(torch.full((B * H * W, Cc), SENT, dtype=dt), 16, fill=SENT)
    ops.lpips_tap_bwd(av, d, B, H, W, din=padded_rows(din, 12)[1] if use_din else None, dtap=padded_rows(dtap, 12)[1] if use_tap else None,
                      dpool=padded_rows(dpool, 12)[1] if use_pool else None)
    assert torch.equal(d.cpu(), ref) and bool((buf[:, Cc:] == SENT).all())
    assert bool((d.cpu()[act.float() == 0] == 0).all())


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float32])
def test_tap_bwd_in_place_mask(dt):
    ops, _ = _ops()
    (B, H, W, Cc), act, din, _, _, _ = tap_case(dt)
    d = din.clone().to(DEV)
    ops.lpips_tap_bwd(act.to(DEV), d, B, H, W, din=d)
    assert torch.equal(d.cpu(), torch.where(act.float() > 0, din.float(), torch.zeros(())).to(dt))


# ---- distance -------------------------------------------------------------------------------------------------------------------------------
def distance_ref(p, t, w, P):
    """float64: per-row value sum_c w (p^ - t^)^2 / P, the gradient by the documented formula, and the magnitudes the bounds are built from."""
    eps = 1e-10
    n = p.pow(2).sum(1, keepdim=True).sqrt()
    d, dt_ = n + eps, t.pow(2).sum(1, keepdim=True).sqrt() + eps
    ph, th = p / d, t / dt_
    val = (w * (ph - th) ** 2).sum(1) / P
    g = 2 * w * (ph - th) / P
    second = torch.where(n > 0, p * (g * p).sum(1, keepdim=True) / (d * d * torch.where(n > 0, n, torch.ones_like(n))), torch.zeros_like(p))
    grad = g / d - second
    G = 2 * w * (ph.abs() + th.abs()) / P
    gmag = G / d + torch.where(n > 0, p.abs() * (G * p.abs()).sum(1, keepdim=True) / (d * d * torch.where(n > 0, n, torch.ones_like(n))), torch.zeros_like(p))
    vmag = (w * (ph.abs() + th.abs()) ** 2).sum(1) / P
    return val, grad, vmag, gmag


@pytest.mark.parametrize("Cc", [64, 512])
@pytest.mark.parametrize("P", [1, 4, 2304])
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_distance(Cc, P, dt):
    ops, _ = _ops()
    B = 3
    g = gen(50 + Cc + P)
    p = torch.randn(B * P, Cc, generator=g).clamp(min=0).to(dt)
    t = torch.randn(B * P, Cc, generator=g).clamp(min=0).to(dt)
    p[2 * P + P // 2] = 0                                                                 # a pred pixel and a target pixel with every channel zero
    t[1 * P + P // 3] = 0
    w = torch.rand(Cc, generator=g) / Cc
    val, grad, vmag, gmag = distance_ref(p.double(), t.double(), w.double(), P)
    # the formula is autograd's wherever autograd is finite (rows with a non-zero norm)
    pa = p.double().requires_grad_()
    ga, = torch.autograd.grad((w.double() * (pa / (pa.pow(2).sum(1, keepdim=True).sqrt() + 1e-10) - (t.double() / (t.double().pow(2).sum(1, keepdim=True).sqrt() + 1e-10))) ** 2).sum() / P, pa)
    live = torch.isfinite(ga).all(1)
    assert int((~live).sum()) == 1 and float((ga[live] - grad[live]).abs().max()) <= 1e-12 * float(grad[live].abs().max())
    loss0 = torch.tensor([0.5, -0.25, 2.0])
    ref_loss = loss0.double() + val.reshape(B, P).sum(1)
    # loss: <= 64 U on each pixel's value (norms, divisions, the weighted square), <= 32 U for the sums (at most 26 additions deep), 2 U for the final scale and add
    tol_loss = 96 * U * vmag.reshape(B, P).sum(1) + 2 * U * (loss0.double().abs() + ref_loss.abs())
    _, pv = padded_rows(p, Cc + 8)
    _, tv = padded_rows(t, Cc + 4)
    dbuf, dp = padded_rows(torch.full((B * P, Cc), SENT), Cc + 12, fill=SENT)
    scratch = torch.zeros(ops.lpips_distance_scratch(B, P), device=DEV)
    loss = loss0.clone().to(DEV)
    ops.lpips_distance(pv, tv, w.to(DEV), B, P, loss, dp, scratch)
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(dp).all())
    within(f"distance loss C{Cc} P{P}", loss, ref_loss, tol_loss)
    within(f"distance grad C{Cc} P{P}", dp, grad, 64 * U * gmag)
    assert bool((dbuf[:, Cc:] == SENT).all())
    # the same bits on a second run, and without the gradient
    loss2, dp2 = loss0.clone().to(DEV), torch.empty_like(dp)
    ops.lpips_distance(pv, tv, w.to(DEV), B, P, loss2, dp2, scratch)
    loss3 = loss0.clone().to(DEV)
    ops.lpips_distance(pv, tv, w.to(DEV), B, P, loss3, None, scratch)
    assert torch.equal(loss, loss2) and torch.equal(dp, dp2) and torch.equal(loss, loss3)


def test_distance_refusals_leave_the_outputs_untouched():
    ops, L = _ops()
    B, P, Cc = 2, 4, 64
    p = torch.rand(B * P + 1, Cc, device=DEV)
    t = torch.rand(B * P + 1, Cc, device=DEV)
    w = torch.rand(Cc, device=DEV)
    loss = torch.full((B,), SENT, device=DEV)
    dp = torch.full((B * P, Cc), SENT, device=DEV)
    scratch = torch.full((B,), SENT, device=DEV)
    ptr = lambda x, off=0: C.c_void_p(x.data_ptr() + off)

    def call(pred=ptr(p), ldp=Cc, tgt=ptr(t), ldt=Cc, B_=B, P_=P, C_=Cc, dpred=ptr(dp), lddp=Cc):
        return L.lpips_distance(pred, ldp, tgt, ldt, 1, ptr(w), B_, P_, C_, ptr(loss), dpred, lddp, ptr(scratch), ops._stream())

    for kw in (dict(pred=ptr(p, 4)), dict(tgt=ptr(t, 8)), dict(dpred=ptr(dp, 4)), dict(ldp=Cc + 2), dict(lddp=Cc - 4), dict(C_=62), dict(C_=516, ldp=516, ldt=516, lddp=516),
               dict(B_=0), dict(P_=0), dict(P_=-3), dict(C_=0), dict(pred=None)):
        assert call(**kw) == -1, kw
        assert L.lib.fm_last_error().decode().startswith("fm_lpips_distance")
    torch.cuda.synchronize()
    assert bool((loss == SENT).all()) and bool((dp == SENT).all()) and bool((scratch == SENT).all())
    assert call() == 0


# ---- the ReLU epilogues of the implicit convolution --------------------------------------------------------------------------------------
def conv_operands(B, H, W, Cc, N, seed):
    g = gen(seed)
    x = torch.randn(B * H * W, Cc, generator=g).to(torch.bfloat16)
    w = (torch.randn(N, 9 * Cc, generator=g) * (2.0 / (9 * Cc)) ** 0.5).to(torch.bfloat16)          # taps outermost: [n][tap C + c]
    bias = 0.2 * torch.randn(N, generator=g)
    w4 = w.double().reshape(N, 3, 3, Cc).permute(0, 3, 1, 2)
    acc = nchw_to_rows(F.conv2d(rows_to_nchw(x.double(), B, H, W), w4, padding=1))
    mag = nchw_to_rows(F.conv2d(rows_to_nchw(x.double().abs(), B, H, W), w4.abs(), padding=1))
    return x, w, bias, acc, mag


CONV_SHAPES = [(1, 4, 4, 64, 64), (3, 6, 10, 128, 256)]          # M = 180: no multiple of the 128-row tile, two column tiles


@pytest.mark.parametrize("B,H,W,Cc,N", CONV_SHAPES)
def test_conv_relu_epilogue(B, H, W, Cc, N):
    ops, L = _ops()
    x, w, bias, acc, mag = conv_operands(B, H, W, Cc, N, 61)
    b16 = bf_vals(bias).double()                                                          # the epilogue adds bf16(bias)
    pre = acc + b16
    tol = 9 * Cc * U * mag + U * (acc.abs() + b16.abs()) + BF * pre.abs()
    buf, out = padded_rows(torch.full((B * H * W, N), SENT, dtype=torch.bfloat16), N + 8, fill=SENT)
    ops.gemm_nt(x.to(DEV), w.to(DEV), out, epilogue=L.EPI_RELU, bias=bias.to(DEV), M=B * H * W, N=N, K=9 * Cc, conv=dict(C=Cc, H=H, W=W, Ho=H, Wo=W))
    within("conv + FM_EPI_RELU", out, pre.clamp(min=0), tol)
    assert bool((out >= 0).all()) and bool((buf[:, N:] == SENT).all())
    # max(bf16(acc + bias), 0) of the plain launch, bit for bit - of the UNSPLIT plain launch: a small FM_EPI_BF16 convolution may be cut over
    # K (another summation order), the ReLU epilogue never is
    plain = torch.empty(B * H * W, N, dtype=torch.bfloat16, device=DEV)
    L.lib.fm_lab_set(9, 0)
    try:
        ops.gemm_nt(x.to(DEV), w.to(DEV), plain, epilogue=L.EPI_BF16, bias=bias.to(DEV), M=B * H * W, N=N, K=9 * Cc, conv=dict(C=Cc, H=H, W=W, Ho=H, Wo=W))
    finally:
        L.lib.fm_lab_set(9, 1)
    assert torch.equal(out.float(), plain.float().clamp(min=0))


@pytest.mark.parametrize("B,H,W,Cc,N", CONV_SHAPES)
def test_conv_relu_bwd_epilogue(B, H, W, Cc, N):
    ops, L = _ops()
    x, w, _, acc, mag = conv_operands(B, H, W, Cc, N, 62)
    res = torch.randn(B * H * W, N, generator=gen(63)).clamp(min=0).to(torch.bfloat16)
    live = res.double() > 0
    ref = torch.where(live, acc, torch.zeros_like(acc))
    tol = torch.where(live, 9 * Cc * U * mag + BF * acc.abs(), torch.zeros_like(acc))     # masked elements are exactly 0
    _, rv = padded_rows(res, N + (4 if N == 64 else 8))                                   # 8-byte and 16-byte mask loads
    buf, out = padded_rows(torch.full((B * H * W, N), SENT, dtype=torch.bfloat16), N + 8, fill=SENT)
    ops.gemm_nt(x.to(DEV), w.to(DEV), out, epilogue=L.EPI_RELU_BWD, res=rv, M=B * H * W, N=N, K=9 * Cc, conv=dict(C=Cc, H=H, W=W, Ho=H, Wo=W))
    within("conv + FM_EPI_RELU_BWD", out, ref, tol)
    assert bool((buf[:, N:] == SENT).all())


def test_relu_epilogue_refusals_leave_out_untouched():
    ops, L = _ops()
    B, H, W, Cc, N = 1, 4, 4, 64, 64
    x, w, bias, _, _ = conv_operands(B, H, W, Cc, N, 64)
    x, w, bias = x.to(DEV), w.to(DEV), bias.to(DEV)
    res = torch.ones(B * H * W, N, dtype=torch.bfloat16, device=DEV)
    out = torch.full((B * H * W, N), SENT, dtype=torch.bfloat16, device=DEV)
    out2 = torch.full((B * H * W, N), SENT, dtype=torch.bfloat16, device=DEV)
    conv = dict(C=Cc, H=H, W=W, Ho=H, Wo=W)
    xd = torch.zeros(64, 9 * Cc, dtype=torch.bfloat16, device=DEV)                        # a dense launch of the same K (64 rows: the tiled kernels)
    outd = torch.full((64, N), SENT, dtype=torch.bfloat16, device=DEV)
    bad = [lambda: ops.gemm_nt(xd, w, outd, epilogue=L.EPI_RELU, bias=bias),
           lambda: ops.gemm_nt(xd, w, outd, epilogue=L.EPI_RELU_BWD, res=res.repeat(4, 1)),
           lambda: ops.gemm_nt(xd[:16], w, outd, epilogue=L.EPI_RELU, bias=bias, M=16),    # (the few-row route)
           lambda: ops.gemm_nt(x, w, out, epilogue=L.EPI_RELU_BWD, M=B * H * W, N=N, K=9 * Cc, conv=conv),
           lambda: ops.gemm_nt(x, w, out, epilogue=L.EPI_RELU_BWD, res=res, bias=bias, M=B * H * W, N=N, K=9 * Cc, conv=conv),
           lambda: ops.gemm_nt(x, w, out, epilogue=L.EPI_RELU, out2=out2, M=B * H * W, N=N, K=9 * Cc, conv=conv),
           lambda: ops.gemm_nt(x, w, out, epilogue=L.EPI_RELU_BWD, res=res, out2=out2, M=B * H * W, N=N, K=9 * Cc, conv=conv),
           lambda: ops.gemm_nt(x, w, out, epilogue=L.EPI_RELU, res=res, M=B * H * W, N=N, K=9 * Cc, conv=conv)]
    for i, f in enumerate(bad):
        with pytest.raises(RuntimeError, match="fm_gemm_nt"):
            f()
    torch.cuda.synchronize()
    assert bool((out == SENT).all()) and bool((out2 == SENT).all()) and bool((outd == SENT).all())
    xf = torch.zeros(8, 64, device=DEV)
    with pytest.raises(RuntimeError, match="fm_gemm_f32"):
        ops.gemm_nt(xf, torch.zeros(64, 64, device=DEV), torch.zeros(8, 64, device=DEV), epilogue=L.EPI_RELU_BWD)


@pytest.mark.parametrize("ldx", [72, 74])          # 72: the fp32 matrix-core kernel; 74 (row stride not a multiple of 4): the LDS-tiled FMA kernel
def test_gemm_f32_relu(ldx):
    ops, L = _ops()
    M, N, K = 70, 64, 72
    g = gen(71)
    x, w, bias = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) * K ** -0.5, 0.2 * torch.randn(N, generator=g)
    pre = x.double() @ w.double().T + bias.double()
    mag = x.double().abs() @ w.double().abs().T + bias.double().abs()
    _, xv = padded_rows(x, ldx, fill=0.0)
    buf, out = padded_rows(torch.full((M, N), SENT), N + 4, fill=SENT)
    ops.gemm_nt(xv, w.to(DEV), out, epilogue=L.EPI_RELU, bias=bias.to(DEV), M=M, N=N, K=K)
    within("gemm_f32 + FM_EPI_RELU", out, pre.clamp(min=0), (K + 1) * U * mag)
    assert bool((out >= 0).all()) and bool((out == 0).any()) and bool((buf[:, N:] == SENT).all())
