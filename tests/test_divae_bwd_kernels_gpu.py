"""The four backward kernels of the detokenizer's fp32 mode (csrc/unet_f32_bwd.hip) on a real MI355X, each alone: fm_unet_col2im_f32,
fm_groupnorm_nhwc_bwd_f32, fm_unet_attention_bwd_f32, fm_silu_bwd_f32 against float64 torch autograd of the upstream operation.

The rule is the one of tests/test_divae_fp32_gpu.py, per output tensor: max |HIP - float64| <= 8 x max(own, 2^-24 max |float64|), own = max |the
same torch expression in float32 on the CPU - float64|; the floor is half an fp32 ulp of the tensor's largest entry.  Every output buffer has a
sentinel row behind it and sentinel columns beside it, which must keep their bits; every kernel runs twice and must repeat its bits."""
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ml-4m_amd"))
from tests.parity_log import record  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = 7.0
FACTOR = 8.0
U = 2.0 ** -24


def _ops():
    from fourm.hip import ops, _lib
    return ops, _lib


def randn(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def sentinel(rows, cols, ld):
    """(rows + 1, ld) buffer full of the sentinel and its (rows, cols) view."""
    buf = torch.full((rows + 1, ld), SENT, device=DEV, dtype=torch.float32)
    return buf, buf[:rows, :cols]


def untouched(buf, rows, cols):
    mask = torch.ones(buf.shape, dtype=torch.bool, device=buf.device)
    mask[:rows, :cols] = False
    return bool((buf[mask] == SENT).all())


def grads(fn, inputs, weights, dtype):
    """d <fn(inputs), weights> / d inputs on the CPU in ``dtype``"""
    xs = [t.detach().to(dtype).clone().requires_grad_(True) for t in inputs]
    (fn(*xs) * weights.to(dtype)).sum().backward()
    return [t.grad.detach() for t in xs]


def under_the_rule(kernel, case, name, got, ref64, ref32):
    err = float((got.double().cpu() - ref64).abs().max())
    own = float((ref32.double() - ref64).abs().max())
    floor = U * float(ref64.abs().max())
    ratio = err / max(own, floor)
    print(f"{kernel} {case} {name}: err {err:.3e}, own {own:.3e}, floor {floor:.3e}, ratio {ratio:.3g} (bound {FACTOR:g})")
    record("divae.fp32.grad", case=f"{kernel} {case}", tensor=name, err_vs_float64=err, cpu_fp32_err_vs_float64=own, floor=floor, ratio=ratio)
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(ref64.shape)
    assert err <= FACTOR * max(own, floor), (kernel, case, name, err, own, floor)


# ------------------------------------------------------------------------------------------------
# fm_unet_col2im_f32
# ------------------------------------------------------------------------------------------------
def im2col_torch(x, B, H, W, C, stride, up1):
    """x rows (B * (H >> up1) * (W >> up1), C) -> (B * Ho * Wo, 9 C), columns tap * C + c: nearest up-sampling, zero border, F.unfold"""
    a = x.view(B, H >> up1, W >> up1, C).permute(0, 3, 1, 2)
    if up1:
        a = a.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
    cols = F.unfold(a, 3, padding=1, stride=stride)                # (B, C * 9, L), rows ordered (c, tap)
    L_ = cols.shape[2]
    return cols.view(B, C, 9, L_).permute(0, 3, 2, 1).reshape(B * L_, 9 * C)


COL2IM = [  # (B, H, W, C) of the source feature map, stride, up1, ld, accumulate
    (2, 5, 5, 4, 1, 0, 4, 0),
    (2, 6, 6, 8, 2, 0, 12, 0),       # ld > C
    (1, 5, 5, 4, 2, 0, 4, 1),        # odd size, Ho = 3; accumulate onto a non-zero buffer
    (2, 3, 3, 8, 1, 1, 8, 0),        # read on the up-sampled 6 x 6 grid: 36 taps per inner source pixel
]


@pytest.mark.parametrize("B,Hs,Ws,C,stride,up1,ld,accumulate", COL2IM)
def test_col2im(B, Hs, Ws, C, stride, up1, ld, accumulate):
    H, W = Hs << up1, Ws << up1                                    # the forward's logical grid
    ops, L = _ops()
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    Rs = B * (H >> up1) * (W >> up1)
    col = randn(B * Ho * Wo, 9 * C, seed=1)
    x0 = randn(Rs, C, seed=2)
    fn = lambda x: im2col_torch(x, B, H, W, C, stride, up1)
    prev = randn(Rs, C, seed=3) if accumulate else torch.zeros(Rs, C)
    ref64 = grads(fn, [x0], col, torch.float64)[0] + prev.double()
    ref32 = grads(fn, [x0], col, torch.float32)[0] + prev
    ldc = 9 * C + 4
    colbuf = torch.full((B * Ho * Wo, ldc), float("nan"), device=DEV)
    colbuf[:, :9 * C] = col.to(DEV)
    outs = []
    for _ in range(2):
        buf, out = sentinel(Rs, C, ld)
        out.copy_(prev.to(DEV))
        L.check(L.unet_col2im_f32(ops._p(colbuf), ldc, ops._p(out), ld, C, B, H, W, 3, stride, up1, accumulate, ops._stream()))
        assert untouched(buf, Rs, C)
        outs.append(out.clone())
    assert torch.equal(outs[0], outs[1])
    under_the_rule("col2im", f"B{B} H{H} W{W} C{C} s{stride} up{up1} ld{ld} acc{accumulate}", "dsrc", outs[0], ref64, ref32)
    if not accumulate:
        # the adjoint identity against the FORWARD kernel: <im2col(x), c> = <x, col2im(c)>; im2col copies, col2im sums <= 36 terms per element
        xg = x0.to(DEV).contiguous()
        fw = torch.empty(B * Ho * Wo, 9 * C, device=DEV)
        L.check(L.unet_im2col_f32(ops._p(xg), C, C, None, 0, 0, 0, 0, ops._p(fw), 9 * C, 9 * C, B, H, W, 3, stride, up1, ops._stream()))
        lhs = float((fw.double().cpu() * col.double()).sum())
        rhs = float((x0.double() * outs[0].double().cpu()).sum())
        tol = 36 * U * float((x0.double().abs() * grads(fn, [x0], col.abs(), torch.float64)[0]).sum())
        assert abs(lhs - rhs) <= tol, (lhs, rhs, tol)


# ------------------------------------------------------------------------------------------------
# fm_groupnorm_nhwc_bwd_f32
# ------------------------------------------------------------------------------------------------
def gn_torch(silu, B, HW, C):
    def fn(x, w, b, add=None):
        z = x.view(B, HW, C).permute(0, 2, 1)
        if add is not None:
            z = z + add[:, :, None]
        y = F.group_norm(z, 32, w, b, 1e-5)
        y = F.silu(y) if silu else y
        return y.permute(0, 2, 1).reshape(B * HW, C)
    return fn


@pytest.mark.parametrize("with_add", [False, True])
@pytest.mark.parametrize("silu", [0, 1])
@pytest.mark.parametrize("B,HW,C", [(2, 5, 64), (3, 16, 96), (1, 4, 128)])
def test_groupnorm_backward(B, HW, C, silu, with_add):
    ops, L = _ops()
    R = B * HW
    x, dy = randn(R, C, seed=4, scale=1.5) + 0.3, randn(R, C, seed=5)
    w, b = 1.0 + randn(C, seed=6, scale=0.1), randn(C, seed=7, scale=0.05)
    ins = [x, w, b] + ([randn(B, C, seed=8, scale=0.5)] if with_add else [])
    fn = gn_torch(silu, B, HW, C)
    ref64, ref32 = grads(fn, ins, dy, torch.float64), grads(fn, ins, dy, torch.float32)
    ldx, lddy, lddx, ld_add = C + 4, C + 8, C + 12, C + 4
    xb = torch.full((R, ldx), float("nan"), device=DEV); xb[:, :C] = x.to(DEV)
    dyb = torch.full((R, lddy), float("nan"), device=DEV); dyb[:, :C] = dy.to(DEV)
    ab = None
    if with_add:
        ab = torch.full((B, ld_add), float("nan"), device=DEV); ab[:, :C] = ins[3].to(DEV)
    wg, bg = w.to(DEV), b.to(DEV)
    scratch = torch.empty(2 * B * C, device=DEV)
    runs = []
    for _ in range(2):
        dxbuf, dx = sentinel(R, C, lddx)
        wbuf, dwb = sentinel(2, C, C + 4)                          # row 0: dw, row 1: db
        dabuf, dadd = sentinel(B, C, ld_add)
        L.check(L.groupnorm_nhwc_bwd_f32(ops._p(dyb), lddy, ops._p(xb), ldx, ops._p(ab), ld_add if with_add else 0, ops._p(wg), ops._p(bg), ops._p(dx), lddx,
                                         ops._p(dwb[0]), ops._p(dwb[1]), ops._p(dadd) if with_add else None, ld_add if with_add else 0, ops._p(scratch),
                                         B, HW, C, 32, 1e-5, silu, ops._stream()))
        assert untouched(dxbuf, R, C) and untouched(wbuf, 2, C)
        assert untouched(dabuf, B, C) if with_add else bool((dabuf == SENT).all())
        runs.append((dx.clone(), dwb[0].clone(), dwb[1].clone(), dadd.clone()))
    assert all(torch.equal(a, c) for a, c in zip(*runs))
    case = f"B{B} HW{HW} C{C} silu{silu} add{int(with_add)}"
    for i, name in enumerate(("dx", "dw", "db", "dadd")[:len(ins)]):
        under_the_rule("gn_bwd", case, name, runs[0][i], ref64[i], ref32[i])
    # dw and db may be switched off one by one: the other keeps its bits, dx too
    dxbuf, dx = sentinel(R, C, lddx)
    only_db = torch.full((C,), SENT, device=DEV)
    L.check(L.groupnorm_nhwc_bwd_f32(ops._p(dyb), lddy, ops._p(xb), ldx, ops._p(ab), ld_add if with_add else 0, ops._p(wg), ops._p(bg), ops._p(dx), lddx,
                                     None, ops._p(only_db), None, 0, ops._p(scratch), B, HW, C, 32, 1e-5, silu, ops._stream()))
    assert torch.equal(dx, runs[0][0]) and torch.equal(only_db, runs[0][2])


# ------------------------------------------------------------------------------------------------
# fm_unet_attention_bwd_f32
# ------------------------------------------------------------------------------------------------
def attn_torch(B, T, heads, ch):
    def fn(qkv):                                                   # QKVAttentionLegacy on rows (B * T, heads * 3 * ch)
        q, k, v = qkv.view(B, T, heads * 3 * ch).permute(0, 2, 1).reshape(B * heads, 3 * ch, T).split(ch, dim=1)
        scale = 1 / math.sqrt(math.sqrt(ch))
        w = torch.softmax(torch.einsum("bct,bcs->bts", q * scale, k * scale), dim=-1)
        a = torch.einsum("bts,bcs->bct", w, v).reshape(B, heads * ch, T)
        return a.permute(0, 2, 1).reshape(B * T, heads * ch)
    return fn


@pytest.mark.parametrize("B,T,heads,ch", [(2, 4, 1, 64), (2, 16, 1, 64), (1, 49, 2, 32)])
def test_attention_backward(B, T, heads, ch):
    ops, L = _ops()
    C = heads * ch
    qkv, do = randn(B * T, 3 * C, seed=9, scale=1.2), randn(B * T, C, seed=10)
    fn = attn_torch(B, T, heads, ch)
    ref64, ref32 = grads(fn, [qkv], do, torch.float64)[0], grads(fn, [qkv], do, torch.float32)[0]
    ld, lddo, lddqkv = 3 * C + 4, C + 8, 3 * C + 12
    qb = torch.full((B * T, ld), float("nan"), device=DEV); qb[:, :3 * C] = qkv.to(DEV)
    dob = torch.full((B * T, lddo), float("nan"), device=DEV); dob[:, :C] = do.to(DEV)
    scratch = torch.empty(3 * B * heads * T, device=DEV)
    outs = []
    for _ in range(2):
        buf, dqkv = sentinel(B * T, 3 * C, lddqkv)
        L.check(L.unet_attention_bwd_f32(ops._p(qb), ld, ops._p(dob), lddo, ops._p(dqkv), lddqkv, ops._p(scratch), B, T, heads, ch, ops._stream()))
        assert untouched(buf, B * T, 3 * C)
        outs.append(dqkv.clone())
    assert torch.equal(outs[0], outs[1])
    assert not bool((outs[0] == SENT).any())                       # every element of dqkv is written
    under_the_rule("attn_bwd", f"B{B} T{T} heads{heads} ch{ch}", "dqkv", outs[0], ref64, ref32)


# ------------------------------------------------------------------------------------------------
# fm_silu_bwd_f32
# ------------------------------------------------------------------------------------------------
def test_silu_backward():
    ops, L = _ops()
    n = 260
    x = torch.linspace(-20.0, 20.0, n) + randn(n, seed=11, scale=0.01)
    dy = randn(n, seed=12)
    ref64, ref32 = grads(F.silu, [x], dy, torch.float64)[0], grads(F.silu, [x], dy, torch.float32)[0]
    xg, dyg = x.to(DEV), dy.to(DEV)
    outs = []
    for _ in range(2):
        buf = torch.full((n + 4,), SENT, device=DEV)
        L.check(L.silu_bwd_f32(ops._p(dyg), ops._p(xg), ops._p(buf), n, ops._stream()))
        assert bool((buf[n:] == SENT).all())
        outs.append(buf[:n].clone())
    assert torch.equal(outs[0], outs[1])
    under_the_rule("silu_bwd", f"n{n}", "dx", outs[0], ref64, ref32)
