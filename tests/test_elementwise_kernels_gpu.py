"""Entry points of csrc/elementwise.hip that no test called directly, on a real MI355X: fm_fold_colscale_grad, fm_scale_rows_bf16,
fm_bf16_to_f32_scaled, the n % 4 != 0 tails of fm_f32_to_bf16, and fm_adamw_shadow (scalar path, element-wise shadow store, tile-to-job
search at job boundaries).  Each is compared element by element with a float64 (or exact) restatement; every bound is derived from the
fp32 unit roundoff u = 2^-24 and written next to its check; padding the kernel must not read holds NaN, padding it must not write holds a
sentinel."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests.parity_log import record

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -24
SENT = 7.0


def _lib():
    from fourm.hip import _lib as L
    return L


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def f32(x):
    return float(np.float32(x))


def refused(rc, text):
    assert rc == -1, f"the launcher returned {rc} for a bad argument"
    msg = _lib().lib.fm_last_error().decode()
    assert text in msg, msg


def within(name, got, ref, tol):
    err = (got.double() - ref).abs()
    bad = ~(err <= tol)
    ratio = float((err / (tol + 1e-300)).max())
    assert not bool(bad.any()), f"{name}: {int(bad.sum())} of {bad.numel()} outside the bound, worst err/tol {ratio:.3g}, first at {bad.nonzero()[0].tolist()}"
    return ratio


def bits16(t):
    return t.contiguous().view(torch.int16)


# ------------------------------------------------------------------------------------------------
# fm_fold_colscale_grad
# ------------------------------------------------------------------------------------------------
def _fold_jobs(shapes, null_gw=(), null_gg=(), seed=0):
    """Host tensors and the job table.  dWp has ld_dwp = cols + 3 with NaN in the padding; gW / ggamma are pre-filled and carry a guard row /
    element."""
    L = _lib()
    g = gen(seed)
    jobs = (L.FoldGradJob * len(shapes))()
    host, dev = [], []
    for i, (r, c) in enumerate(shapes):
        ld = c + 3
        dwp = torch.full((r, ld), float("nan"))
        dwp[:, :c] = torch.randn(r, c, generator=g)
        h = dict(dWp=dwp, W=torch.randn(r, c, generator=g), gamma=torch.randn(c, generator=g), gW=torch.randn(r + 1, c, generator=g),
                 ggamma=torch.randn(c + 1, generator=g))
        d = {k: v.to(DEV) for k, v in h.items()}
        j = jobs[i]
        j.dWp, j.W, j.gamma = d["dWp"].data_ptr(), d["W"].data_ptr(), d["gamma"].data_ptr()
        j.gW = None if i in null_gw else d["gW"].data_ptr()
        j.ggamma = None if i in null_gg else d["ggamma"].data_ptr()
        j.rows, j.cols, j.ld_dwp = r, c, ld
        host.append(h); dev.append(d)
    return jobs, host, dev


def _fold_check(label, shapes, host, dev, null_gw, null_gg):
    worst = 0.0
    torch.cuda.synchronize()
    for i, (r, c) in enumerate(shapes):
        h, gw, gg = host[i], dev[i]["gW"].cpu(), dev[i]["ggamma"].cpu()
        d = h["dWp"][:, :c].double()
        if i in null_gw:
            assert torch.equal(gw, h["gW"]), f"{label} job {i}: gW written through a NULL pointer's neighbour"
        else:
            # gW0 + d * gamma: one product and one sum (or one FMA), each within u of its result:  <= 2 u (|gW0| + |d gamma|)
            t = d * h["gamma"].double()
            worst = max(worst, within(f"{label} job {i} gW", gw[:r], h["gW"][:r].double() + t, 2 * U * (h["gW"][:r].double().abs() + t.abs())))
            assert torch.equal(gw[r], h["gW"][r])
        if i in null_gg:
            assert torch.equal(gg, h["ggamma"])
        else:
            # rows products (u each) summed with the prefill in some order ((rows + 1) u first order), second order in the factor 2
            t = d * h["W"].double()
            tol = 2 * (r + 2) * U * (h["ggamma"][:c].double().abs() + t.abs().sum(0))
            worst = max(worst, within(f"{label} job {i} ggamma", gg[:c], h["ggamma"][:c].double() + t.sum(0), tol))
            assert float(gg[c]) == float(h["ggamma"][c])
    return worst


def test_fold_colscale_grad_mixed_jobs():
    """Four shapes in one launch (the grid is sized by the largest: a small job's out-of-range blocks must do nothing), gW NULL in one job and
    ggamma NULL in another."""
    L = _lib()
    shapes = [(1, 4), (64, 64), (70, 130), (200, 65), (64, 64), (70, 130)]
    null_gw, null_gg = (4,), (5,)
    jobs, host, dev = _fold_jobs(shapes, null_gw, null_gg, seed=1)
    L.check(L.fold_colscale_grad(C.addressof(jobs), len(shapes), stream()))
    record("elementwise_kernels.fold_colscale_grad", worst_err_over_tol=_fold_check("fold", shapes, host, dev, null_gw, null_gg))


def test_fold_colscale_grad_job_limit():
    L = _lib()
    base = [(1, 4), (64, 64), (70, 130), (200, 65), (5, 3), (65, 1)]
    shapes = [base[i % len(base)] for i in range(48)]
    jobs, host, dev = _fold_jobs(shapes, seed=2)
    L.check(L.fold_colscale_grad(C.addressof(jobs), 48, stream()))
    record("elementwise_kernels.fold_colscale_grad_48", worst_err_over_tol=_fold_check("fold48", shapes, host, dev, (), ()))
    jobs49, host49, dev49 = _fold_jobs([(2, 4)] * 49, seed=3)
    refused(L.fold_colscale_grad(C.addressof(jobs49), 49, stream()), "FM_FOLD_MAX_JOBS")
    torch.cuda.synchronize()
    assert all(torch.equal(d["gW"].cpu(), h["gW"]) and torch.equal(d["ggamma"].cpu(), h["ggamma"]) for d, h in zip(dev49, host49))


# ------------------------------------------------------------------------------------------------
# fm_scale_rows_bf16
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,N,pad,rps", [(7, 8, 8, 3), (50, 72, 16, 7), (8200, 4096, 8, 197)])
def test_scale_rows_bf16(R, N, pad, rps):
    """x[r][:] *= s[r // rows_per_sample]: one fp32 multiply and one round-to-nearest-even, so bit-equal to the same two operations in torch.
    R is no multiple of rows_per_sample; the scales include 0, 1 and 1 / 0.9; 8200 x 4096 / 8 pieces exceed 16384 x 256 threads, so the
    grid-stride loop runs."""
    L = _lib()
    g = gen(R + N)
    ld = N + pad
    assert R % rps != 0 and (R * N // 8 > 16384 * 256 or R < 8200)
    x = torch.full((R + 1, ld), SENT, dtype=torch.bfloat16)
    x[:R, :N] = torch.randn(R, N, generator=g).bfloat16()
    ns = (R + rps - 1) // rps
    s = torch.rand(ns, generator=g) * 2
    s[:3] = torch.tensor([0.0, 1.0, 1.0 / 0.9])[:min(3, ns)]
    xd, sd = x.to(DEV), s.to(DEV)
    L.check(L.scale_rows_bf16(xd.data_ptr(), ld, sd.data_ptr(), rps, R, N, stream()))
    want = x.clone()
    want[:R, :N] = (x[:R, :N].float() * s[torch.arange(R) // rps][:, None]).bfloat16()
    assert torch.equal(bits16(xd.cpu()), bits16(want))          # the padding columns and the row past the end included


def test_scale_rows_bf16_refusals():
    L = _lib()
    x = torch.zeros(4, 32, dtype=torch.bfloat16, device=DEV)
    s = torch.ones(4, device=DEV)
    msg = "N, ld multiples of 8; 16-byte aligned"
    refused(L.scale_rows_bf16(x.data_ptr(), 32, s.data_ptr(), 1, 4, 12, stream()), msg)
    refused(L.scale_rows_bf16(x.data_ptr(), 20, s.data_ptr(), 1, 4, 16, stream()), msg)
    refused(L.scale_rows_bf16(x.data_ptr() + 2, 32, s.data_ptr(), 1, 3, 16, stream()), msg)


# ------------------------------------------------------------------------------------------------
# fm_bf16_to_f32_scaled / fm_f32_to_bf16
# ------------------------------------------------------------------------------------------------
SIZES = [1, 3, 4, 5, 1027, 2 * 1024 * 1024 + 5]      # the last one is past the grid cap (2048 blocks x 256 threads x 4): stride loop + scalar tail


@pytest.mark.parametrize("n", SIZES)
def test_bf16_to_f32_scaled(n):
    """dst = scale * float(src): one fp32 multiply, bit-equal to torch.  The values are N(0, 1) bf16 and the scale 1 / 3, so no product is
    subnormal; the element past n keeps its sentinel."""
    L = _lib()
    scale = f32(1.0 / 3.0)
    src = torch.randn(n, generator=gen(n)).bfloat16()
    src[0] = 0.0
    srcd = src.to(DEV)
    dst = torch.full((n + 1,), SENT, device=DEV)
    L.check(L.bf16_to_f32_scaled(srcd.data_ptr(), dst.data_ptr(), n, scale, stream()))
    got = dst.cpu()
    want = src.float() * torch.tensor(scale, dtype=torch.float32)
    assert torch.equal(got[:n].view(torch.int32), want.view(torch.int32)) and float(got[n]) == SENT


@pytest.mark.parametrize("n", SIZES)
def test_f32_to_bf16_tails_and_specials(n):
    """Round to nearest even, bit-equal to torch: exact ties (both directions), +-0, +-inf, the largest finite value (rounds to inf) and NaN
    (stays NaN), in the 4-wide body and in the scalar tail; no subnormal input.  The element past n keeps its sentinel."""
    L = _lib()
    big = float(np.finfo(np.float32).max)
    special = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8), -(1.0 + 3 * 2.0 ** -8), 0.0, -0.0, float("inf"), -float("inf"),
                            big, -big, float("nan"), 1.0 + 2.0 ** -8 + 2.0 ** -20, 1.0 + 2.0 ** -8 - 2.0 ** -20], dtype=torch.float32)
    src = torch.randn(n, generator=gen(n + 1))
    k = min(n, len(special))
    src[:k] = special[:k]
    if n > 2 * len(special):
        src[n - len(special):] = special.flip(0)                # specials in the scalar tail too
    else:
        src[n - 1] = special[(n * 5) % len(special)]
    srcd = src.to(DEV)
    dst = torch.full((n + 1,), SENT, dtype=torch.bfloat16, device=DEV)
    L.check(L.f32_to_bf16(srcd.data_ptr(), dst.data_ptr(), n, stream()))
    got, want = dst.cpu(), src.bfloat16()
    nan = torch.isnan(src)
    assert bool(torch.isnan(got[:n][nan]).all())
    assert torch.equal(bits16(got[:n])[~nan], bits16(want)[~nan]) and float(got[n]) == SENT
    if n >= 11:
        assert float(got[0]) == 1.0 and float(got[1]) == 1.0 + 2.0 ** -6 and math.isinf(float(got[8]))     # ties to even; max finite -> inf


# ------------------------------------------------------------------------------------------------
# fm_adamw_shadow
# ------------------------------------------------------------------------------------------------
class Err:
    """A float64 value with a bound on |computed fp32 value - value|, propagated operation by operation.  Every fp32 operation returns the
    rounding of its exact result on the COMPUTED operands: error = propagated operand error, plus u (w u for sqrt / division, which may be
    a few ulps off) times the largest magnitude the computed result can have.  A contraction to FMA skips a rounding and stays inside."""

    def __init__(self, v, e=None):
        self.v = torch.as_tensor(v, dtype=torch.float64)
        self.e = torch.zeros_like(self.v) if e is None else e

    @staticmethod
    def _rnd(v, prop, w=1.0):
        return Err(v, prop + w * U * (v.abs() + prop))

    def __mul__(a, b):
        return Err._rnd(a.v * b.v, a.v.abs() * b.e + b.v.abs() * a.e + a.e * b.e)

    def __add__(a, b):
        return Err._rnd(a.v + b.v, a.e + b.e)

    def __sub__(a, b):
        return Err._rnd(a.v - b.v, a.e + b.e)

    def __truediv__(a, b):
        lo = b.v.abs() - b.e
        assert bool((lo > 0).all())
        v = a.v / b.v
        return Err._rnd(v, (a.e + v.abs() * b.e) / lo, w=4.0)

    def sqrt(a):
        lo = a.v - a.e
        assert bool((lo > 0).all())
        return Err._rnd(a.v.sqrt(), a.e / (2 * lo.sqrt()), w=4.0)


def adamw64(p, m, v, g, lr, b1, b2, eps, wd, bc1, bc2s, gm):
    """The update of adamw_shadow_kernel, term by term, in float64 with its fp32 error bound: (p, m, v) as Err.  All scalars are the fp32
    values the kernel receives."""
    c = lambda x: Err(float(x))
    ge = Err(g) * c(gm)
    pe = Err(p) * (c(1.0) - c(lr) * c(wd))
    me = c(b1) * Err(m) + (c(1.0) - c(b1)) * ge
    ve = c(b2) * Err(v) + (c(1.0) - c(b2)) * ge * ge
    pe = pe - (c(lr) / c(bc1)) * me / (ve.sqrt() / c(bc2s) + c(eps))
    return pe, me, ve


ADAMW_JOBS = [  # rows, cols, ld_plain (None: no shadow)
    (64, 128, 136),     # vector path, exactly one tile of 8192: the next job starts on a tile boundary
    (3, 77, 80),        # cols % 4 != 0: scalar path
    (130, 68, 70),      # vector update, ld_plain % 4 != 0: element-wise shadow store
    (129, 200, None),   # four tiles, the last one partial; dst_plain = NULL
]


def test_adamw_shadow_three_steps():
    L = _lib()
    g0 = gen(77)
    lr, b1, b2, eps, wd = f32(1e-3), f32(0.9), f32(0.95), f32(1e-8), f32(0.05)
    state, tiles = [], 0
    jobs = (L.AdamWJob * len(ADAMW_JOBS))()
    for i, (r, c, ld) in enumerate(ADAMW_JOBS):
        s = dict(p=torch.randn(r, c, generator=g0).to(DEV), m=(torch.randn(r, c, generator=g0) * 0.1).to(DEV),
                 v=(torch.rand(r, c, generator=g0) * 0.01 + 1e-4).to(DEV), g=torch.zeros(r, c, device=DEV),
                 sh=torch.full((r + 1, ld), SENT, dtype=torch.bfloat16, device=DEV) if ld else None)
        j = jobs[i]
        j.p, j.g, j.m, j.v = s["p"].data_ptr(), s["g"].data_ptr(), s["m"].data_ptr(), s["v"].data_ptr()
        j.dst_plain, j.ld_plain = (s["sh"].data_ptr(), ld) if ld else (None, 0)
        j.rows, j.cols, j.tile_start = r, c, tiles
        tiles += (r * c + 8191) // 8192
        state.append(s)
    assert tiles == 8 and [j.tile_start for j in jobs] == [0, 1, 2, 4]
    table = torch.frombuffer(bytearray(bytes(jobs)), dtype=torch.uint8).to(DEV)      # the job table is a DEVICE pointer
    n_total = sum(r * c for r, c, _ in ADAMW_JOBS)
    worst, worst_ss = {"p": 0.0, "m": 0.0, "v": 0.0}, 0.0
    for step in (1, 2, 3):
        bc1, bc2s = f32(1.0 - b1 ** step), f32(math.sqrt(1.0 - b2 ** step))        # what the launcher computes on the host
        gm = f32(0.5) if step == 2 else 1.0
        before = []
        for s in state:
            s["g"].copy_(torch.randn(s["g"].shape, generator=g0))
            before.append({k: s[k].cpu() for k in ("p", "m", "v", "g")})
        grad_mult = torch.tensor([gm], device=DEV) if step == 2 else None
        # step 3: the device hyper-parameters override the (deliberately wrong) scalar arguments
        hyper = torch.tensor([lr, wd, bc1, bc2s], device=DEV) if step == 3 else None
        lr_arg, wd_arg, step_arg = (99.0, 0.9, 17) if step == 3 else (lr, wd, step)
        sumsq = torch.zeros(1, device=DEV)
        L.check(L.adamw_shadow(table.data_ptr(), len(jobs), tiles, lr_arg, b1, b2, eps, wd_arg, step_arg, grad_mult.data_ptr() if step == 2 else None,
                               hyper.data_ptr() if step == 3 else None, sumsq.data_ptr(), stream()))
        torch.cuda.synchronize()
        ss64 = 0.0
        for i, (s, b) in enumerate(zip(state, before)):
            ref = adamw64(b["p"], b["m"], b["v"], b["g"], lr, b1, b2, eps, wd, bc1, bc2s, gm)
            for name, e in zip("pmv", ref):
                worst[name] = max(worst[name], within(f"step {step} job {i} {name}", s[name].cpu(), e.v, e.e))
            assert torch.equal(s["g"].cpu(), b["g"])
            ss64 += float(b["g"].double().pow(2).sum())
            r, c, ld = ADAMW_JOBS[i]
            if ld:
                sh = s["sh"].cpu()
                assert torch.equal(bits16(sh[:r, :c]), bits16(s["p"].cpu().bfloat16())), f"step {step} job {i}: shadow != bf16(new p)"
                assert bool((sh[:r, c:] == SENT).all()) and bool((sh[r] == SENT).all()), f"step {step} job {i}: shadow padding written"
        # sum of n squares: each square u, partial sums per thread, wave and atomic: depth far below n / 64 + 64
        tol = 2 * (n_total / 64 + 64) * U * ss64
        err = abs(float(sumsq.cpu()[0]) - ss64)
        assert err <= tol, (step, err, tol)
        worst_ss = max(worst_ss, err / tol)
    record("elementwise_kernels.adamw_shadow", worst_err_over_tol=max(worst.values()), p_err_over_tol=worst["p"], m_err_over_tol=worst["m"],
           v_err_over_tol=worst["v"], sumsq_err_over_tol=worst_ss)
