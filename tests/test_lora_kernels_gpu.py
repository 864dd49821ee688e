"""fm_lora_apply / fm_lora_grad (csrc/lora.hip) on a real MI355X, element by element against a float64 restatement on the same inputs.

Bounds (u = 2^-24, fp32 unit roundoff; hulp = half an ulp of a bf16 store, as in tests/test_divae_kernels_gpu.py):
  P = x down^T       fp32 sums of K products in an order the test does not fix: |P - P64| <= E_P = (K + 1) u (|x| |down|^T)
  y += s P up^T      r fused multiply-adds on the kernel's own P, one more for the sum with y, then the store:
                     E = |s| (E_P |up|^T + (r + 2) u (|P64| + E_P) |up|^T) + u (|y| + |s| |P64| |up|^T), + hulp(|want| + E) for a bf16 y
  out (+)= s a^T b   a sum over R rows in any order (the row ranges of different workgroups meet in atomics), the scale, and one
                     rounding per workgroup partial added to the output: (R + 3 + splits) u (|out| + |s| |a|^T |b|)
Pad columns of x / a and every row >= R hold NaN and must not reach a result; pad columns and rows >= R of y and P must keep their bits."""
import ctypes as C
import itertools

import pytest
import torch

from tests.test_divae_kernels_gpu import U, check, hulp

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
SENT = 7.0
BF, F32 = torch.bfloat16, torch.float32
DTYPES = {"bf16": (BF, BF), "bf16_f32y": (BF, F32), "fp32": (F32, F32)}


def _ops():
    from fourm.hip import _lib, ops
    return ops, _lib


def gen(seed):
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    return g


def operand(R, cols, ld, dtype, seed, extra_rows=2):
    """(R + extra, ld) buffer full of NaN with N(0, 1) values in [:R, :cols]; -> (buffer, the values as float64)."""
    buf = torch.full((R + extra_rows, ld), NAN, dtype=dtype, device=DEV)
    buf[:R, :cols] = torch.randn(R, cols, generator=gen(seed)).to(DEV).to(dtype)
    return buf, buf[:R, :cols].double()


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32).clone()


def apply_case(R, K, N, r, xdt, ydt, seed, backward=False, scale=0.75):
    """One launch; returns the worst err / bound of P and of y.  backward: x is dY (R, K = out_features), y is dX (R, N = in_features)."""
    ops, _ = _ops()
    ldx, ldy = K + 8, N + 4
    x, x64 = operand(R, K, ldx, xdt, seed)
    y, y64 = operand(R, N, ldy, ydt, seed + 1)
    y_before = bits(y)
    in_f, out_f = (N, K) if backward else (K, N)
    down = (torch.randn(r, in_f, generator=gen(seed + 2)) / r).to(DEV)
    up = (torch.randn(out_f, r, generator=gen(seed + 3)) * 0.3).to(DEV)
    p = torch.full((R + 1, r), SENT, dtype=F32, device=DEV)
    ops.lora_apply(x, down, up, y, scale, p, R, K, N, backward=backward)
    torch.cuda.synchronize()
    # P = x a, y += s P b: forward a = down^T, b = up^T; backward Q = dY up, dX += s Q down
    a64, b64 = (up.double(), down.double()) if backward else (down.double().t(), up.double().t())
    P64 = x64 @ a64
    E_P = (K + 1) * U * (x64.abs() @ a64.abs())
    rp = check(f"P R={R} K={K} N={N} r={r}", p[:R], P64, E_P)
    assert bool((p[R] == SENT).all()), "P written past row R"
    want = y64 + scale * (P64 @ b64)
    mag = y64.abs() + abs(scale) * (P64.abs() @ b64.abs())
    E = abs(scale) * (E_P @ b64.abs() + (r + 2) * U * ((P64.abs() + E_P) @ b64.abs())) + U * mag
    if ydt == BF:
        E = E + hulp(want.abs() + E)
    ry = check(f"y R={R} K={K} N={N} r={r}", y[:R, :N], want, E)
    after = bits(y)
    keep = torch.ones_like(after, dtype=torch.bool)
    keep[:R, :N] = False
    assert torch.equal(after[keep], y_before[keep]), "y written outside (R, N)"
    assert float((y[:R, :N].double() - y64).abs().max()) > 1e-3          # (the update is really there)
    return rp, ry


@pytest.mark.parametrize("r", [1, 4, 12, 64])
@pytest.mark.parametrize("dt", list(DTYPES))
def test_lora_apply_forward(dt, r):
    """R in {1, 63, 130} (one partial tile, three tiles), K in {64, 200}, N in {64, 136}; r = 64 with K = 200 runs the sliced staging
    (two K slices), r = 64 with N = 328 two N slices."""
    xdt, ydt = DTYPES[dt]
    worst = (0.0, 0.0)
    shapes = list(itertools.product((1, 63, 130), (64, 200), (64, 136)))
    if r == 64:
        shapes.append((70, 200, 328))
    for i, (R, K, N) in enumerate(shapes):
        rp, ry = apply_case(R, K, N, r, xdt, ydt, seed=100 * r + 10 * i)
        worst = (max(worst[0], rp), max(worst[1], ry))
    print(f"lora_apply {dt} r={r}: worst err/bound P {worst[0]:.3g}, y {worst[1]:.3g}")


@pytest.mark.parametrize("r", [1, 4, 12, 64])
@pytest.mark.parametrize("dt", list(DTYPES))
def test_lora_apply_backward_roles(dt, r):
    """dX += s (dY up) down through the transposed element strides; Q = dY up comes back in p_out."""
    xdt, ydt = DTYPES[dt]
    worst = (0.0, 0.0)
    for i, (R, K, N) in enumerate(itertools.product((1, 63, 130), (64, 200), (64, 136))):
        rp, ry = apply_case(R, K, N, r, xdt, ydt, seed=7000 + 100 * r + 10 * i, backward=True)
        worst = (max(worst[0], rp), max(worst[1], ry))
    print(f"lora_apply backward {dt} r={r}: worst err/bound Q {worst[0]:.3g}, dX {worst[1]:.3g}")


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("r", [1, 4, 12, 64])
@pytest.mark.parametrize("adt", [BF, F32], ids=["bf16", "fp32"])
def test_lora_grad(adt, r, accumulate):
    """Both output layouts ((n, r): lora_up's, (r, n): lora_down's); R = 700 spreads the rows over three workgroups per column chunk."""
    ops, _ = _ops()
    scale, worst = -0.5, 0.0
    for i, (R, n, transposed) in enumerate(itertools.product((1, 63, 130, 700), (64, 136, 200), (False, True))):
        a, a64 = operand(R, n, n + 12, adt, 300 * r + i)
        b = torch.full((R + 2, r), NAN, dtype=F32, device=DEV)
        b[:R] = torch.randn(R, r, generator=gen(900 + i)).to(DEV)
        shape = (r, n) if transposed else (n, r)
        out0 = torch.randn(*shape, generator=gen(50 + i)).to(DEV) if accumulate else torch.full(shape, NAN, dtype=F32, device=DEV)
        out = out0.clone()
        ops.lora_grad(a, b, out, scale, R, n, transposed=transposed, accumulate=accumulate)
        torch.cuda.synchronize()
        g64 = scale * (a64.t() @ b[:R].double())
        mag = abs(scale) * (a64.abs().t() @ b[:R].double().abs())
        if accumulate:
            base = out0.double().t() if transposed else out0.double()
            g64, mag = g64 + base, mag + base.abs()
        got = out.t() if transposed else out
        splits = (R + 255) // 256
        worst = max(worst, check(f"grad R={R} n={n} r={r} T={transposed}", got, g64, (R + 3 + splits) * U * mag))
    print(f"lora_grad r={r} accumulate={accumulate}: worst err/bound {worst:.3g}")


def test_argument_refusals():
    _, L = _ops()
    x = torch.zeros(8, 64, dtype=BF, device=DEV)
    y = torch.zeros(8, 64, dtype=BF, device=DEV)
    d = torch.zeros(64, 64, dtype=F32, device=DEV)
    p = torch.zeros(8, 64, dtype=F32, device=DEV)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    X, Y, D, Pp = (C.c_void_p(t.data_ptr()) for t in (x, y, d, p))

    def apply(x=X, ldx=64, down=D, up=D, y=Y, ldy=64, p=Pp, R=8, K=64, N=64, r=4):
        return L.lora_apply(x, ldx, down, K, 1, up, r, 1, y, ldy, 1.0, p, R, K, N, r, 0, 0, st)

    def grad(a=X, lda=64, b=Pp, out=D, R=8, n=64, r=4):
        return L.lora_grad(a, lda, b, out, r, 1, 1.0, 0, R, n, r, 0, st)

    def refused(rc, text):
        assert rc < 0, "the launcher accepted a bad argument"
        assert text in L.lib.fm_last_error().decode(), L.lib.fm_last_error().decode()

    assert apply() == 0 and grad() == 0
    for kw in (dict(x=None), dict(down=None), dict(up=None), dict(y=None), dict(p=None)):
        refused(apply(**kw), "null pointer")
    for kw in (dict(a=None), dict(b=None), dict(out=None)):
        refused(grad(**kw), "null pointer")
    for r in (0, 65, -1):
        refused(apply(r=r), "rank")
        refused(grad(r=r), "rank")
    refused(apply(R=0), ">= 1")
    refused(grad(R=0), ">= 1")
    refused(apply(ldx=66), "multiples of 4")
    refused(apply(ldy=62), "multiples of 4")
    refused(apply(ldx=60), "multiples of 4")                      # a multiple of 4, but narrower than K
    refused(grad(lda=66), "multiple of 4")
    refused(grad(lda=32), "multiple of 4")
    refused(apply(x=C.c_void_p(x.data_ptr() + 2)), "misaligned")
    refused(apply(y=C.c_void_p(y.data_ptr() + 4)), "misaligned")
    refused(grad(a=C.c_void_p(x.data_ptr() + 2)), "misaligned")
    refused(L.lora_apply(X, 64, D, 64, 1, D, 4, 1, Y, 64, 1.0, Pp, 8, 64, 64, 4, 1, 0, st), "fp32 x with bf16 y")
    torch.cuda.synchronize()
    assert float(y.float().abs().max()) == 0.0          # (all-zero operands, and no refused call launched anything)
