"""The two kernels behind CLIP's vision tower on a real MI355X, element by element against float64:
FM_EPI_QUICK_GELU on every dispatch route of the dense NT GEMM family (and in fm_gemm_f32), and fm_clip_embed_ln (csrc/clip.hip).

QuickGELU bounds (u16 = 2^-8, the unit roundoff of bf16: a correctly rounded store is within u16 |value| / (1 + u16) of the value):
  out2:  |out2 - v| <= u16 |v| + (K + 4) 2^-24 S,  v = x w^T + bf16(bias) in float64, S = |x| |w|^T + |bias| - the rounding of the store plus
         the deterministic bound of a K-term fp32 dot product, the accumulation allowance of tests/test_fp32_kernels_gpu.py;
  out:   |out - q(out2)| <= u16 |q(out2)|, q(p) = p / (1 + exp(-1.702 p)) in float64 on the kernel's OWN out2.  The store alone can reach
         1 / (1 + u16) = 0.996 of that bound (a value just above a power of two, half way between two bf16 numbers); what is left, a
         relative 2^-16 = 1.5e-5, covers the fast exponential (2 ulp), the rounding of its argument (|1.702 p| 2^-24: 1e-6 at |p| = 10)
         and the reciprocal (1 ulp) - about 2e-6 together at the magnitudes used here.  Measured: 0.92 - 0.996 on every route."""
import os

import pytest
import torch
import torch.nn.functional as F

from tests.parity_log import record

pytestmark = pytest.mark.gpu

DEV = "cuda"
U16 = 2.0 ** -8
U = 2.0 ** -24
FN = 2.0 ** -20
SENT = 7.0
bf16 = torch.bfloat16


def _ops():
    from fourm.hip import ops, _lib
    return ops, _lib


def randn(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def q64(p):
    return p / (1.0 + torch.exp(-1.702 * p))


def sentinel(M, N, dtype, ld=None):
    """(M, N) view of an (M + 1, ld) buffer full of the sentinel."""
    ld = ld or N + 8
    buf = torch.full((M + 1, ld), SENT, device=DEV, dtype=dtype)
    return buf, buf[:M, :N]


def untouched(buf, M, N):
    keep = torch.ones_like(buf, dtype=torch.bool)
    keep[:M, :N] = False
    return bool((buf[keep] == SENT).all())


def worst(err, tol):
    return float((err / (tol + 1e-300)).max())


# route -> (M, N, K, lab): the smallest shape the route's own condition admits, M never a multiple of the tile height.
#   skinny   M <= 32 (gemm_skinny.hip; K >= 64)                       tile128  M <= 128: 128 x 128 tiles of gemm.hip
#   auto_k   M > 128, K < 1536: configuration 11 (128 x 256)           auto_kl  K >= 1536: configuration 10
#   auto_256 N % 256 == 0 and the 256 x 256 tiling fills the chip in whole rounds (256 tiles): configuration 12
#   nt3_192 / nt3_256  the staged lock-step kernel (gemm_nt3.hip; M >= 2048, gated by FOURM_NT3_LAB bit 131072 as for FM_EPI_GELU)
ROUTES = {
    "skinny": (7, 44, 64, 0),
    "tile128": (100, 76, 64, 0),
    "auto_k": (200, 320, 128, 0),
    "auto_kl": (200, 136, 1536, 0),
    "auto_256": (255 * 256 + 20, 256, 64, 0),
    "nt3_192": (2050, 192, 128, 131072),
    "nt3_256": (2050, 256, 128, 131072),
}


def launch(route, x, w, out, **kw):
    ops, L = _ops()
    lab = ROUTES[route][3]
    base = int(os.environ.get("FOURM_NT3_LAB", "0"))
    if lab:
        L.lib.fm_lab_set(3, base | lab)
    try:
        ops.gemm_nt(x, w, out, epilogue=L.EPI_QUICK_GELU, **kw)
    finally:
        if lab:
            L.lib.fm_lab_set(3, base)


@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("route", list(ROUTES))
def test_quick_gelu_epilogue(route, with_bias):
    M, N, K, _ = ROUTES[route]
    seed = 100 + 7 * list(ROUTES).index(route)
    x = randn(M, K, seed=seed).to(bf16)
    w = randn(N, K, scale=K ** -0.5, seed=seed + 1).to(bf16)
    bias = randn(N, scale=0.5, seed=seed + 2) if with_bias else None
    ld = 320 if route.startswith("nt3") else None                               # the staged epilogue wants whole 128-byte rows
    obuf, out = sentinel(M, N, bf16, ld)
    pbuf, pre = sentinel(M, N, bf16, ld)
    launch(route, x, w, out, bias=bias, out2=pre)
    b64 = bias.to(bf16).double() if with_bias else torch.zeros(N, device=DEV, dtype=torch.float64)
    v = x.double() @ w.double().t() + b64
    S = x.double().abs() @ w.double().abs().t() + b64.abs()
    tol_pre = U16 * v.abs() + (K + 4) * U * S
    e_pre = (pre.double() - v).abs()
    want = q64(pre.double())
    e_out = (out.double() - want).abs()
    r_pre, r_out = worst(e_pre, tol_pre), worst(e_out, U16 * want.abs())
    print(f"quick_gelu {route} bias={with_bias} M={M} N={N} K={K}: out2 err/tol {r_pre:.3f}, out err/tol {r_out:.3f}")
    record("clip.quick_gelu", route=route, bias=with_bias, M=M, N=N, K=K, pre_err_over_tol=r_pre, out_err_over_tol=r_out)
    assert bool(torch.isfinite(out.float()).all())
    assert bool((e_pre <= tol_pre).all()), (route, r_pre)
    assert bool((e_out <= U16 * want.abs()).all()), (route, r_out)
    assert untouched(obuf, M, N) and untouched(pbuf, M, N)
    # without the second output: the same activation bits
    obuf2, out_b = sentinel(M, N, bf16, ld)
    launch(route, x, w, out_b, bias=bias)
    assert torch.equal(out_b, out) and untouched(obuf2, M, N)


@pytest.mark.parametrize("route", ["skinny", "auto_k"])
def test_quick_gelu_saturates_without_nan(route):
    """A bias of +-1e4: exp overflows to inf on one side and underflows to 0 on the other; out is -0 / +0 or the pre-activation itself."""
    M, N, K, _ = ROUTES[route]
    x, w = randn(M, K, seed=5).to(bf16), randn(N, K, scale=K ** -0.5, seed=6).to(bf16)
    bias = torch.where(torch.arange(N, device=DEV) % 2 == 0, 1e4, -1e4).float()
    _, out = sentinel(M, N, bf16)
    _, pre = sentinel(M, N, bf16)
    launch(route, x, w, out, bias=bias, out2=pre)
    o, p = out.float(), pre.float()
    assert not bool(torch.isnan(o).any()) and bool((p.abs() > 9e3).all())
    assert bool(((o == 0) | (o == p)).all())
    assert bool((o[:, 0::2] == p[:, 0::2]).all()) and bool((o[:, 1::2] == 0).all())


@pytest.mark.parametrize("form", ["mfma", "fma"])
def test_quick_gelu_f32(form):
    """fm_gemm_f32 (both kernels: 16-byte aligned rows take the fp32 matrix cores, an odd row stride the FMA kernel) with the rule of the
    "gelu" case of tests/test_fp32_kernels_gpu.py: the dot-product bound tv = (K + 4) u S carried through the slope (|q'| <= 1.11 < 1.2),
    4 u |v| for the rounding of the exponent's argument and FN |q(v)| for expf and the division; out2 within tv."""
    ops, L = _ops()
    M, N, K = 129, 130, 36
    xb = torch.zeros(M, K + (0 if form == "mfma" else 1), device=DEV)
    x = xb[:, :K]
    x.copy_(randn(M, K, seed=11))
    w = randn(N, K, scale=K ** -0.5, seed=12)
    bias = randn(N, seed=13)
    obuf, out = sentinel(M, N, torch.float32)
    pbuf, pre = sentinel(M, N, torch.float32)
    ops._gemm_f32(x, w, out, epilogue=L.EPI_QUICK_GELU, bias=bias, out2=pre)
    v = x.double() @ w.double().t() + bias.double()
    tv = (K + 4) * U * (x.double().abs() @ w.double().abs().t() + bias.double().abs())
    tol = 1.2 * tv + 4 * U * v.abs() + FN * q64(v).abs()
    e_out, e_pre = (out.double() - q64(v)).abs(), (pre.double() - v).abs()
    print(f"quick_gelu f32 {form}: out err/tol {worst(e_out, tol):.3f}, out2 err/tol {worst(e_pre, tv):.3f}")
    assert bool((e_out <= tol).all()) and bool((e_pre <= tv).all())
    assert untouched(obuf, M, N) and untouched(pbuf, M, N)
    big = torch.where(torch.arange(N, device=DEV) % 2 == 0, 1e4, -1e4).float()
    ops._gemm_f32(x, w, out, epilogue=L.EPI_QUICK_GELU, bias=big, out2=pre)
    assert not bool(torch.isnan(out).any()) and bool(((out == 0) | (out == pre)).all())


# ------------------------------------------------------------------------------------------------
# fm_clip_embed_ln
# ------------------------------------------------------------------------------------------------
def clip_embed_ln(patches, f32_rows, cls, pos, w, b, out, B, G, D, eps=1e-5, ldp=None, ldo=None):
    ops, L = _ops()
    ldp = ldp if ldp is not None else patches.stride(0) if patches is not None else D
    ldo = ldo if ldo is not None else out.stride(0) if out is not None else D
    return L.clip_embed_ln(ops._p(patches), ldp, 1 if f32_rows else 0, ops._p(cls), ops._p(pos), ops._p(w), ops._p(b), ops._p(out), ldo, B, G, D, eps,
                           ops._stream())


@pytest.mark.parametrize("rows_f32", [False, True], ids=["bf16", "f32"])
@pytest.mark.parametrize("B,G,D", [(3, 16, 128), (2, 9, 192), (1, 1, 64), (2, 3, 2048)])
def test_clip_embed_ln(B, G, D, rows_f32):
    """Every output element against float64 within 8 x the largest error of F.layer_norm in float32 on the same rows (the project's fp32 rule,
    tests/test_divae_f32_kernels_gpu.py).  Patch rows and the stream have padded leading dimensions; NaN in the pad columns and in the rows
    past the live count of the input must not be read, the sentinel around the output must stay."""
    _, L = _ops()
    seed = B + 3 * G + D
    dt = torch.float32 if rows_f32 else bf16
    src = torch.full((B * G + 2, D + 8), float("nan"), device=DEV, dtype=dt)
    src[:B * G, :D] = randn(B * G, D, seed=seed).to(dt)
    cls, pos = randn(D, scale=0.5, seed=seed + 1), randn(G + 1, D, scale=0.5, seed=seed + 2)
    w, b = 1.0 + 0.2 * randn(D, seed=seed + 3), 0.1 * randn(D, seed=seed + 4)
    R = B * (G + 1)
    obuf, out = sentinel(R, D, torch.float32, D + 4)
    L.check(clip_embed_ln(src, rows_f32, cls, pos, w, b, out, B, G, D))
    rows = torch.cat([cls.double().expand(B, 1, D), src[:B * G, :D].double().view(B, G, D)], 1) + pos.double()
    ref = F.layer_norm(rows, (D,), w.double(), b.double(), 1e-5).view(R, D)
    own = F.layer_norm(rows.float().cpu(), (D,), w.cpu(), b.cpu(), 1e-5).view(R, D)
    err = float((out.double() - ref).abs().max())
    own_err = float((own.double() - ref.cpu()).abs().max())
    print(f"clip_embed_ln B={B} G={G} D={D} f32={rows_f32}: kernel vs float64 {err:.3e}, torch fp32 vs float64 {own_err:.3e}, ratio {err / own_err:.3g}")
    record("clip.embed_ln", B=B, G=G, D=D, rows_f32=rows_f32, err=err, torch_fp32_err=own_err)
    assert bool(torch.isfinite(out).all())
    assert err <= 8 * own_err, (err, own_err)
    assert untouched(obuf, R, D)
    # no bias: LN without the additive part
    L.check(clip_embed_ln(src, rows_f32, cls, pos, w, None, out, B, G, D))
    ref0 = F.layer_norm(rows, (D,), w.double(), None, 1e-5).view(R, D)
    assert float((out.double() - ref0).abs().max()) <= 8 * own_err


def test_clip_embed_ln_refusals():
    _, L = _ops()
    B, G, D = 2, 3, 64
    p16, p32 = torch.zeros(B * G, D, device=DEV, dtype=bf16), torch.zeros(B * G, D, device=DEV)
    cls, pos, w, b = torch.zeros(D, device=DEV), torch.zeros(G + 1, D, device=DEV), torch.ones(D, device=DEV), torch.zeros(D, device=DEV)
    out = torch.full((B * (G + 1), D), SENT, device=DEV)

    def refused(match, patches=p16, f32_rows=False, cls=cls, pos=pos, w=w, b=b, out=out, B=B, G=G, D=D, **kw):
        assert clip_embed_ln(patches, f32_rows, cls, pos, w, b, out, B, G, D, **kw) == -1
        assert match in L.lib.fm_last_error().decode(), L.lib.fm_last_error().decode()

    assert clip_embed_ln(p16, False, cls, pos, w, b, out, B, G, D) == 0 and clip_embed_ln(p32, True, cls, pos, w, None, out, B, G, D) == 0
    out.fill_(SENT)
    torch.cuda.synchronize()
    for name in ("patches", "cls", "pos", "w", "out"):
        refused("null pointer", **{name: None})
    for kw in (dict(B=0), dict(G=0), dict(D=0)):
        refused("must be positive", **kw)
    refused("multiple of 4", D=62)
    refused("multiple of 4", D=2052, ldp=2052, ldo=2052)
    refused("ldp=", ldp=60)
    refused("ldp=", ldo=60)
    refused("ldp=", ldp=66)
    refused("ldp=", ldo=66)
    refused("16-byte aligned", patches=p32.view(-1)[1:1 + (B * G - 1) * D].view(B * G - 1, D), f32_rows=True, B=1)
    refused("16-byte aligned", w=torch.ones(D + 1, device=DEV)[1:])
    refused("16-byte aligned", out=torch.zeros(B * (G + 1) * D + 1, device=DEV)[1:].view(B * (G + 1), D))
    refused("exceed the grid", B=2 ** 30, G=3)
    torch.cuda.synchronize()
    assert bool((out == SENT).all())                                             # nothing was launched by a refused call
