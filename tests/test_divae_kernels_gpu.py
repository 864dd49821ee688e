"""Per-kernel numerics of the diffusion detokenizer (DiVAE decoder) on a real MI355X: the nine entry points of csrc/unet.hip
(fm_unet_im2col, fm_groupnorm_nhwc, fm_unet_attention, fm_add_bf16, fm_silu_f32_to_bf16, fm_timestep_embedding, fm_diffusion_x0,
fm_quantile_abs, fm_diffusion_step) and the implicit-convolution path of fm_gemm_nt (conv=), each against a float64 (or exact)
restatement of the upstream operation it replaces, on the same bf16 / fp32 inputs.  tests/test_divae.py bounds the largest element
of a few shapes and whole decodes at the 1e-2 level; here every element is held to a bound derived from u = 2^-24 (fp32 unit
roundoff), the half-ulp of a bf16 store (hulp: 2^(e - 8) in the binade 2^e, i.e. 2^-9 ... 2^-8 of |want|), the length of the kernel's
summation chains and the documented accuracy of __expf / rsqrtf / expf / logf / cosf / sinf (1 ulp = 2 u each; v_exp_f32 behind __expf:
1 ulp after the argument's own roundings), written next to its check.  Pad columns of every output start as a sentinel and must stay so; pad columns the kernel must not read
hold NaN.

Not run: a launch large enough for grid_for (csrc/unet.hip) to clamp the grid.  The clamp sits at 65535 * 16 workgroups of 256
threads; the smallest such launch (fm_unet_im2col: 16 bytes per thread) writes 4.3 GB, beyond the 1 GB a test here may hold."""
import math
import os

import pytest
import torch
import torch.nn.functional as F

from tests.parity_log import record

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -24           # fp32 unit roundoff (half an ulp)
ETA = 2.0 ** -126        # smallest normal fp32 / bf16: results below it may be flushed to zero
SENT = 7.0


def _ops():
    from fourm.hip import ops, _lib
    return ops, _lib


def gen(seed):
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    return g


def randn(*shape, scale=1.0, mean=0.0, seed=0):
    return (torch.randn(*shape, generator=gen(seed)) * scale + mean).to(DEV)


def f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


def check(name, got, ref, tol):
    """|got - ref| <= tol element-wise (float64); returns the worst err / tol."""
    err = (got.double() - ref).abs()
    tol = torch.as_tensor(tol, dtype=torch.float64, device=err.device).expand_as(err)
    bad = ~(err <= tol)
    ratio = float((err / (tol + 1e-300)).max()) if err.numel() else 0.0
    assert not bool(bad.any()), f"{name}: {int(bad.sum())} of {err.numel()} outside the bound, worst err/tol {ratio:.3g}"
    return ratio


def padded(src, ld, fill=float("nan")):
    """src (rows, cols) copied into a (rows, ld) buffer; returns the (rows, cols) view (row stride ld)."""
    buf = torch.full((src.shape[0], ld), fill, device=DEV, dtype=src.dtype)
    buf[:, :src.shape[1]] = src
    return buf[:, :src.shape[1]]


def sentinel_rows(rows, cols, ld, dtype=torch.bfloat16):
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


def hulp(z):
    """Half an ulp of a bf16 store of a value of magnitude z: bf16 keeps 8 significant bits, so in the binade 2^e <= z < 2^(e + 1) the
    spacing is 2^(e - 7) and a correctly rounded store errs by up to 2^(e - 8) - between 2^-9 z (top of the binade) and 2^-8 z (bottom).
    The exact half-ulp is used: 2^-9 z for every z would refuse correctly rounded results in the lower part of each binade."""
    z = torch.as_tensor(z, dtype=torch.float64)
    two_k = ((torch.frexp(z)[1].long() - 9 + 1023).clamp(min=1) << 52).view(torch.float64)          # 2^(e - 8) built from its bits: exact
    return torch.where(z > 0, two_k, torch.zeros_like(z))


def bf16_rne(x64):
    """float64 -> the nearest bf16 value (8 significant bits, ties to even), as float64, on the bit pattern: the 45 low bits of the
    52-bit fraction go, round half to even; normal range only."""
    b = x64.contiguous().view(torch.int64)
    b = (b + ((1 << 44) - 1) + ((b >> 45) & 1)) & ~((1 << 45) - 1)
    return b.view(torch.float64)


def ru(v, m):
    return (v + m - 1) // m * m


# ------------------------------------------------------------------------------------------------
# fm_unet_im2col
# ------------------------------------------------------------------------------------------------
def im2col_ref(s1, s2, B, H, W, H2, W2, ksize, stride, up1):
    """float32 restatement on the bf16 values (every step a copy, so exact): src1 (B, H >> up1, W >> up1, C1) repeated x2 when up1,
    src2 (B, H2, W2, C2) through F.interpolate(mode="nearest") to (H, W) (unet.py:732), concatenated along channels, zero border,
    tap (ky, kx) of output pixel (oy, ox) = in[oy stride + ky - pad][ox stride + kx - pad]; columns tap * C + c."""
    C1 = s1.shape[1]
    a = s1.float().view(B, H >> up1, W >> up1, C1)
    if up1:
        a = a.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    if s2 is not None:
        b = s2.float().cpu().view(B, H2, W2, -1).permute(0, 3, 1, 2)
        b = F.interpolate(b, (H, W), mode="nearest").permute(0, 2, 3, 1).to(a.device)
        a = torch.cat([a, b], dim=3)
    pad = ksize // 2
    Ho, Wo = (H + 2 * pad - ksize) // stride + 1, (W + 2 * pad - ksize) // stride + 1
    ap = F.pad(a, (0, 0, pad, pad, pad, pad))
    taps = [ap[:, ky:ky + stride * (Ho - 1) + 1:stride, kx:kx + stride * (Wo - 1) + 1:stride, :] for ky in range(ksize) for kx in range(ksize)]
    return torch.cat(taps, dim=3).reshape(B * Ho * Wo, -1), Ho, Wo


IM2COL_CASES = [  # B, H, W, C1, C2, H2, W2, ksize, stride, up1
    (2, 9, 11, 8, 0, 0, 0, 3, 1, 0), (2, 9, 11, 48, 0, 0, 0, 3, 2, 0), (3, 14, 14, 64, 0, 0, 0, 3, 1, 0), (3, 14, 14, 8, 0, 0, 0, 3, 2, 0),
    (2, 7, 7, 256, 0, 0, 0, 3, 1, 0), (2, 7, 7, 48, 0, 0, 0, 3, 2, 0), (5, 1, 1, 64, 0, 0, 0, 3, 1, 0), (5, 1, 1, 8, 0, 0, 0, 3, 2, 0),
    (2, 9, 11, 64, 0, 0, 0, 1, 1, 0),                                              # the zero-padded copy for C % 64 != 0
    (2, 14, 10, 48, 0, 0, 0, 3, 1, 1), (1, 8, 6, 64, 0, 0, 0, 3, 2, 1),           # nearest x2 in front
    (2, 9, 11, 64, 48, 9, 11, 1, 1, 0), (2, 7, 7, 256, 256, 7, 7, 1, 1, 0),       # skip concatenation
    (2, 9, 11, 8, 64, 9, 11, 3, 1, 0), (2, 14, 14, 48, 8, 14, 14, 3, 2, 0),
    (2, 56, 56, 48, 8, 14, 14, 3, 1, 0), (8, 56, 56, 64, 32, 14, 14, 3, 1, 0),    # the decoder's first convolution: patch rows | conditioning
    (2, 8, 6, 8, 48, 4, 2, 3, 1, 0), (1, 46, 46, 8, 8, 14, 28, 3, 1, 0), (1, 46, 46, 8, 8, 14, 28, 1, 1, 0),
    (2, 8, 6, 8, 8, 4, 3, 3, 1, 1),                                               # up1 together with a second source
]


@pytest.mark.parametrize("B,H,W,C1,C2,H2,W2,ksize,stride,up1", IM2COL_CASES)
def test_im2col_bitwise(B, H, W, C1, C2, H2, W2, ksize, stride, up1):
    """fm_unet_im2col == the index-by-index gather bit for bit (pure copies).  ld1 > C1 and ld2 > C2 with NaN in the pad columns, kpad = the
    next multiple of 64 (columns [ksize^2 C, kpad) exactly 0), ldo > kpad (columns >= kpad and the row past the end keep the sentinel).
    The second source follows F.interpolate(mode="nearest"), which for (14, 28) under (46, 46) is not y * H2 / H."""
    ops, L = _ops()
    seed = B + 3 * H + 5 * W + C1 + 7 * C2 + ksize + stride + up1
    s1 = padded(randn(B * (H >> up1) * (W >> up1), C1, seed=seed).bfloat16(), C1 + 8)
    s2 = padded(randn(B * H2 * W2, C2, seed=seed + 1).bfloat16(), C2 + 16) if C2 else None
    ref, Ho, Wo = im2col_ref(s1, s2, B, H, W, H2, W2, ksize, stride, up1)
    kk = ksize * ksize * (C1 + C2)
    kpad, R = ru(kk, 64), B * Ho * Wo
    buf, out = sentinel_rows(R, kpad, kpad + 8)
    L.check(L.unet_im2col(ops._p(s1), s1.stride(0), C1, ops._p(s2), s2.stride(0) if C2 else 0, C2, H2, W2, ops._p(buf), buf.stride(0), kpad,
                          B, H, W, ksize, stride, up1, ops._stream()))
    assert torch.equal(out[:, :kk].contiguous().view(torch.int16), ref.bfloat16().view(torch.int16))
    assert bool((out[:, kk:] == 0).all())
    assert untouched(buf, R, kpad)


def test_im2col_second_source_is_f_interpolate_for_every_ratio():
    """Every pair of grids n_out, n_in <= 64, on the kernel: channel 0 of the second source holds its row, channel 1 its column (integers
    below 64 are exact in bf16); a ksize = 1 launch over an (n_out, 65 - n_out) grid must reproduce F.interpolate(mode="nearest")
    (unet.py:732) of the (n_in, 65 - n_in) source - rows and columns run through the ratios in opposite order, so both axes see every one.
    (tests/test_divae.py holds the same index formula, in Python, to F.interpolate on the CPU.)"""
    ops, L = _ops()
    bad = []
    for n_in in range(1, 65):
        w_in = 65 - n_in
        yy, xx = torch.meshgrid(torch.arange(n_in, dtype=torch.float32), torch.arange(w_in, dtype=torch.float32), indexing="ij")
        src = torch.zeros(n_in, w_in, 8)
        src[..., 0], src[..., 1] = yy, xx
        s2 = src.reshape(-1, 8).bfloat16().to(DEV)
        for n_out in range(1, 65):
            w_out = 65 - n_out
            s1 = torch.zeros(n_out * w_out, 8, dtype=torch.bfloat16, device=DEV)
            out = torch.full((n_out * w_out, 64), SENT, dtype=torch.bfloat16, device=DEV)
            L.check(L.unet_im2col(ops._p(s1), 8, 8, ops._p(s2), 8, 8, n_in, w_in, ops._p(out), 64, 64, 1, n_out, w_out, 1, 1, 0, ops._stream()))
            want = F.interpolate(src.permute(2, 0, 1)[None], (n_out, w_out), mode="nearest")[0].permute(1, 2, 0).reshape(-1, 8)
            if not torch.equal(out[:, 8:16].float().cpu(), want):
                bad.append((n_out, w_out, n_in, w_in))
    assert not bad, (len(bad), bad[:10])


def test_im2col_refusals():
    ops, L = _ops()
    s = torch.zeros(64, 64, dtype=torch.bfloat16, device=DEV)
    out = torch.zeros(64, 1024, dtype=torch.bfloat16, device=DEV)

    def call(C1=8, kpad=576, H=4, W=4, ksize=3, up1=0, ldo=1024):
        return L.unet_im2col(ops._p(s), 64, C1, None, 0, 0, 0, 0, ops._p(out), ldo, kpad, 1, H, W, ksize, 1, up1, ops._stream())
    refused(call(C1=12), "multiples of 8")
    refused(call(C1=64, kpad=512), "too small for")
    refused(call(H=5, up1=1), "fm_unet_im2col: up1")
    refused(call(ksize=5), "ksize=5 (1 or 3)")
    assert bool((out == 0).all())


# ------------------------------------------------------------------------------------------------
# fm_groupnorm_nhwc
# ------------------------------------------------------------------------------------------------
GN_FUSED_ENV = int(os.environ.get("FOURM_GN_FUSED", "1"))
GN_EPS = f32(1e-5)


def gn_is_fused(B, C, G, ld_add):
    """The launcher's choice (csrc/unet.hip fm_groupnorm_nhwc): one workgroup per (sample, group) when there are 64 of them and a group's
    row is a whole number of 8-byte quads that divides 256."""
    cpg = C // G
    return bool(GN_FUSED_ENV and B * G >= 64 and cpg % 4 == 0 and 256 % (cpg // 4) == 0 and ld_add % 4 == 0)


def silu_tol(t, dt):
    """SiLU s = t / (1 + e^-t) evaluated in fp32 on a t that carries an error dt: |s'| <= 1.1; __expf(-t) = v_exp_f32(-t log2 e): the
    product and the constant's rounding move the exponent by 2 u |t| log2 e, i.e. 2 u |t| relative in e, v_exp_f32 adds 1 ulp (2 u), and
    e enters s through e / (1 + e) <= 1; then 1 + e (u) and the division (<= 2.5 ulp):
        |s - want| <= 1.1 dt + (2 |t| + 9) u |want| + ETA (+ |want| for t < -88).
    t < -88: e^-t leaves the fp32 range (inf from t = -88.73 on), s becomes -0 where the exact value is up to 89 * 2^-128 = 2.6e-37 -
    fp32 torch's x * sigmoid(x) does the same; ETA: a result below the normal range may be flushed."""
    s = t * torch.sigmoid(t)
    return s, 1.1 * dt + (2 * t.abs() + 9) * U * s.abs() + ETA + torch.where(t < -88.0, s.abs(), torch.zeros_like(s))


def gn_ref_tol(x, add, w, b, B, HW, C, G, eps, silu, fused):
    """float64 GroupNorm (nn.py:23-25: F.group_norm in fp32, biased variance) of v = x (bf16) + add (fp32), SiLU behind (unet.py:230-246),
    and the element-wise bound of the form the launcher runs.  n = HW cpg values per group, c = v - mean, rstd = (var + eps)^-1/2.

    Three kernels (gn_stats / gn_finalize / gn_apply): d = (x + add) - shift, two roundings: dd = u (|v| + |d|).  Longest summation chain
    L = ceil(min(32, HW) / row_lanes) per thread + row_lanes cpg in LDS + chunks in gn_finalize (row_lanes = 256 / (C / 4)); 1 / n and
    the product with it add 2 u:
        |d md|  <= mean dd + (L + 2) u mean |d|                                    (md = mean - shift)
        |d var| <= mean 2 |d| dd + (L + 3) u mean d^2 + 2 |md| |d md| + 2 u md^2 + u var      (var = E[d^2] - md^2: the md^2 terms are what a
                                                                                               shift far from the mean costs)
        |d c|   <= u (|v| + |d| + |c|) + |d md|                                   (gn_apply: ((x + add) - shift) - md)
    One workgroup per group (gn_fused_kernel): chain Lm = ceil(HW / rows_per_it) + 10 for the mean (quad tree 2, 64-lane tree 6, 4 waves 2),
    Lq = 4 ceil(HW / rows_per_it) + 8 for the squares; d = (x + add) - mean':
        |d mean| <= (Lm + 2) u mean |v|;   |d c| <= u (|v| + |c|) + |d mean|;   |d var| <= 2 max|d c| mean |c| + max|d c|^2 + (Lq + 3) u var
    Both: rstd lies between (var + eps +- d var)^-1/2 (the lower argument clamped at eps: fmaxf(var, 0)), rsqrtf and the sum add 4 u:
        |t - want| <= |w| rstd |d c| + |w| |c| |d rstd| + 4 u |c rstd w| + u |want|,
    then SiLU (silu_tol) and the bf16 store hulp(|want| + E) + E.  For N(0.7, 1.5) maps the store's term dominates (E is ~ 1e-5 |want|);
    E matters for large means, near-constant groups (rstd ~ eps^-1/2 amplifies d c) and the outlier shift."""
    cpg = C // G
    v = x.double().view(B, HW, C) + (add.double()[:, None, :] if add is not None else 0.0)
    vg = v.view(B, HW, G, cpg)
    gmean = lambda z: z.mean(dim=(1, 3), keepdim=True)
    gmax = lambda z: z.amax(dim=(1, 3), keepdim=True)
    mean = gmean(vg)
    c = vg - mean
    var = gmean(c * c)
    rstd = (var + eps).rsqrt()
    w64, b64 = w.double().view(1, 1, G, cpg), b.double().view(1, 1, G, cpg)
    want = c * rstd * w64 + b64
    if fused:
        it = -(-HW // (256 // (cpg // 4)))
        Lm, Lq = it + 10, 4 * it + 8
        dc = U * (vg.abs() + c.abs()) + (Lm + 2) * U * gmean(vg.abs())
        dvar = 2 * gmax(dc) * gmean(c.abs()) + gmax(dc) ** 2 + (Lq + 3) * U * var
    else:
        row_lanes = 256 // (C // 4)
        Lc = -(-min(32, HW) // row_lanes) + row_lanes * cpg + -(-HW // 32)
        shift = vg[:, :1, :, :1]
        d = vg - shift
        md = mean - shift
        dd = U * (vg.abs() + d.abs())
        dmd = gmean(dd) + (Lc + 2) * U * gmean(d.abs())
        dvar = gmean(2 * d.abs() * dd) + (Lc + 3) * U * gmean(d * d) + 2 * md.abs() * dmd + 2 * U * md * md + U * var
        dc = dd + U * c.abs() + dmd
        del d, dd
    r_hi = (torch.clamp(var - dvar, min=0.0) + eps).rsqrt()
    r_lo = (var + dvar + eps).rsqrt()
    drstd = torch.maximum(r_hi - rstd, rstd - r_lo) + 4 * U * rstd
    E = w64.abs() * rstd * dc + w64.abs() * c.abs() * drstd + 4 * U * (c * rstd * w64).abs() + U * want.abs()
    del dc, c, vg, v
    if silu:
        want, E = silu_tol(want, E)
    tol = hulp(want.abs() + E) + E
    return want.reshape(B * HW, C), tol.reshape(B * HW, C)


def gn_run(x, add, w, b, B, HW, C, G, silu, ldx, ldy, ld_add):
    ops, L = _ops()
    xb = padded(x, ldx)
    ab = padded(add, ld_add) if add is not None else None
    buf, y = sentinel_rows(B * HW, C, ldy)
    st = torch.full((B * G * ((HW + 31) // 32 + 1) * 2 + 8,), float("nan"), device=DEV)
    args = (ops._p(xb), ldx, ops._p(ab), ld_add if add is not None else 0, ops._p(w), ops._p(b), ops._p(buf), ldy, ops._p(st), B, HW, C, G, GN_EPS,
            1 if silu else 0, ops._stream())
    L.check(L.groupnorm_nhwc(*args))
    first = y.clone()
    assert untouched(buf, B * HW, C)
    L.check(L.groupnorm_nhwc(*args))
    assert torch.equal(first.view(torch.int16), y.contiguous().view(torch.int16)), "two runs differ"          # the determinism csrc/unet.hip promises
    return first


def gn_affine(C, seed):
    """weights in [0.5, 1.5), small biases; channel 1 lands near t = -20 (|SiLU| ~ 4e-8), channel 2 near t = 0."""
    w = torch.rand(C, generator=gen(seed)) + 0.5
    b = torch.randn(C, generator=gen(seed + 1)) * 0.2
    if C >= 4:
        w[1], b[1], w[2], b[2] = 0.01, -20.0, 1e-3, 0.0
    return w.to(DEV), b.to(DEV)


GN_SHAPES = [  # B, HW, C, G        production maps at batch 1 (three kernels) and 8 (one workgroup per group), then the edges
    (1, 3136, 256, 32), (8, 3136, 256, 32), (1, 784, 512, 32), (8, 784, 512, 32), (1, 196, 768, 32), (8, 196, 768, 32), (1, 49, 1024, 32), (8, 49, 1024, 32),
    (8, 784, 768, 32), (1, 196, 1024, 32),
    (3, 1, 256, 32), (2, 31, 512, 32), (8, 33, 256, 32), (3, 50, 512, 32),
    (2, 50, 96, 8), (9, 33, 96, 8),          # C / 4 = 24 does not divide 256 (idle threads in gn_stats_kernel); cpg = 12: falls back from the fused form
    (2, 31, 256, 1), (70, 33, 32, 1), (8, 50, 64, 8), (2, 33, 4, 1), (64, 31, 4, 1),
]


@pytest.mark.parametrize("B,HW,C,G", GN_SHAPES)
def test_groupnorm_shapes(B, HW, C, G):
    """Inputs N(0.7, 1.5) with an N(0, 1) addend, SiLU on and off, ldx / ldy / ld_add wider than C (NaN / sentinel pads)."""
    x = randn(B * HW, C, scale=1.5, mean=0.7, seed=B + HW + C).bfloat16()
    add = randn(B, C, seed=B + HW + C + 1)
    w, b = gn_affine(C, HW + C)
    worst = 0.0
    for silu, a, ld_add in ((True, add, C + 4), (False, None, 0), (False, add, C + 4)):
        y = gn_run(x, a, w, b, B, HW, C, G, silu, C + 8, C + 12, ld_add)
        want, tol = gn_ref_tol(x, a, w, b, B, HW, C, G, GN_EPS, silu, gn_is_fused(B, C, G, ld_add))
        worst = max(worst, check(f"groupnorm {(B, HW, C, G)} silu={silu} add={a is not None}", y, want, tol))
        del want, tol
    record("divae_kernels.groupnorm_nhwc", B=B, HW=HW, C=C, G=G, fused=gn_is_fused(B, C, G, C + 4), worst_err_over_tol=worst)


@pytest.mark.parametrize("B,HW,C,G", [(1, 196, 256, 32), (8, 196, 256, 32), (2, 50, 96, 8), (1, 3136, 256, 32), (8, 784, 512, 32)])
@pytest.mark.parametrize("kind", ["mean100", "mean-300", "constant_group", "first_value_outlier", "addend50"])
def test_groupnorm_hard_inputs(B, HW, C, G, kind):
    """(b) maps of mean 100 / -300 and deviation 1 (bf16 spacing 0.5 / 2 there; the reference sees the same bf16 values): what the shift of
    the three-kernel form and the centred second sweep of the fused form are for; (c) one group constant: variance 0, the output is the
    bias up to |w| eps^-1/2 |d c| (upstream's F.group_norm amplifies the rounding of its own mean in the same way), finite; (d) the
    first value of a group 1e3 away from the rest - the three-kernel form's shift is then a bad centre and its variance carries
    (L + 3) u (mean - shift)^2: the bound has that term (gn_ref_tol), nothing more is promised; (e) an addend of magnitude 50 on a map of
    magnitude 1."""
    cpg = C // G
    seed = B + HW + C + len(kind)
    add = None
    if kind == "mean100":
        x = randn(B * HW, C, mean=100.0, seed=seed)
    elif kind == "mean-300":
        x = randn(B * HW, C, mean=-300.0, seed=seed)
    elif kind == "constant_group":
        x = randn(B * HW, C, seed=seed)
        x[:, cpg:2 * cpg] = 0.7
    elif kind == "first_value_outlier":
        x = randn(B * HW, C, seed=seed)
        x.view(B, HW, C)[:, 0, 0] = 1000.0
        x.view(B, HW, C)[:, 0, cpg] = -1000.0
    else:
        x = randn(B * HW, C, seed=seed)
        add = randn(B, C, scale=50.0, seed=seed + 1)
    x = x.bfloat16()
    w, b = gn_affine(C, seed + 2)
    worst = 0.0
    for silu in (True, False):
        y = gn_run(x, add, w, b, B, HW, C, G, silu, C + 8, C, C if add is not None else 0)
        assert bool(torch.isfinite(y.float()).all())
        want, tol = gn_ref_tol(x, add, w, b, B, HW, C, G, GN_EPS, silu, gn_is_fused(B, C, G, C))
        worst = max(worst, check(f"groupnorm {kind} {(B, HW, C, G)} silu={silu}", y, want, tol))
        del want, tol
    record("divae_kernels.groupnorm_nhwc_hard", kind=kind, B=B, HW=HW, C=C, G=G, worst_err_over_tol=worst)


def test_groupnorm_refusals():
    ops, L = _ops()
    x = torch.zeros(8, 2048, dtype=torch.bfloat16, device=DEV)
    w = torch.zeros(2048, device=DEV)
    st = torch.zeros(4096, device=DEV)

    def call(C=64, G=32, ldx=2048):
        return L.groupnorm_nhwc(ops._p(x), ldx, None, 0, ops._p(w), ops._p(w), ops._p(x), ldx, ops._p(st), 1, 4, C, G, 1e-5, 0, ops._stream())
    refused(call(C=60, G=32), "C % groups == 0")
    refused(call(C=6, G=1), "C % 4 == 0")
    refused(call(C=2048, G=32), "C <= 1024")
    refused(call(ldx=2046), "C % groups == 0")


# ------------------------------------------------------------------------------------------------
# fm_unet_attention
# ------------------------------------------------------------------------------------------------
def attn_ref_tol(qkv, B, T, heads, ch):
    """float64 QKVAttentionLegacy (unet.py:345-374): per head [q | k | v], weight = softmax((q s)(k s)^T), s = ch^-1/4, out = weight v.
    Kernel (unet_attn_kernel): q / sqrt(ch) (sqrtf, division, product: 3 u), a ch-term FMA chain per score:
        |d score| <= (ch + 3) u sum_d |q_d k_d| / sqrt(ch) =: ds;  a softmax weight moves by 2 ds relative (numerator and denominator).
    e = __expf(score - max): the subtraction u |score - max| + the argument's 2 u |.| + 1 ulp -> (3 D + 3) u relative, D = max - score;
    below e^-87 the weight flushes to 0 (an absolute 2^-126 per key).  Denominator: ceil(T / 256) + 6 + 3 additions of positive terms.
    Output: a T-term FMA chain on p v, reciprocal and product (4 u).  With A = sum_s weight_s |v_s|:
        |o - want| <= (2 ds_max + (ceil(T / 256) + T + 13) u) A + u sum_s weight_s (3 D_s + 3) (|v_s| + A) + T 2^-126 max|v|,
    then the bf16 store hulp(|want| + E) + E (the store's term dominates: E is ~ (T + ch) u A)."""
    x = qkv.double().view(B, T, heads, 3, ch)
    q, k, v = x[:, :, :, 0], x[:, :, :, 1], x[:, :, :, 2]
    sc = torch.einsum("bthc,bshc->bhts", q, k) / math.sqrt(ch)
    ds = (ch + 3) * U * torch.einsum("bthc,bshc->bhts", q.abs(), k.abs()) / math.sqrt(ch)
    wgt = torch.softmax(sc, dim=-1)
    want = torch.einsum("bhts,bshc->bthc", wgt, v)
    A = torch.einsum("bhts,bshc->bthc", wgt, v.abs())
    D = sc.amax(dim=-1, keepdim=True) - sc
    we = wgt * (3 * torch.clamp(D, max=88.0) + 3)
    e_exp = U * (torch.einsum("bhts,bshc->bthc", we, v.abs()) + we.sum(-1).permute(0, 2, 1)[..., None] * A)
    dsm = ds.amax(dim=-1).permute(0, 2, 1)[..., None]
    E = (2.1 * dsm + (-(-T // 256) + T + 13) * U) * A + e_exp + T * ETA * float(v.abs().max())
    tol = hulp(want.abs() + E) + E
    return want.reshape(B * T, heads * ch), tol.reshape(B * T, heads * ch)


ATTN_SHAPES = [(8, 196, 1, 512), (8, 49, 1, 512), (3, 1, 2, 64), (2, 63, 4, 8), (2, 65, 2, 64), (2, 257, 1, 520), (2, 784, 2, 64), (1, 257, 4, 8)]


@pytest.mark.parametrize("B,T,heads,ch", ATTN_SHAPES)
def test_unet_attention_elementwise(B, T, heads, ch):
    """N(0, 1) rows; ld > heads 3 ch (NaN pad) and ldo > heads ch (what unet.py:277-280 passes when C % 64 != 0), sentinels."""
    ops, L = _ops()
    W = heads * 3 * ch
    qkv = padded(randn(B * T, W, seed=T + ch + heads).bfloat16(), W + 8)
    buf, out = sentinel_rows(B * T, heads * ch, ru(heads * ch, 64) + 8)
    L.check(L.unet_attention(ops._p(qkv), qkv.stride(0), ops._p(buf), buf.stride(0), B, T, heads, ch, ops._stream()))
    want, tol = attn_ref_tol(qkv, B, T, heads, ch)
    r = check(f"attention {(B, T, heads, ch)}", out, want, tol)
    assert untouched(buf, B * T, heads * ch)
    record("divae_kernels.unet_attention", B=B, T=T, heads=heads, ch=ch, worst_err_over_tol=r)


@pytest.mark.parametrize("kind", ["dominant_key", "equal_scores"])
def test_unet_attention_extreme_scores(kind):
    """One key ahead of every other score by more than 90 (__expf underflows to 0 for the rest: the output is that key's value row), and
    all-equal scores (identical keys: the output is the mean of the values)."""
    ops, L = _ops()
    B, T, heads, ch = 2, 65, 2, 64
    x = randn(B, T, heads, 3, ch, seed=7 if kind == "dominant_key" else 8)
    if kind == "dominant_key":
        x[:, :, :, 0] = 6.0 + 0.25 * x[:, :, :, 0]                          # q . k_5 / 8 ~ 288, the others ~ N(0, 36)
        x[:, 5, :, 1] = 6.0
    else:
        x[:, :, :, 1] = x[:, :1, :, 1]
    qkv = x.reshape(B * T, heads * 3 * ch).bfloat16()
    buf, out = sentinel_rows(B * T, heads * ch, heads * ch + 8)
    L.check(L.unet_attention(ops._p(qkv), qkv.stride(0), ops._p(buf), buf.stride(0), B, T, heads, ch, ops._stream()))
    want, tol = attn_ref_tol(qkv, B, T, heads, ch)
    if kind == "dominant_key":
        x64 = qkv.double().view(B, T, heads, 3, ch)
        top = (torch.einsum("bthc,bshc->bhts", x64[:, :, :, 0], x64[:, :, :, 1]) / 8.0).topk(2, dim=-1).values
        assert float((top[..., 0] - top[..., 1]).min()) > 90.0
    r = check(f"attention {kind}", out, want, tol)
    assert untouched(buf, B * T, heads * ch)
    record("divae_kernels.unet_attention_extreme", kind=kind, worst_err_over_tol=r)


def test_unet_attention_lds_boundary_and_refusals():
    """q[ch] | p[T] in LDS: (ch + T) 4 bytes <= 60 KB.  ch + T = 15360 runs (and is checked), 15368 is refused."""
    ops, L = _ops()
    B, T, heads, ch = 1, 8, 1, 15352
    qkv = randn(B * T, 3 * ch, scale=0.5, seed=9).bfloat16()
    buf, out = sentinel_rows(B * T, ch, ch + 8)
    L.check(L.unet_attention(ops._p(qkv), qkv.stride(0), ops._p(buf), buf.stride(0), B, T, heads, ch, ops._stream()))
    want, tol = attn_ref_tol(qkv, B, T, heads, ch)
    check("attention ch + T = 15360", out, want, tol)
    assert untouched(buf, B * T, ch)
    big = torch.zeros(8, 3 * 15360, dtype=torch.bfloat16, device=DEV)
    o = torch.zeros(8, 15360, dtype=torch.bfloat16, device=DEV)
    refused(L.unet_attention(ops._p(big), 3 * 15360, ops._p(o), 15360, 1, 8, 1, 15360, ops._stream()), "ch + T = 15368 too large")
    refused(L.unet_attention(ops._p(big), 36, ops._p(o), 16, 1, 8, 1, 12, ops._stream()), "ch % 8 == 0")
    assert bool((o == 0).all())


# ------------------------------------------------------------------------------------------------
# fm_add_bf16, fm_silu_f32_to_bf16
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,C", [(1, 4), (37, 100), (3001, 256), (6272, 768)])
def test_add_bf16_bitwise(rows, C):
    """out = bf16(a + b) (unet.py: skip_connection(x) + h, x + attention), bit for bit the float64 sum rounded once to the nearest-even
    bf16.  The fp32 sum of two bf16 values (8 significant bits) is exact when their exponents differ by at most 16; beyond that it rounds
    once, to within 2^-24 of the larger operand - a bf16 value, whose nearest rounding boundaries lie at least 2^-10 of it away - so the
    store's second rounding returns the larger operand, exactly what one rounding of the exact sum gives.  Magnitudes from 2^-20 to 2^20
    mixed, exact cancellation (a = -b) and +-0 included; lda / ldb / ldo wider than C, NaN / sentinel pads."""
    ops, L = _ops()
    g = gen(rows + C)
    mag = lambda: torch.randn(rows, C, generator=g) * torch.exp2(torch.randint(-20, 21, (rows, C), generator=g).float())
    a, b = mag().bfloat16(), mag().bfloat16()
    b[::3, ::2] = -a[::3, ::2]
    a[0, 0], b[0, 0] = 0.0, -0.0
    a, b = padded(a.to(DEV), C + 4), padded(b.to(DEV), C + 8)
    buf, out = sentinel_rows(rows, C, C + 12)
    L.check(L.add_bf16(ops._p(a), a.stride(0), ops._p(b), b.stride(0), ops._p(buf), buf.stride(0), rows, C, ops._stream()))
    want = bf16_rne(a.double() + b.double())
    assert torch.equal(out.double(), want), int((out.double() != want).sum())
    assert untouched(buf, rows, C)
    refused(L.add_bf16(ops._p(a), a.stride(0), ops._p(b), b.stride(0), ops._p(buf), buf.stride(0), rows, C + 2, ops._stream()), "bad argument")


@pytest.mark.parametrize("n", [1, 255, 1000, 257 * 31])
def test_silu_f32_to_bf16(n):
    """y = bf16(x sigmoid(x)) (the SiLU in front of ResBlock.emb_layers / inside time_embed, unet.py:195-201): silu_tol with dt = 0 and the
    bf16 store: |y - want| <= hulp(|want| + E) + E, E = (2 |x| + 9) u |want| + ETA (+ |want| for x < -88).  Inputs over [-100, 100], +-0, denormals (the result
    x / 2 may flush), +-88 where e^-x leaves the fp32 range; n not a multiple of 256; the elements past n keep the sentinel."""
    ops, L = _ops()
    g = gen(n)
    x = (torch.rand(n, generator=g) * 200 - 100)
    x[::5] = torch.randn((n + 4) // 5, generator=g)
    special = torch.tensor([0.0, -0.0, 1e-40, -1e-40, 88.0, -88.0, 100.0, -100.0, -20.0, 1e-3, -87.5])
    k = min(n, special.numel())
    x[:k] = special[:k]
    x = x.to(DEV)
    buf = torch.full((n + 9,), SENT, dtype=torch.bfloat16, device=DEV)
    L.check(L.silu_f32_to_bf16(ops._p(x), ops._p(buf), n, ops._stream()))
    want, E = silu_tol(x.double(), 0.0)
    r = check(f"silu n={n}", buf[:n], want, hulp(want.abs() + E) + E)
    assert bool((buf[n:] == SENT).all())
    record("divae_kernels.silu_f32_to_bf16", n=n, worst_err_over_tol=r)
    refused(L.silu_f32_to_bf16(ops._p(x), ops._p(buf), 0, ops._stream()), "bad argument")


# ------------------------------------------------------------------------------------------------
# fm_timestep_embedding
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [64, 256, 320, 7])
def test_timestep_embedding(dim):
    """[cos(t f_j) | sin(t f_j)], f_j = exp(-ln(max_period) j / half) (nn.py:114-131); odd dim: a last column of zeros.  fp32 chain of the
    kernel (and of upstream): ln(max_period) (logf, 1 ulp = 2 u), the product with j and the division (u each) move the exponent e_j
    by 4 u |e_j|, i.e. f_j by 4 u ln(max_period) j / half relative; expf 1 ulp (2 u); t f_j (u); cosf / sinf 1 ulp of a value <= 1
    (2 u absolute, taken as 4 u).  A perturbed argument moves cos / sin by at most its own error:
        |out - want| <= hulp(|want|) + c_j u |t f_j| + 4 u,   c_j = 4 ln(max_period) j / half + 3      (c_j <= 40; 3 at j = 0).
    The bf16 store dominates except near the zeros of cos / sin - there a fast-math cosine (argument reduction at fp32 precision in
    revolutions: ~ 1e-4 absolute near t = 999) has to pass c_0 u 999 = 1.8e-4; the worst ratio over |want| < 2^-6 is recorded on its own.
    ldo > dim: the pad keeps the sentinel (unet.py:378-380 zeroes it itself)."""
    ops, L = _ops()
    t = torch.tensor([0.0, 1.0, 39.0, 250.0, 601.5, 999.0, 998.0, 3.0, 500.0], device=DEV)
    B, half, mp = t.numel(), dim // 2, 10000.0
    buf, out = sentinel_rows(B, dim, ru(dim, 64) + 8)
    L.check(L.timestep_embedding(ops._p(t), ops._p(buf), buf.stride(0), B, dim, mp, ops._stream()))
    j = torch.arange(half, dtype=torch.float64, device=DEV)
    f = torch.exp(-math.log(mp) * j / half)
    arg = t.double()[:, None] * f[None]
    want = torch.cat([torch.cos(arg), torch.sin(arg)], dim=1)
    cj = 4 * math.log(mp) * j / half + 3
    e_arg = (cj[None] * U * arg.abs()).repeat(1, 2)
    if dim % 2:
        zero = torch.zeros(B, 1, dtype=torch.float64, device=DEV)
        want, e_arg = torch.cat([want, zero], dim=1), torch.cat([e_arg, zero], dim=1)
        assert bool((out[:, dim - 1] == 0).all())
    tol = hulp(want.abs() + e_arg + 4 * U) + e_arg + 4 * U
    r = check(f"timestep_embedding dim={dim}", out, want, tol)
    small = want.abs() < 2.0 ** -6
    rs = float(((out.double() - want).abs() / tol)[small].max()) if bool(small.any()) else 0.0
    assert untouched(buf, B, dim)
    record("divae_kernels.timestep_embedding", dim=dim, worst_err_over_tol=r, worst_err_over_tol_near_zeros=rs, n_near_zeros=int(small.sum()))
    refused(L.timestep_embedding(ops._p(t), ops._p(buf), dim - 1, B, dim, mp, ops._stream()), "bad argument")


# ------------------------------------------------------------------------------------------------
# fm_diffusion_x0, fm_quantile_abs, fm_diffusion_step
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 3 * 32 * 32 + 5, 3 * 224 * 224])
def test_diffusion_x0(n):
    """x0 = c0 sample + c1 model_output (scheduling_ddim.py:270-283; the host picks c0, c1 per prediction type): two products and a sum, or a
    product and an FMA: |x0 - want| <= 2 u (|c0 s| + |c1 m|).  The coefficients reach the kernel as fp32: the reference uses fp32(c)."""
    ops, L = _ops()
    s, m = randn(n, seed=n), randn(n, scale=3.0, seed=n + 1)
    c0, c1 = f32(0.8312345), f32(-0.5559876)
    buf = torch.full((n + 7,), SENT, device=DEV)
    L.check(L.diffusion_x0(ops._p(s), ops._p(m), c0, c1, ops._p(buf), n, ops._stream()))
    want = c0 * s.double() + c1 * m.double()
    r = check(f"diffusion_x0 n={n}", buf[:n], want, 2 * U * ((c0 * s.double()).abs() + (c1 * m.double()).abs()))
    assert bool((buf[n:] == SENT).all())
    record("divae_kernels.diffusion_x0", n=n, worst_err_over_tol=r)
    refused(L.diffusion_x0(ops._p(s), None, c0, c1, ops._p(buf), n, ops._stream()), "bad argument")


def quantile_rank(n, q):
    """torch.quantile's rank in the input's dtype: pos = fp32(q) * fp32(n - 1); lo = floor(pos), hi = ceil(pos), frac = pos - lo."""
    pos = torch.tensor(q, dtype=torch.float32) * torch.tensor(float(n - 1), dtype=torch.float32)
    return int(torch.floor(pos)), int(torch.ceil(pos)), float(pos - torch.floor(pos))


def quantile_ref(v, q):
    """torch.quantile(|x|, q, dim=1, interpolation="linear") (scheduling_ddim.py:203-205) restated on v = the float64 sort of |x|:
    v[lo] + (v[hi] - v[lo]) frac with the fp32 rank of quantile_rank.  Returns the value and max(v[lo], v[hi])."""
    lo, hi, frac = quantile_rank(v.shape[1], q)
    return v[:, lo] + (v[:, hi] - v[:, lo]) * frac, torch.maximum(v[:, lo], v[:, hi])


def quantile_close(name, got, ref, vmax, allow_nan_for_inf=False):
    """|got - ref| <= 3 u max(v[lo], v[hi]): one fp32 subtraction (u |v[hi] - v[lo]|), one product (u), one sum (u), each at most
    max(v[lo], v[hi]).  inf and NaN (inf - inf at a rank on infinite values, as torch gives) must match as such.
    allow_nan_for_inf (for torch.quantile itself): torch.lerp switches to v[hi] - (v[hi] - v[lo]) (1 - frac) at frac >= 0.5, which is NaN for an
    infinite v[hi] above a finite v[lo], where the one-sided form the kernel (and this reference) uses gives inf - the by-design difference
    of the lerp form; on finite values the two forms agree within the same 3 u."""
    got, ref, vmax = got.double().cpu(), ref.double().cpu(), vmax.double().cpu()
    fin = torch.isfinite(ref)
    same = (got == ref) | (torch.isnan(got) & torch.isnan(ref))
    if allow_nan_for_inf:
        same = same | (torch.isnan(got) & torch.isinf(ref))
    assert bool(same[~fin].all()), (name, got[~fin], ref[~fin])
    return check(name, got[fin], ref[fin], 3 * U * vmax[fin]) if bool(fin.any()) else 0.0


def quantile_rows(n, B, seed):
    """Row 0 (and every row from 7 on): N(0, 1).  1: constant.  2: the smaller half a run of duplicates (for even n the run ends exactly at
    lo of q = 0.5, so v[lo] < v[lo + 1]; for odd n the rank of q = 0.5 lies just past it).  3: the larger half duplicates of the
    maximum (v[lo] == v[lo + 1] at the upper ranks).  4: +-0, denormals and three inf.  5: negative values larger in magnitude than
    every positive one.  6: every magnitude twice (ties at every rank)."""
    g = gen(seed)
    x = torch.randn(B, n, generator=g)
    if B > 1:
        x[1] = -0.25
    if B > 2:
        x[2, :n // 2] = 0.125
        x[2, n // 2:] = x[2, n // 2:].abs() + 0.5
    if B > 3:
        x[3, n // 2:] = -9.0
    if B > 4 and n >= 8:
        x[4, :7] = torch.tensor([0.0, -0.0, 1e-40, -3e-39, float("inf"), -float("inf"), float("inf")])
    if B > 5:
        x[5] = torch.where(x[5] < 0, x[5] * 100 - 10, x[5])
    if B > 6:
        x[6, n // 2:2 * (n // 2)] = -x[6, :n // 2]
    return x[:, torch.randperm(n, generator=g)].contiguous()


QUANTILE_N = [1, 2, 255, 3001, 3072, 150528, 196608]
QUANTILE_Q = [0.0, 0.5, 0.995, 0.999, 1.0]
# frac = pos - floor(pos) != 0, pos = fp32(q) fp32(n - 1):
#   n = 2: q = 0.5 (0.5), 0.995, 0.999;  255: 0.995 (252.73), 0.999 (253.746);  3072: 0.5 (1535.5), 0.995 (3055.645), 0.999 (3067.929);
#   150528: 0.5 (75263.5), 0.995 (149774.359375), 0.999 (150376.46875);  196608: 0.5 (98303.5), 0.995 (195623.96875), 0.999 (196410.390625).
#   Whole ranks: q = 0 and 1 always, every q at n = 1 and n = 3001, q = 0.5 at n = 255 (127).  That is 14 of these 35 pairs; QUANTILE_EXTRA adds
#   n = 4, 256, 1000, 4096 at q = 0.5, 0.995, 0.999, all fractional (1.5, 2.985, 2.997; 127.5, 253.725, 254.745; 499.5, 994.005, 998.001; 2047.5,
#   4074.525, 4090.905): 26 of the 47 pairs interpolate (test_quantile_cases_interpolate counts them).
QUANTILE_EXTRA = [(n, q) for n in (4, 256, 1000, 4096) for q in (0.5, 0.995, 0.999)]
QUANTILE_CASES = [(n, q) for n in QUANTILE_N for q in QUANTILE_Q] + QUANTILE_EXTRA


def test_quantile_cases_interpolate():
    frac = [quantile_rank(n, q)[2] for n, q in QUANTILE_CASES]
    assert sum(f != 0 for f in frac) * 2 >= len(frac), frac


@pytest.mark.parametrize("B", [1, 64])
@pytest.mark.parametrize("n", QUANTILE_N + [4, 256, 1000, 4096])
def test_quantile_abs(n, B):
    """fm_quantile_abs (four radix passes + the pass for v[lo + 1]) against quantile_ref, and quantile_ref against torch.quantile on the CPU
    (first 8 rows), both to 3 u max(v[lo], v[hi]) (quantile_close)."""
    ops, L = _ops()
    x = quantile_rows(n, B, seed=n + B)
    xc = x.to(DEV)
    v = x.abs().double().sort(dim=1).values
    worst = 0.0
    for q in [q for nn, q in QUANTILE_CASES if nn == n]:
        buf = torch.full((B + 3,), SENT, device=DEV)
        L.check(L.quantile_abs(ops._p(xc), B, n, q, ops._p(buf), ops._stream()))
        ref, vmax = quantile_ref(v, q)
        worst = max(worst, quantile_close(f"quantile n={n} q={q} B={B}", buf[:B], ref, vmax))
        assert bool((buf[B:] == SENT).all())
        quantile_close(f"torch.quantile n={n} q={q}", torch.quantile(x[:8].abs(), q, dim=1), ref[:8], vmax[:8], allow_nan_for_inf=True)
    record("divae_kernels.quantile_abs", n=n, B=B, worst_err_over_tol=worst)


def test_quantile_refusals():
    ops, L = _ops()
    x, out = torch.zeros(4, 8, device=DEV), torch.zeros(4, device=DEV)
    refused(L.quantile_abs(ops._p(x), 4, 8, 1.5, ops._p(out), ops._stream()), "bad argument")
    refused(L.quantile_abs(ops._p(x), 4, 0, 0.5, ops._p(out), ops._stream()), "bad argument")
    refused(L.quantile_abs(ops._p(x), 4, 8, -0.1, ops._p(out), ops._stream()), "bad argument")


@pytest.mark.parametrize("with_x0_out", [False, True])
@pytest.mark.parametrize("with_noise", [False, True])
@pytest.mark.parametrize("mode", ["quantile", "clip", "neither"])
@pytest.mark.parametrize("per_sample", [3 * 32 * 32 + 5, 1000])
def test_diffusion_step(per_sample, mode, with_noise, with_x0_out):
    """The element-wise half of DDIMScheduler.step (scheduling_ddim.py:284-330) with _threshold_sample's clamp (:206-211) in front:
        s_b = clamp(quantile_b, 1, sample_max_value);  v = clamp(x0, -s_b, s_b) / s_b   |   clamp(x0, -r, r)   |   x0
        out = k0 v + k1 sample + k2 model_output (+ k3 noise).
    B = 3 with quantiles 0.4 (clamped up to 1), 1.37 and 9.0 (clamped down to sample_max_value = 2.5).  v: the clamps are exact, the division
    <= 2.5 ulp: |v - want| <= 5 u |want| (0 without the quantile: bitwise).  out: T = 3 or 4 products (u each) added in a chain (T - 1 sums):
        |out - want| <= (T + 1) u sum |k_i term_i| + |k0| |d v|."""
    ops, L = _ops()
    B, n = 3, 3 * per_sample
    x0, smp, mo, nz = (randn(n, scale=sc, seed=per_sample + i) for i, sc in enumerate((1.5, 1.0, 2.0, 1.0)))
    quant = torch.tensor([0.4, 1.37, 9.0], device=DEV)
    s_max, clip = 2.5, 1.0
    k = [f32(c) for c in (0.93, -0.21, 0.0625, 0.37)]
    obuf, xbuf = torch.full((n + 5,), SENT, device=DEV), torch.full((n + 5,), SENT, device=DEV)
    L.check(L.diffusion_step(ops._p(x0), ops._p(quant) if mode == "quantile" else None, s_max, clip if mode == "clip" else 0.0, ops._p(smp), ops._p(mo),
                             ops._p(nz) if with_noise else None, k[0], k[1], k[2], k[3], ops._p(obuf), ops._p(xbuf) if with_x0_out else None, B, per_sample,
                             ops._stream()))
    v = x0.double()
    dv = torch.zeros_like(v)
    if mode == "quantile":
        s = quant.double().clamp(1.0, s_max).repeat_interleave(per_sample)
        v = torch.maximum(torch.minimum(v, s), -s) / s
        dv = 5 * U * v.abs()
    elif mode == "clip":
        v = v.clamp(-clip, clip)
    terms = [k[0] * v, k[1] * smp.double(), k[2] * mo.double()] + ([k[3] * nz.double()] if with_noise else [])
    want = sum(terms)
    tol = (len(terms) + 1) * U * sum(t.abs() for t in terms) + abs(k[0]) * dv
    r = check(f"diffusion_step {mode} noise={with_noise}", obuf[:n], want, tol)
    assert bool((obuf[n:] == SENT).all())
    if with_x0_out:
        if mode == "quantile":
            check("diffusion_step x0_out", xbuf[:n], v, dv)
            assert float(xbuf[:n].abs().max()) <= 1.0
        else:
            assert torch.equal(xbuf[:n].double(), v)
        assert bool((xbuf[n:] == SENT).all())
    else:
        assert bool((xbuf == SENT).all())
    record("divae_kernels.diffusion_step", per_sample=per_sample, mode=mode, noise=with_noise, worst_err_over_tol=r)


def test_diffusion_step_refusal():
    ops, L = _ops()
    x = torch.zeros(8, device=DEV)
    refused(L.diffusion_step(ops._p(x), None, 1.0, 0.0, None, ops._p(x), None, 1.0, 0.0, 0.0, 0.0, ops._p(x), None, 1, 8, ops._stream()), "bad argument")
    refused(L.diffusion_step(ops._p(x), None, 1.0, 0.0, ops._p(x), ops._p(x), None, 1.0, 0.0, 0.0, 0.0, ops._p(x), None, 1, 0, ops._stream()), "bad argument")


# ------------------------------------------------------------------------------------------------
# fm_gemm_nt with conv= : the implicit 3 x 3 convolution
# ------------------------------------------------------------------------------------------------
LAB_DEFAULTS = {9: int(os.environ.get("FOURM_NT_SMALL", "1")), 10: int(os.environ.get("FOURM_CONV_K32", "1"))}

CONV_SHAPES = [  # B, H, W, C, Co, stride, up, ldx, extra output columns
    (2, 14, 14, 128, 256, 1, 0, 128, 0), (8, 7, 7, 512, 512, 1, 0, 512, 0), (3, 28, 28, 256, 256, 2, 0, 256, 0), (2, 28, 28, 256, 512, 1, 1, 256, 0),
    (2, 56, 56, 256, 48, 1, 0, 256, 16), (1, 9, 11, 64, 100, 1, 0, 64, 28), (8, 56, 56, 256, 256, 1, 0, 256, 0),          # the seven of tests/test_divae.py
    (5, 1, 1, 64, 132, 1, 0, 72, 12), (3, 2, 3, 128, 4, 2, 0, 136, 8),                 # a 1 x 1 grid; 2 x 3 at stride 2 (M = 6)
    (1, 127, 1, 64, 100, 1, 0, 64, 4), (1, 3, 43, 64, 132, 1, 0, 80, 4),               # M = 127 and 129: a dead-row tail one below / above a tile
    (1, 12, 20, 128, 132, 1, 1, 128, 8), (2, 6, 10, 64, 64, 2, 1, 64, 0),              # nearest x2 on a non-square grid, B = 1
]


def conv_operands(B, hi, wi, C, Co, ldx, seed):
    """Asymmetric over (y, x, tap): the map carries a ramp per pixel (0.75 + y / hi along rows, 1 + 0.5 x / wi along columns) on top of N(0, 1)
    channels, the weights a ramp per tap (1 + tap / 4): a transposed tap or a mirrored border moves the result by tens of percent."""
    x = torch.randn(B, hi, wi, C, generator=gen(seed))
    x = x * 0.5 + (0.75 + torch.arange(hi).view(1, hi, 1, 1) / hi) * (1.0 + 0.5 * torch.arange(wi).view(1, 1, wi, 1) / wi)
    w4 = torch.randn(Co, C, 3, 3, generator=gen(seed + 1)) / (3.0 * C ** 0.5) * (1.0 + torch.arange(9).view(1, 1, 3, 3) / 4.0)
    bias = torch.randn(Co, generator=gen(seed + 2))
    return padded(x.reshape(-1, C).bfloat16().to(DEV), ldx), w4.bfloat16().to(DEV), bias.to(DEV)


@pytest.mark.parametrize("B,H,W,C,Co,stride,up,ldx,extra", CONV_SHAPES)
def test_implicit_conv_every_path(B, H, W, C, Co, stride, up, ldx, extra):
    """fm_gemm_nt(conv=) against float64 F.conv2d(padding=1) of the same bf16 operands (nearest x2 in front for up = 1: Upsample, unet.py:103-130;
    stride 2: Downsample :133-160), through every launch path of csrc/gemm.hip: fp32 output; bf16 output at K-step 32 / 64
    (fm_lab_set(10, 1 | 0)) with split-K allowed or not (fm_lab_set(9, 1 | 0)).  MFMA accumulation in fp32 over K = 9 C exact bf16 products,
    in the form of the split3 GEMM's bound: (K + 3) u S, S = sum |x| |w|; a split launch stores up to 16 fp32 slices and adds them (16 u S
    more); the bias is added in fp32 (u), rounded to bf16 first on the bf16 paths (the reference takes the same bias):
        E = (K + 3 + 16) u S + 2 u |bias|;   fp32 output: |out - want| <= E;   bf16 output: hulp(|want| + E) + E.
    E is the worst case of a K-term chain and exceeds the store's term for K >= 1152 (S / |want| ~ sqrt(K) here); what it must exclude - a
    lost K-tile, a wrong tap, a mirrored border - is of the order of |want| itself.  Every path also equals fm_unet_im2col + the plain
    GEMM on the same rows to one bf16 ulp (2 hulp) + 2 E.  ldx > C with NaN pad columns; ldo > Co: columns [Co, ldo) and the row
    past the end keep the sentinel."""
    ops, L = _ops()
    hi, wi = H >> up, W >> up
    x, w4, bias = conv_operands(B, hi, wi, C, Co, ldx, seed=H * W + C + Co + stride)
    wk = w4.permute(0, 2, 3, 1).reshape(Co, 9 * C).contiguous()           # taps outermost
    Ho, Wo = (H + 2 - 3) // stride + 1, (W + 2 - 3) // stride + 1
    M, K = B * Ho * Wo, 9 * C
    ldo = ru(Co, 4) + extra
    x64 = x.double().view(B, hi, wi, C).permute(0, 3, 1, 2)
    if up:
        x64 = F.interpolate(x64, scale_factor=2, mode="nearest")
    to_rows = lambda t: t.permute(0, 2, 3, 1).reshape(M, Co)
    acc = to_rows(F.conv2d(x64, w4.double(), None, stride=stride, padding=1))
    S = to_rows(F.conv2d(x64.abs(), w4.double().abs(), None, stride=stride, padding=1))
    col = torch.zeros(M, K, device=DEV, dtype=torch.bfloat16)
    L.check(L.unet_im2col(ops._p(x), ldx, C, None, 0, 0, 0, 0, ops._p(col), K, K, B, H, W, 3, stride, up, ops._stream()))
    worst = 0.0
    try:
        for f32_out, k32, small in [(True, 1, 1)] + [(False, k32, small) for k32 in (1, 0) for small in (1, 0)]:
            L.lib.fm_lab_set(10, k32)
            L.lib.fm_lab_set(9, small)
            odt = torch.float32 if f32_out else torch.bfloat16
            epi = L.EPI_F32 if f32_out else L.EPI_BF16
            b64 = bias.double() if f32_out else bias.bfloat16().double()
            want = acc + b64
            E = (K + 3 + 16) * U * S + 2 * U * b64.abs()
            tol = E if f32_out else hulp(want.abs() + E) + E
            buf, got = sentinel_rows(M, Co, ldo, odt)
            ops.gemm_nt(x, wk, buf, epilogue=epi, bias=bias, M=M, N=Co, K=K, conv=dict(C=C, H=H, W=W, Ho=Ho, Wo=Wo, stride=stride, up=up))
            name = f"conv {(B, H, W, C, Co, stride, up)} f32={f32_out} k32={k32} small={small}"
            worst = max(worst, check(name, got, want, tol))
            assert untouched(buf, M, Co), name
            buf2, plain = sentinel_rows(M, Co, ldo, odt)
            ops.gemm_nt(col, wk, buf2, epilogue=epi, bias=bias, M=M, N=Co, K=K)
            check(name + " vs im2col + GEMM", got, plain.double(), 2 * E if f32_out else 2 * hulp(want.abs() + E) + 2 * E)
    finally:
        for key, val in LAB_DEFAULTS.items():
            L.lib.fm_lab_set(key, val)
    record("divae_kernels.implicit_conv", B=B, H=H, W=W, C=C, Co=Co, stride=stride, up=up, worst_err_over_tol=worst)


def test_implicit_conv_refusals():
    ops, L = _ops()
    x = torch.zeros(64, 64, dtype=torch.bfloat16, device=DEV)
    w = torch.zeros(64, 576, dtype=torch.bfloat16, device=DEV)
    out = torch.zeros(64, 64, dtype=torch.bfloat16, device=DEV)

    def call(**kw):
        conv = dict(C=64, H=4, W=4, Ho=4, Wo=4, stride=1, up=0)
        conv.update(kw)
        with pytest.raises(RuntimeError) as e:
            ops.gemm_nt(x, w, out, M=16, N=64, K=576, conv=conv)
        return str(e.value)
    assert "fm_gemm_nt (conv): C=32" in call(C=32)
    assert "stride=3" in call(stride=3)
    assert "output grid does not match" in call(Ho=2, Wo=2)
    assert bool((out == 0).all())
