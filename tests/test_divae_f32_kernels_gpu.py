"""Per-kernel numerics of the fp32 compute mode of the diffusion detokenizer on a real MI355X: the six entry points of csrc/unet_f32.hip
(fm_unet_im2col_f32, fm_groupnorm_nhwc_f32, fm_unet_attention_f32, fm_add_f32, fm_silu_f32, fm_timestep_embedding_f32), each alone against
float64, on the smallest shapes that reach every branch (helpers shared with tests/test_divae_kernels_gpu.py, the bf16 kernels' file).

Bounds: the gather and the add are exact.  A kernel that rounds is held to the project's fp32 rule - its largest error against float64 at
most 8 x the largest error of torch's own fp32 evaluation of the same operation on the same input (a different summation order and the
device's expf / sqrt against the host's are what may differ between two correct fp32 evaluations).  fm_silu_f32 has a direct bound: 1 ulp for
expf and half an ulp each for the addition and the division are at most 2^-23 + 2 * 2^-24 = 2 * 2^-23 of the result."""
import pytest
import torch
import torch.nn.functional as F

import tests.test_divae_kernels_gpu as K
from tests import divae_f64_util as F64
from tests.parity_log import record

pytestmark = pytest.mark.gpu

DEV = "cuda"
FACTOR = 8.0
f32 = torch.float32


def within_rule(name, got, ref64, torch32, **case):
    err = float((got.double().cpu() - ref64).abs().max())
    own = float((torch32.double() - ref64).abs().max())
    print(f"{name} {case}: kernel vs float64 {err:.3e}, torch fp32 vs float64 {own:.3e}, ratio {err / max(own, 1e-300):.3g} (bound {FACTOR:g})")
    record("divae.fp32.kernels", kernel=name, err_vs_float64=err, torch_fp32_err_vs_float64=own, **case)
    assert err <= FACTOR * own, (name, case, err, own)


# ------------------------------------------------------------------------------------------------
# fm_unet_im2col_f32
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,C1,C2,H2,W2,ksize,stride,up1", [
    (2, 9, 11, 24, 8, 3, 4, 3, 1, 0),            # two sources, the second on a coarser grid
    (2, 7, 7, 64, 0, 0, 0, 3, 2, 0),             # stride 2 on an odd grid
    (1, 6, 10, 32, 0, 0, 0, 3, 1, 1),            # read through the nearest x2 up-sampling from 3 x 5
    (3, 5, 5, 40, 24, 5, 5, 1, 1, 0),            # the concatenation
])
def test_im2col_f32_bitwise(B, H, W, C1, C2, H2, W2, ksize, stride, up1):
    """A pure gather: bit-equal to the torch restatement.  ld1 > C1 and ld2 > C2 with NaN in the pad columns; kpad wider than the data (the
    pad columns exactly 0); ldo > kpad (columns from kpad on and the row past the end keep the sentinel)."""
    ops, L = K._ops()
    seed = B + 3 * H + 5 * W + C1 + 7 * C2 + ksize + stride + up1
    s1 = K.padded(K.randn(B * (H >> up1) * (W >> up1), C1, seed=seed), C1 + 4)
    s2 = K.padded(K.randn(B * H2 * W2, C2, seed=seed + 1), C2 + 8) if C2 else None
    ref, Ho, Wo = K.im2col_ref(s1.contiguous(), s2.contiguous() if C2 else None, B, H, W, H2, W2, ksize, stride, up1)
    Kc = ksize * ksize * (C1 + C2)
    kpad, ldo = Kc + 8, Kc + 8 + 4
    buf, out = K.sentinel_rows(B * Ho * Wo, kpad, ldo, dtype=f32)
    L.check(L.unet_im2col_f32(ops._p(s1), s1.stride(0), C1, ops._p(s2), s2.stride(0) if C2 else 0, C2, H2, W2, ops._p(out), ldo, kpad, B, H, W, ksize, stride, up1,
                              ops._stream()))
    assert torch.equal(out[:, :Kc], ref)
    assert bool((out[:, Kc:] == 0).all()) and K.untouched(buf, B * Ho * Wo, kpad)


def test_im2col_f32_nearest_rule_is_f_interpolate():
    """The second source's index rule against F.interpolate(mode="nearest") for every (n_in, n_out) up to 32, rows and columns alike."""
    ops, L = K._ops()
    N = 32
    wrong = torch.zeros((), dtype=torch.int64, device=DEV)
    for n_in in range(1, N + 1):
        src = torch.arange(n_in, dtype=f32)
        grid = torch.zeros(n_in, n_in, 4)
        grid[..., 0], grid[..., 1] = src[:, None], src[None, :]               # channel 0 = source row, channel 1 = source column
        s2 = grid.reshape(n_in * n_in, 4).to(DEV)
        for n_out in range(1, N + 1):
            idx = F.interpolate(src.view(1, 1, n_in, 1), (n_out, 1), mode="nearest").view(-1)
            s1 = torch.zeros(n_out * n_out, 4, device=DEV)
            out = torch.empty(n_out * n_out, 8, device=DEV)
            L.check(L.unet_im2col_f32(ops._p(s1), 4, 4, ops._p(s2), 4, 4, n_in, n_in, ops._p(out), 8, 8, 1, n_out, n_out, 1, 1, 0, ops._stream()))
            want = idx.to(DEV)
            got = out.view(n_out, n_out, 8)
            wrong += (got[..., 4] != want[:, None]).sum() + (got[..., 5] != want[None, :]).sum()
    assert int(wrong) == 0


# ------------------------------------------------------------------------------------------------
# fm_groupnorm_nhwc_f32
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,HW,C,G,with_add,silu", [(1, 50, 64, 32, False, False), (3, 49, 96, 32, False, False), (2, 1024, 128, 32, True, True),
                                                    (2, 16, 1024, 32, False, False)])
def test_groupnorm_f32(B, HW, C, G, with_add, silu):
    ops, L = K._ops()
    seed = B * 1000 + HW + C
    x = K.padded(K.randn(B * HW, C, scale=1.5, mean=0.7, seed=seed), C + 4)
    add = K.padded(K.randn(B, C, seed=seed + 1), C + 12) if with_add else None
    w, b = torch.rand(C, generator=K.gen(seed + 2)).to(DEV) + 0.5, K.randn(C, scale=0.2, seed=seed + 3)
    buf, y = K.sentinel_rows(B * HW, C, C + 8, dtype=f32)

    def launch():
        L.check(L.groupnorm_nhwc_f32(ops._p(x), x.stride(0), ops._p(add), add.stride(0) if with_add else 0, ops._p(w), ops._p(b), ops._p(y), y.stride(0), B, HW, C, G,
                                     1e-5, 1 if silu else 0, ops._stream()))
        return y.clone()

    def ref(dt):
        xin = x.contiguous().cpu().to(dt).view(B, HW, C) + (add.contiguous().cpu().to(dt)[:, None, :] if with_add else 0.0)
        r = F.group_norm(xin.permute(0, 2, 1), G, w.cpu().to(dt), b.cpu().to(dt), 1e-5).permute(0, 2, 1)
        return (F.silu(r) if silu else r).reshape(B * HW, C)

    got = launch()
    within_rule("fm_groupnorm_nhwc_f32", got, ref(torch.float64), ref(f32), B=B, HW=HW, C=C, add=with_add, silu=silu)
    assert K.untouched(buf, B * HW, C)
    assert torch.equal(launch(), got)                                     # fixed summation order


# ------------------------------------------------------------------------------------------------
# fm_unet_attention_f32
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T,heads,ch", [(2, 30, 2, 64), (1, 200, 1, 40), (2, 1, 1, 8)])
def test_unet_attention_f32(B, T, heads, ch):
    ops, L = K._ops()
    qkv = K.padded(K.randn(B * T, heads * 3 * ch, seed=T + ch), heads * 3 * ch + 4)
    buf, out = K.sentinel_rows(B * T, heads * ch, heads * ch + 4, dtype=f32)
    L.check(L.unet_attention_f32(ops._p(qkv), qkv.stride(0), ops._p(out), out.stride(0), B, T, heads, ch, ops._stream()))

    def ref(dt):                                                          # QKVAttentionLegacy (unet.py:355-370) on rows
        v = qkv.contiguous().cpu().to(dt).view(B, T, heads, 3, ch)
        q, k, vv = v[:, :, :, 0], v[:, :, :, 1], v[:, :, :, 2]
        s = 1.0 / (ch ** 0.5) ** 0.5
        wgt = torch.softmax(torch.einsum("bthc,bshc->bhts", q * s, k * s), dim=-1)
        return torch.einsum("bhts,bshc->bthc", wgt, vv).reshape(B * T, heads * ch)

    within_rule("fm_unet_attention_f32", out, ref(torch.float64), ref(f32), B=B, T=T, heads=heads, ch=ch)
    assert K.untouched(buf, B * T, heads * ch)


# ------------------------------------------------------------------------------------------------
# fm_add_f32 / fm_silu_f32 / fm_timestep_embedding_f32
# ------------------------------------------------------------------------------------------------
def test_add_f32_exact_on_strided_rows():
    ops, L = K._ops()
    rows, C = 37, 50                                                      # 1850 values: no multiple of the workgroup size
    a, b = K.padded(K.randn(rows, C, seed=1), C + 3), K.padded(K.randn(rows, C, scale=30.0, seed=2), C + 5)
    buf, out = K.sentinel_rows(rows, C, C + 2, dtype=f32)
    L.check(L.add_f32(ops._p(a), a.stride(0), ops._p(b), b.stride(0), ops._p(out), out.stride(0), rows, C, ops._stream()))
    assert torch.equal(out, a + b) and K.untouched(buf, rows, C)


def test_silu_f32():
    ops, L = K._ops()
    n = 5003
    x = K.randn(n, scale=4.0, seed=9)
    x[:8] = torch.tensor([0.0, -0.0, 88.0, -88.0, -100.0, 100.0, 1e-30, -20.0], device=DEV)
    buf = torch.full((n + 5,), K.SENT, device=DEV)
    L.check(L.silu_f32(ops._p(x), ops._p(buf), n, ops._stream()))
    x64 = x.double().cpu()
    ref = x64 * torch.sigmoid(x64)
    K.check("fm_silu_f32", buf[:n].cpu(), ref, 2 * 2.0 ** -23 * ref.abs() + K.ETA)
    assert bool((buf[n:] == K.SENT).all())


@pytest.mark.parametrize("dim", [64, 33])
def test_timestep_embedding_f32(dim):
    ops, L = K._ops()
    ts = [0.0, 3.0, 417.0, 999.0]
    t = torch.tensor(ts)
    buf, out = K.sentinel_rows(len(ts), dim, dim + 3, dtype=f32)
    L.check(L.timestep_embedding_f32(ops._p(t.to(DEV)), ops._p(out), out.stride(0), len(ts), dim, 10000.0, ops._stream()))
    ref64, ref32 = F64.timestep_embedding(t, dim, torch.float64), F64.timestep_embedding(t, dim, f32)
    for i, tv in enumerate(ts):
        within_rule("fm_timestep_embedding_f32", out[i], ref64[i], ref32[i], t=tv, dim=dim)
    assert K.untouched(buf, len(ts), dim)


def test_f32_kernels_refuse_bad_arguments_before_any_launch():
    ops, L = K._ops()
    x = torch.zeros(64, 64, device=DEV)
    w = torch.ones(64, device=DEV)
    s = ops._stream()
    K.refused(L.groupnorm_nhwc_f32(None, 64, None, 0, ops._p(w), ops._p(w), ops._p(x), 64, 1, 64, 64, 32, 1e-5, 0, s), "fm_groupnorm_nhwc_f32")
    K.refused(L.groupnorm_nhwc_f32(ops._p(x), 64, None, 0, ops._p(w), ops._p(w), ops._p(x), 64, 1, 64, 60, 32, 1e-5, 0, s), "C=60 groups=32")
    K.refused(L.unet_attention_f32(ops._p(x), 64, ops._p(x), 64, 1, 4, 1, 6, s), "ch=6")
    K.refused(L.unet_attention_f32(ops._p(x), 64, None, 64, 1, 4, 1, 8, s), "fm_unet_attention_f32")
    K.refused(L.unet_im2col_f32(None, 64, 64, None, 0, 0, 0, 0, ops._p(x), 64, 64, 1, 8, 8, 1, 1, 0, s), "fm_unet_im2col_f32")
    K.refused(L.unet_im2col_f32(ops._p(x), 64, 6, None, 0, 0, 0, 0, ops._p(x), 64, 64, 1, 8, 8, 1, 1, 0, s), "multiples of 4")
    K.refused(L.unet_im2col_f32(ops._p(x), 64, 8, None, 0, 0, 0, 0, ops._p(x), 64, 64, 1, 8, 8, 3, 1, 0, s), "too small")
    K.refused(L.add_f32(ops._p(x), 64, None, 64, ops._p(x), 64, 4, 64, s), "fm_add_f32")
    K.refused(L.silu_f32(None, ops._p(x), 64, s), "fm_silu_f32")
    K.refused(L.timestep_embedding_f32(ops._p(w), None, 64, 1, 64, 10000.0, s), "fm_timestep_embedding_f32")
    torch.cuda.synchronize()
    assert float(x.abs().max()) == 0.0                                    # nothing was launched
