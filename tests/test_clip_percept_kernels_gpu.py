"""The kernels behind the CLIP perceptual loss on a real MI355X, element by element against float64: fm_feat_distance, fm_quick_gelu_bwd(_f32),
fm_clip_embed_ln_bwd and fm_tap_add (csrc/clip.hip, csrc/elementwise.hip).

The fp32 rule (the project's): every element of an fp32 result is within
    8 x max(largest error of the same formula evaluated by torch in float32 on the CPU, half an fp32 ulp of the tensor's largest entry)
of the float64 value.  bf16 results add one bf16 rounding of the value: 2^-8 |value|, the unit roundoff of bf16."""
import pytest
import torch
import torch.nn.functional as F

from tests.clip_percept_util import feature_loss
from tests.parity_log import record

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -24
SENT = 7.0
bf16 = torch.bfloat16


def _ops():
    from fourm.hip import ops, _lib
    return ops, _lib


def gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def randn(*shape, scale=1.0, seed=0):
    return torch.randn(*shape, generator=gen(seed)) * scale


def strided(src, ld, dtype=torch.float32, fill=float("nan")):
    """src (rows, cols) on the device as a view of a (rows + 1, ld) buffer whose other entries are ``fill``; returns (buffer, view)."""
    buf = torch.full((src.shape[0] + 1, ld), fill, device=DEV, dtype=dtype)
    buf[:src.shape[0], :src.shape[1]] = src.to(DEV, dtype)
    return buf, buf[:src.shape[0], :src.shape[1]]


def untouched(buf, rows, cols):
    keep = torch.ones_like(buf, dtype=torch.bool)
    keep[:rows, :cols] = False
    return bool((buf[keep] == SENT).all())


def fp32_tol(ref, cpu32):
    return 8 * max(float((cpu32.double() - ref).abs().max()), U * float(ref.abs().max()))


def within(name, got, ref, tol):
    """Every element of ``got`` within ``tol`` (a number or a tensor) of ``ref``; returns the worst err / tol."""
    err = (got.double().cpu() - ref).abs()
    ratio = float((err / (torch.as_tensor(tol, dtype=torch.float64) + 1e-300)).max())
    assert bool((err <= tol).all()), f"{name}: worst err / tol {ratio:.3g}"
    return ratio


# ------------------------------------------------------------------------------------------------
# fm_feat_distance
# ------------------------------------------------------------------------------------------------
def feat_distance(pred, tgt, B, T, D, mode, loss, dpred, ldp=None, ldt=None, lddp=None):
    ops, L = _ops()
    return L.feat_distance(ops._p(pred), ldp if ldp is not None else pred.stride(0), ops._p(tgt), ldt if ldt is not None else tgt.stride(0), B, T, D, mode,
                           ops._p(loss), ops._p(dpred), lddp if lddp is not None else dpred.stride(0), ops._stream())


def distance_reference(p, t, B, T, D, mode, dtype):
    """(per-sample value (B,), its gradient (B * T, D)) of one tap in ``dtype`` by autograd: upstream's term divided by the batch size."""
    pr = p.to(dtype).view(B, T, D).requires_grad_()
    val = feature_loss(pr, t.to(dtype).view(B, T, D), mode) / B
    grad, = torch.autograd.grad(val.sum(), pr)
    return val.detach(), grad.reshape(B * T, D)


@pytest.mark.parametrize("mode", ["cosine", "l1"])
@pytest.mark.parametrize("D", [64, 192])
@pytest.mark.parametrize("T", [5, 17, 65])
def test_feat_distance(T, D, mode):
    """B = 3 samples of T tokens (fewer tokens than the 16 wavefronts of a workgroup, one more than 16, one more than 4 x 16), every operand
    with its own leading dimension > D and NaN around the live columns.  One token of the target equals the prediction (sign(0) = 0 in the
    L1 form).  The loss is accumulated: two calls on a pre-filled vector; both calls give the same gradient bits."""
    _, L = _ops()
    B = 3
    R = B * T
    seed = 10 * T + D
    p = randn(R, D, seed=seed)
    t = p + 0.5 * randn(R, D, seed=seed + 1)
    t[T // 2] = p[T // 2]
    m = L.FEAT_COSINE if mode == "cosine" else L.FEAT_L1
    _, pd = strided(p, D + 4)
    _, td = strided(t, D + 8)
    dbuf, dp = strided(torch.full((R, D), SENT), D + 12, fill=SENT)
    loss0 = randn(B, seed=seed + 2)
    loss = loss0.to(DEV)
    L.check(feat_distance(pd, td, B, T, D, m, loss, dp))
    first = dp.clone()
    L.check(feat_distance(pd, td, B, T, D, m, loss, dp))
    assert torch.equal(dp, first) and untouched(dbuf, R, D)
    val64, g64 = distance_reference(p, t, B, T, D, mode, torch.float64)
    val32, g32 = distance_reference(p, t, B, T, D, mode, torch.float32)
    r_g = within("dpred", dp, g64, fp32_tol(g64, g32))
    want = loss0.double() + 2 * val64
    r_l = within("loss", loss, want, fp32_tol(want, (loss0 + val32) + val32))
    print(f"feat_distance {mode} T={T} D={D}: dpred err/tol {r_g:.3f}, loss err/tol {r_l:.3f}")
    record("clip.percept.feat_distance", mode=mode, T=T, D=D, dpred_err_over_tol=r_g, loss_err_over_tol=r_l)
    if mode == "l1":
        assert float(dp[T // 2].abs().max()) == 0.0                            # identical rows: every sign is 0
    # a second pair of runs from the same start: the same bits (fixed-order sums, no atomics)
    loss_b = loss0.to(DEV)
    L.check(feat_distance(pd, td, B, T, D, m, loss_b, dp))
    L.check(feat_distance(pd, td, B, T, D, m, loss_b, dp))
    assert torch.equal(loss_b, loss) and torch.equal(dp, first)


def test_feat_distance_refusals():
    _, L = _ops()
    B, T, D = 2, 3, 64
    p, t = torch.ones(B * T, D, device=DEV), torch.ones(B * T, D, device=DEV)
    loss, dp = torch.full((B,), SENT, device=DEV), torch.full((B * T, D), SENT, device=DEV)

    def refused(match, pred=p, tgt=t, B=B, T=T, D=D, mode=0, loss=loss, dpred=dp, **kw):
        assert feat_distance(pred, tgt, B, T, D, mode, loss, dpred, **kw) == -1
        assert match in L.lib.fm_last_error().decode(), L.lib.fm_last_error().decode()

    for name in ("pred", "tgt", "loss", "dpred"):
        refused("null pointer", ldp=D, ldt=D, lddp=D, **{name: None})
    refused("neither", mode=2)
    refused("neither", mode=-1)
    for kw in (dict(B=0), dict(T=0), dict(D=0)):
        refused("must be positive", **kw)
    refused("multiple of 4", D=62)
    refused("multiple of 4", D=2052, ldp=2052, ldt=2052, lddp=2052)
    for name in ("ldp", "ldt", "lddp"):
        refused("ldp=", **{name: 60})
        refused("ldp=", **{name: 66})
    off = torch.ones(B * T * D + 1, device=DEV)[1:].view(B * T, D)
    refused("16-byte aligned", pred=off)
    refused("16-byte aligned", tgt=off)
    refused("16-byte aligned", dpred=off)
    torch.cuda.synchronize()
    assert bool((loss == SENT).all()) and bool((dp == SENT).all())               # nothing was launched by a refused call


# ------------------------------------------------------------------------------------------------
# fm_quick_gelu_bwd, fm_quick_gelu_bwd_f32
# ------------------------------------------------------------------------------------------------
def qgelu_grad(da, u):
    s = torch.sigmoid(1.702 * u)
    return da * (s * (1 + 1.702 * u * (1 - s)))


@pytest.mark.parametrize("H", [8, 520])
@pytest.mark.parametrize("R", [1, 130])
def test_quick_gelu_bwd_bf16(R, H):
    """Pre-activations uniform in [-12, 12] (both tails of the sigmoid), Hp = H + 8, leading dimensions Hp + 8.  Bound per element: one bf16
    rounding of the value, 2^-8 |ref|, plus the fp32 evaluation in front of it: 2^-16 |ref| (the fast exponential and the rounding of its
    argument, |1.702 u| 2^-24 <= 1.3e-6 at |u| = 12; the allowance of the QuickGELU epilogue's own test) and 2^-21 |da| (1 + 1.702 u (1 - s)
    cancels near u = -0.75).  Columns [H, Hp) are written as zero - the layout rule of fm_gelu_bwd, the GEMM behind it reduces over Hp - and
    nothing past Hp is touched."""
    ops, L = _ops()
    Hp, ld = H + 8, H + 16
    u = ((torch.rand(R, Hp, generator=gen(31 + R + H)) * 24 - 12).to(bf16))
    da = randn(R, Hp, seed=32 + R + H).to(bf16)
    _, ud = strided(u, ld, bf16)
    _, dd = strided(da, ld, bf16)
    obuf = torch.full((R + 1, ld), SENT, device=DEV, dtype=bf16)
    out = obuf[:R, :Hp]
    ops.quick_gelu_bwd(dd, ud, out, H, Hp)
    ref = qgelu_grad(da[:, :H].double(), u[:, :H].double())
    tol = (2.0 ** -8 + 2.0 ** -16) * ref.abs() + 2.0 ** -21 * da[:, :H].double().abs()
    r = within("dpre", out[:, :H], ref, tol)
    print(f"quick_gelu_bwd bf16 R={R} H={H}: err/tol {r:.3f}")
    record("clip.percept.quick_gelu_bwd", dtype="bf16", R=R, H=H, err_over_tol=r)
    assert float(out[:, H:].float().abs().max()) == 0.0 and untouched(obuf, R, Hp)


@pytest.mark.parametrize("H", [8, 520])
@pytest.mark.parametrize("R", [1, 130])
def test_quick_gelu_bwd_f32(R, H):
    """The fp32 rule against torch's float32 evaluation of da s (1 + 1.702 u (1 - s)); leading dimensions that are no multiple of 4 (the fp32
    entry point takes any), nothing past column H is touched."""
    ops, L = _ops()
    u = torch.rand(R, H, generator=gen(41 + R + H)) * 24 - 12
    da = randn(R, H, seed=42 + R + H)
    _, ud = strided(u, H + 9)
    _, dd = strided(da, H + 3)
    obuf = torch.full((R + 1, H + 5), SENT, device=DEV)
    out = obuf[:R, :H]
    ops.quick_gelu_bwd(dd, ud, out, H, H + 8)
    ref = qgelu_grad(da.double(), u.double())
    r = within("dpre", out, ref, fp32_tol(ref, qgelu_grad(da, u)))
    print(f"quick_gelu_bwd f32 R={R} H={H}: err/tol {r:.3f}")
    record("clip.percept.quick_gelu_bwd", dtype="f32", R=R, H=H, err_over_tol=r)
    assert untouched(obuf, R, H)


def test_quick_gelu_bwd_refusals():
    ops, L = _ops()
    R, H, Hp = 4, 8, 16
    a16, out16 = torch.zeros(R, Hp, device=DEV, dtype=bf16), torch.full((R, Hp), SENT, device=DEV, dtype=bf16)
    a32, out32 = torch.zeros(R, Hp, device=DEV), torch.full((R, Hp), SENT, device=DEV)
    s = ops._stream()

    def msg():
        return L.lib.fm_last_error().decode()

    assert L.quick_gelu_bwd(None, Hp, ops._p(a16), Hp, ops._p(out16), Hp, R, H, Hp, s) == -1 and "null pointer" in msg()
    assert L.quick_gelu_bwd(ops._p(a16), Hp, ops._p(a16), Hp, None, Hp, R, H, Hp, s) == -1 and "null pointer" in msg()
    assert L.quick_gelu_bwd(ops._p(a16), Hp, ops._p(a16), Hp, ops._p(out16), Hp, R, H, 14, s) == -1 and "multiple of 4" in msg()
    assert L.quick_gelu_bwd(ops._p(a16), Hp, ops._p(a16), Hp, ops._p(out16), Hp, R, 20, Hp, s) == -1 and "Hp >= H" in msg()
    assert L.quick_gelu_bwd(ops._p(a16), Hp, ops._p(a16), Hp, ops._p(out16), 12, R, H, Hp, s) == -1 and "leading dims" in msg()
    assert L.quick_gelu_bwd(ops._p(a16), Hp, ops._p(a16), Hp, ops._p(out16), 18, R, H, Hp, s) == -1 and "leading dims" in msg()
    assert L.quick_gelu_bwd(ops._p(a16.view(-1)[1:]), Hp, ops._p(a16), Hp, ops._p(out16), Hp, R - 1, H, Hp, s) == -1 and "8-byte aligned" in msg()
    assert L.quick_gelu_bwd_f32(ops._p(a32), Hp, None, Hp, ops._p(out32), Hp, R, H, s) == -1 and "null pointer" in msg()
    assert L.quick_gelu_bwd_f32(ops._p(a32), Hp, ops._p(a32), Hp, ops._p(out32), Hp, 0, H, s) == -1 and "positive" in msg()
    assert L.quick_gelu_bwd_f32(ops._p(a32), Hp, ops._p(a32), Hp, ops._p(out32), 6, R, H, s) == -1 and ">= H" in msg()
    torch.cuda.synchronize()
    assert bool((out16 == SENT).all()) and bool((out32 == SENT).all())


# ------------------------------------------------------------------------------------------------
# fm_clip_embed_ln_bwd
# ------------------------------------------------------------------------------------------------
def embed_ln_bwd(dy, patches, f32_rows, pos, w, dpat, B, G, D, eps=1e-5, lddy=None, ldp=None, lddp=None):
    ops, L = _ops()
    return L.clip_embed_ln_bwd(ops._p(dy), lddy if lddy is not None else dy.stride(0), ops._p(patches), ldp if ldp is not None else patches.stride(0),
                               1 if f32_rows else 0, ops._p(pos), ops._p(w), ops._p(dpat), lddp if lddp is not None else dpat.stride(0), B, G, D, eps,
                               ops._stream())


@pytest.mark.parametrize("rows_f32", [False, True], ids=["bf16", "f32"])
@pytest.mark.parametrize("B,G,D", [(3, 16, 128), (2, 64, 128), (2, 12, 192)])
def test_clip_embed_ln_bwd(B, G, D, rows_f32):
    """The grids of clip_a native, clip_a interpolated and clip_b interpolated.  Reference: float64 autograd of
    layer_norm(cat(cls, patches) + pos) for a random gradient of the normalised rows; the class rows of that gradient are NaN on the device
    (they are skipped).  f32 rows by the fp32 rule against torch's float32 autograd; bf16 rows add the rounding of the store, 2^-8 |ref|."""
    _, L = _ops()
    seed = B + 3 * G + D
    dt = bf16 if not rows_f32 else torch.float32
    pat = randn(B * G, D, seed=seed).to(dt)
    cls, pos = randn(D, scale=0.5, seed=seed + 1), randn(G + 1, D, scale=0.5, seed=seed + 2)
    w, b = 1.0 + 0.2 * randn(D, seed=seed + 3), 0.1 * randn(D, seed=seed + 4)
    dy = randn(B, G + 1, D, seed=seed + 5)

    def reference(dtype):
        pr = pat.to(dtype).requires_grad_()
        rows = torch.cat([cls.to(dtype).expand(B, 1, D), pr.view(B, G, D)], 1) + pos.to(dtype)
        out = F.layer_norm(rows, (D,), w.to(dtype), b.to(dtype), 1e-5)
        grad, = torch.autograd.grad(out, pr, dy.to(dtype))
        return grad

    ref, own = reference(torch.float64), reference(torch.float32)
    dyn = dy.clone()
    dyn[:, 0] = float("nan")
    _, dyd = strided(dyn.view(B * (G + 1), D), D + 4)
    _, pd = strided(pat, D + 8, dt)
    obuf = torch.full((B * G + 1, D + 8), SENT, device=DEV, dtype=dt)
    out = obuf[:B * G, :D]
    L.check(embed_ln_bwd(dyd, pd, rows_f32, pos.to(DEV), w.to(DEV), out, B, G, D))
    tol = fp32_tol(ref, own) + (0 if rows_f32 else 2.0 ** -8 * ref.abs())
    r = within("d_patches", out, ref, tol)
    print(f"clip_embed_ln_bwd B={B} G={G} D={D} f32={rows_f32}: err/tol {r:.3f}")
    record("clip.percept.embed_ln_bwd", B=B, G=G, D=D, rows_f32=rows_f32, err_over_tol=r)
    assert bool(torch.isfinite(out.float()).all()) and untouched(obuf, B * G, D)


def test_clip_embed_ln_bwd_refusals():
    _, L = _ops()
    B, G, D = 2, 3, 64
    p16, p32 = torch.zeros(B * G, D, device=DEV, dtype=bf16), torch.zeros(B * G, D, device=DEV)
    dy, pos, w = torch.zeros(B * (G + 1), D, device=DEV), torch.zeros(G + 1, D, device=DEV), torch.ones(D, device=DEV)
    out = torch.full((B * G, D), SENT, device=DEV)

    def refused(match, dy=dy, patches=p32, f32_rows=True, pos=pos, w=w, dpat=out, B=B, G=G, D=D, **kw):
        assert embed_ln_bwd(dy, patches, f32_rows, pos, w, dpat, B, G, D, **kw) == -1
        assert match in L.lib.fm_last_error().decode(), L.lib.fm_last_error().decode()

    for name in ("dy", "patches", "pos", "w", "dpat"):
        refused("null pointer", lddy=D, ldp=D, lddp=D, **{name: None})
    for kw in (dict(B=0), dict(G=0), dict(D=0)):
        refused("must be positive", **kw)
    refused("multiple of 4", D=62)
    refused("multiple of 4", D=2052, lddy=2052, ldp=2052, lddp=2052)
    for name in ("lddy", "ldp", "lddp"):
        refused("lddy=", **{name: 60})
        refused("lddy=", **{name: 66})
    refused("16-byte aligned", patches=p16.view(-1)[4:4 + (B * G - 1) * D].view(B * G - 1, D), f32_rows=False, B=1)
    refused("16-byte aligned", w=torch.ones(D + 1, device=DEV)[1:])
    refused("16-byte aligned", dpat=torch.zeros(B * G * D + 1, device=DEV)[1:].view(B * G, D))
    refused("exceed the grid", B=2 ** 30, G=3)
    torch.cuda.synchronize()
    assert bool((out == SENT).all())


# ------------------------------------------------------------------------------------------------
# fm_tap_add
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_bf", [True, False], ids=["bf16copy", "nocopy"])
@pytest.mark.parametrize("with_scale", [True, False], ids=["scaled", "plain"])
def test_tap_add(with_scale, with_bf):
    """g += row_scale[b] * dtap is exact in fp32: the product and the sum are rounded separately, as the two torch operations are; the bf16
    copy is the round-to-nearest of the new g.  3 samples of 17 rows, D = 64, padded leading dimensions, sentinels around every output."""
    ops, L = _ops()
    B, T, D = 3, 17, 64
    R = B * T
    g0, d = randn(R, D, seed=71), randn(R, D, seed=72)
    s = (1.0 + randn(B, seed=73)).to(DEV) if with_scale else None
    gbuf, g = strided(g0, D + 4, fill=SENT)
    _, dd = strided(d, D + 8)
    bbuf = torch.full((R + 1, D + 12), SENT, device=DEV, dtype=bf16)
    gb = bbuf[:R, :D] if with_bf else None
    want = g.clone()
    want = want + (s.repeat_interleave(T)[:, None] * dd if with_scale else dd)
    ops.tap_add(g, dd, gb, s, T)
    assert torch.equal(g, want) and untouched(gbuf, R, D)
    if with_bf:
        assert torch.equal(gb, want.to(bf16)) and untouched(bbuf, R, D)
    ops.tap_add(g, dd, gb, s, T, R=T)                                          # the first sample's rows only
    assert torch.equal(g[T:], want[T:]) and not torch.equal(g[:T], want[:T])


def test_tap_add_refusals():
    ops, L = _ops()
    R, D = 6, 64
    g, d = torch.full((R, D), SENT, device=DEV), torch.ones(R, D, device=DEV)
    gb, sc = torch.full((R, D), SENT, device=DEV, dtype=bf16), torch.ones(2, device=DEV)
    st = ops._stream()

    def call(g=g, ldg=D, gb=gb, ldgb=D, d=d, ldt=D, sc=sc, rps=3, R=R, D=D):
        return L.tap_add(ops._p(g), ldg, ops._p(gb), ldgb, ops._p(d), ldt, ops._p(sc), rps, R, D, st)

    def refused(match, **kw):
        assert call(**kw) == -1
        assert match in L.lib.fm_last_error().decode(), L.lib.fm_last_error().decode()

    refused("null pointer", g=None)
    refused("null pointer", d=None)
    refused("positive", R=0)
    refused("multiple of 4", D=62)
    refused("rows_per_sample", rps=0)
    for name in ("ldg", "ldgb", "ldt"):
        refused("leading dims", **{name: 60})
        refused("leading dims", **{name: 66})
    refused("aligned", g=torch.zeros(R * D + 1, device=DEV)[1:].view(R, D))
    refused("aligned", d=torch.zeros(R * D + 1, device=DEV)[1:].view(R, D))
    refused("aligned", gb=torch.zeros(R * D + 1, device=DEV, dtype=bf16)[1:].view(R, D))
    torch.cuda.synchronize()
    assert bool((g == SENT).all()) and bool((gb == SENT).all())


# ------------------------------------------------------------------------------------------------
# fm_attn_f32_bwd with scratch: dK / dV reduced in query order (the fp32 mode's reproducible backward)
# ------------------------------------------------------------------------------------------------
def test_attn_f32_bwd_ordered_reduction():
    """The fp32 attention backward with stat_m / stat_l given: dQ, dK, dV by the fp32 rule against float64 autograd (yardstick: torch's float32
    autograd on the CPU), the same bits on a second run, and dK / dV ACCUMULATED onto what the buffers held.  Nq != Nk, two heads, two samples."""
    ops, L = _ops()
    B, H, Nq, Nk, D = 2, 2, 17, 21, 128
    scale = 64 ** -0.5
    q, k, v, do = randn(B * Nq, D, seed=81), randn(B * Nk, D, seed=82), randn(B * Nk, D, seed=83), randn(B * Nq, D, seed=84)

    def reference(dtype):
        qq, kk, vv = (t.to(dtype).requires_grad_() for t in (q, k, v))
        def heads(t, n):
            return t.view(B, n, H, 64).permute(0, 2, 1, 3)
        o = torch.softmax(heads(qq, Nq) @ heads(kk, Nk).transpose(-1, -2) * scale, -1) @ heads(vv, Nk)
        return torch.autograd.grad(o.permute(0, 2, 1, 3).reshape(B * Nq, D), (qq, kk, vv), do.to(dtype))

    ref, own = reference(torch.float64), reference(torch.float32)
    qd, kd, vd, dod = (t.to(DEV) for t in (q, k, v, do))
    o = torch.empty(B * Nq, D, device=DEV)
    ops.attn_fwd(qd, kd, vd, o, B, H, Nq, Nk, scale)
    sm, sl = torch.zeros(B, H, Nq, device=DEV), torch.zeros(B, H, Nq, device=DEV)
    outs = []
    for _ in range(2):
        dq, dk, dv = torch.empty_like(qd), torch.empty_like(kd), torch.empty_like(vd)
        ops.attn_bwd(qd, kd, vd, o, dod, dq, dk, dv, B, H, Nq, Nk, scale, sm, sl)
        outs.append((dq, dk, dv))
    for name, a, b, r, w in zip(("dq", "dk", "dv"), outs[0], outs[1], ref, own):
        assert torch.equal(a, b), name
        ratio = within(name, a, r, fp32_tol(r, w))
        record("clip.percept.attn_f32_bwd_ordered", tensor=name, err_over_tol=ratio)
    # accumulation: the entry point itself adds onto dK / dV (ops.attn_bwd zeroes them first)
    a = L.AttnArgs()
    a.Q, a.K, a.V, a.O = ops._p(qd), ops._p(kd), ops._p(vd), ops._p(o)
    a.ldq = a.ldk = a.ldv = a.ldo = a.lddo = a.lddq = a.lddk = a.lddv = D
    a.B, a.H, a.Nq, a.Nk, a.head_dim, a.mask_kind, a.scale = B, H, Nq, Nk, 64, L.MASK_NONE, scale
    a.stat_m, a.stat_l = ops._p(sm), ops._p(sl)
    dq2, dk2, dv2 = torch.empty_like(qd), torch.full_like(kd, 1.0), torch.full_like(vd, -2.0)
    a.dO, a.dQ, a.dK, a.dV = ops._p(dod), ops._p(dq2), ops._p(dk2), ops._p(dv2)
    L.check(L.attn_f32_bwd(ops.C.byref(a), ops._stream()))
    assert torch.equal(dq2, outs[0][0]) and torch.equal(dk2, outs[0][1] + 1.0) and torch.equal(dv2, outs[0][2] - 2.0)
