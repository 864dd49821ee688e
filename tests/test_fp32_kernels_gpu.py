"""Per-kernel numerics of the fp32 verification path on a real MI355X: every entry point of csrc/fp32_verify.hip and
fm_cross_entropy_f32 against a float64 restatement of the same operation on the same fp32 inputs.  The model-level parity claim
(tests/test_model_gpu.py test_fp32_verification_mode) rests on these kernels; here each one is held, element by element, to a bound
derived from the fp32 unit roundoff u = 2^-24 and written next to its check.  At such bounds a dropped K-step, tile, reduction term or
mask case fails by orders of magnitude, and a bound of this kind cannot fail by chance."""
import pytest
import torch
import torch.nn.functional as F

from tests.parity_log import record
from tests.test_kernels_gpu import CE_COUNTS, CE_VOCABS, ce_reference, segmented_ce_problem

pytestmark = pytest.mark.gpu

DEV = "cuda"
U = 2.0 ** -24           # fp32 unit roundoff
FN = 2.0 ** -20          # a few ulps of expf / erff / tanhf / rsqrtf / logf
ETA = 2.0 ** -126        # smallest normal fp32: results below it may be flushed to zero


def _ops():
    from fourm.hip import ops, _lib
    return ops, _lib


def randn(*shape, scale=1.0, seed=0):
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def uniform(*shape, lo, hi, seed=0):
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    return (torch.rand(*shape, generator=g) * (hi - lo) + lo).to(DEV)


def check(name, got, ref, tol):
    """|got - ref| <= tol element-wise (float64); returns the worst err / tol."""
    err = (got.double() - ref).abs()
    bad = err > tol
    ratio = float((err / (tol + 1e-300)).max()) if err.numel() else 0.0
    assert not bool(bad.any()), f"{name}: {int(bad.sum())} of {err.numel()} outside the bound, worst err/tol {ratio:.3g}"
    return ratio


def frob(got, ref):
    return float((got.double() - ref).norm() / (ref.norm() + 1e-300))


def padded(src, ld, offset=0, fill=0.0):
    """src (rows, cols) copied into a (rows, ld) buffer at column ``offset``; returns the (rows, cols) view."""
    buf = torch.full((src.shape[0], ld), fill, device=DEV)
    buf[:, offset:offset + src.shape[1]] = src
    return buf[:, offset:offset + src.shape[1]]


# ------------------------------------------------------------------------------------------------
# fm_gemm_f32
# ------------------------------------------------------------------------------------------------
def takes_mfma(x_ptr, sxm, sxk, w_ptr, swn, swk, epilogue, L):
    """fm_gemm_f32's dispatch (fp32_verify.hip, fm_gemm_f32):
        nt = p->sxk == 1 && p->swk == 1 && !p->groups && !p->seg_start && p->epilogue != FM_EPI_SWIGLU && p->sxm % 4 == 0 &&
             p->swn % 4 == 0 && ((((uintptr_t)p->X | (uintptr_t)p->W)) & 15) == 0;
    nt -> gemm_f32_mfma_kernel (fp32 matrix cores), otherwise gemm_f32_kernel (LDS-tiled FMA)."""
    return (sxk == 1 and swk == 1 and epilogue != L.EPI_SWIGLU and sxm % 4 == 0 and swn % 4 == 0 and (x_ptr | w_ptr) % 16 == 0)


FORMS = ["mfma", "x_offset", "x_ld_odd", "w_transposed", "x_transposed"]


class Operands:
    """X0 (M, K) and W0 / W2 (N, K) laid out as one operand form:
      mfma          rows padded to a multiple of 4 floats, 16-byte aligned: the matrix-core kernel (except SWIGLU)
      x_offset      X starts one float into its buffer (4-byte aligned only): the FMA kernel
      x_ld_odd      X row stride = 1 mod 4: the FMA kernel
      w_transposed  W a transposed view (swn = 1, swk = N), as the fp32 heads' dY reads the (V, D) master (engine.py, ops.make_groups
                    transposed=1) and engine.wt() passes W for dX: the FMA kernel
      x_transposed  X read through sxm = 1, sxk = M (ops.gemm_tn's X := a^T): the FMA kernel; launched through GemmF32Args directly,
                    since ops._gemm_f32 only takes sxk = 1"""

    def __init__(self, form, X0, W0, W2=None):
        M, K = X0.shape
        self.form, self.M, self.N, self.K = form, M, W0.shape[0], K
        ld = (K + 3) // 4 * 4
        self.x = X0.t().contiguous() if form == "x_transposed" else (
            padded(X0, ld + 4, 1) if form == "x_offset" else padded(X0, ld + 1 if form == "x_ld_odd" else ld))
        if form == "w_transposed":
            self.w = W0.t().contiguous().t()
            self.w2 = W2.t().contiguous().t() if W2 is not None else None
        else:
            self.w = padded(W0, ld)
            self.w2 = padded(W2, ld) if W2 is not None else None
        if form == "x_transposed":
            self.sxm, self.sxk = 1, M
        else:
            self.sxm, self.sxk = self.x.stride(0), 1
        self.swn, self.swk = self.w.stride(0), self.w.stride(1)

    def mfma(self, epilogue, L):
        return takes_mfma(self.x.data_ptr(), self.sxm, self.sxk, self.w.data_ptr(), self.swn, self.swk, epilogue, L)

    def launch(self, out, *, epilogue, bias=None, res=None, out2=None, bias2=None, Hp=0, accumulate=False):
        ops, L = _ops()
        if self.form != "x_transposed":
            return ops._gemm_f32(self.x, self.w, out, epilogue=epilogue, bias=bias, res=res, w2=self.w2 if epilogue == L.EPI_SWIGLU else None,
                                 bias2=bias2, out2=out2, Hp=Hp, accumulate=accumulate)
        a = L.GemmF32Args()
        a.X, a.W, a.W2, a.out, a.out2 = ops._p(self.x), ops._p(self.w), ops._p(self.w2 if epilogue == L.EPI_SWIGLU else None), ops._p(out), ops._p(out2)
        a.res, a.bias, a.bias2 = ops._p(res), ops._p(bias), ops._p(bias2)
        a.sxm, a.sxk, a.swn, a.swk = self.sxm, self.sxk, self.swn, self.swk
        a.M, a.N, a.K = self.M, self.N, self.K
        a.ldo, a.ldo2, a.ldr = out.stride(0), out2.stride(0) if out2 is not None else 0, res.stride(0) if res is not None else 0
        a.Hp, a.epilogue, a.accumulate = Hp, epilogue, 1 if accumulate else 0
        L.check(L.gemm_f32(ops.C.byref(a), ops._stream()))
        return out


def gelu64(v):
    return 0.5 * v * (1.0 + torch.erf(v * 0.5 ** 0.5))


SENT = 7.0


def out_buf(M, N, extra=5):
    """(M, N) view of an (M + 1, N + extra) buffer full of the sentinel: what the kernel must not touch is checked afterwards."""
    buf = torch.full((M + 1, N + extra), SENT, device=DEV)
    return buf, buf[:M, :N]


def untouched(buf, view_rows, view_cols):
    mask = torch.ones_like(buf, dtype=torch.bool)
    mask[:view_rows, :view_cols] = False
    return bool((buf[mask] == SENT).all())


GEMM_SHAPES = [(1, 1, 1), (31, 64, 3), (128, 127, 31), (129, 130, 33), (1000, 2730, 768), (31, 2730, 4100), (129, 64, 4100),
               (128, 130, 768), (1000, 1, 33), (1, 127, 4100)]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
def test_gemm_f32_epilogues(M, N, K, form):
    """fm_gemm_f32 on both kernels (the operand form picks one; ``takes_mfma`` states the rule), every epilogue, against float64.
    Shapes straddle the 64 x 64 tile / 16-wide K-step of gemm_f32_kernel and the 128 x 128 tile / 32-wide K-step of gemm_f32_mfma_kernel.
    Bound per element (deterministic gamma_K bound of a K-term dot product, + bias / res roundings):
        |v - ref| <= (K + 4) u S,   S = (|X| @ |W|^T) + |bias| (+ |res|)
    and for the activations that bound carried through the function's slope plus FN |f(ref)| (+ an absolute term where noted)."""
    ops, L = _ops()
    X0 = randn(M, K, seed=1000 + M + K)
    W0 = randn(N, K, scale=K ** -0.5, seed=2000 + N + K)
    W2 = randn(N, K, scale=K ** -0.5, seed=3000 + N + K)
    bias, bias2 = randn(N, seed=4000 + N), randn(N, seed=5000 + N)
    resb = randn(M, N + 3, seed=6000 + M)
    res = resb[:, :N]                                            # strided residual (ldr = N + 3)
    ops_ = Operands(form, X0, W0, W2)
    X64, W64, W264 = X0.double(), W0.double(), W2.double()
    acc = X64 @ W64.t()
    S = X0.abs().double() @ W0.abs().double().t()
    g = (K + 4) * U
    b64, r64 = bias.double(), res.double()
    worst = {}

    def run(name, epilogue, want, tol, **kw):
        buf, out = out_buf(M, N)
        ops_.launch(out, epilogue=epilogue, **kw)
        worst[name] = check(f"{form} {name}", out, want, tol)
        assert untouched(buf, M, N), (form, name)
        return out

    mf = {e: ops_.mfma(e, L) for e in (L.EPI_F32, L.EPI_SWIGLU)}
    assert mf[L.EPI_F32] == (form == "mfma" and M >= 1), (form, "dispatch")
    assert not mf[L.EPI_SWIGLU]
    run("f32", L.EPI_F32, acc, g * S)
    run("f32_bias", L.EPI_F32, acc + b64, g * (S + b64.abs()), bias=bias)
    run("f32_bias_res", L.EPI_F32, acc + b64 + r64, g * (S + b64.abs() + r64.abs()), bias=bias, res=res)
    run("bf16_bias", L.EPI_BF16, acc + b64, g * (S + b64.abs()), bias=bias)                     # BF16 here: the plain fp32 result
    run("residual", L.EPI_RESIDUAL, r64 + acc + b64, g * (S + b64.abs() + r64.abs()), bias=bias, res=res)
    v, tv = acc + b64, g * (S + b64.abs())
    # tanh' <= 1; tanhf is within a few ulps
    run("tanh", L.EPI_TANH, torch.tanh(v), tv + FN * torch.tanh(v).abs(), bias=bias)
    # GELU: |gelu'| <= 1.13; gelu32 = 0.5 v (1 + erff(v / sqrt 2)): the erff error (2 ulp of a value in (-1, 1)) and the rounding of the
    # argument / of 1 + erf give <= 2.3 u |v| absolute, the two products FN-covered relative roundings
    buf2, pre = out_buf(M, N, extra=9)
    out = run("gelu", L.EPI_GELU, gelu64(v), 1.2 * tv + 4 * U * v.abs() + FN * gelu64(v).abs(), bias=bias, out2=pre)
    worst["gelu_pre"] = check(f"{form} gelu out2", pre, v, tv)
    assert untouched(buf2, M, N)
    # SwiGLU (the FMA kernel only, whatever the form): out = silu(g) u with |silu'| <= 1.1; out2 = [g | pad | u] at columns 0 and Hp
    Hp = (N + 16) // 16 * 16                                     # Hp > H, like 2730 / 2752
    u64 = X64 @ W264.t() + bias2.double()
    tu = g * (X0.abs().double() @ W2.abs().double().t() + bias2.double().abs())
    gu_buf = torch.full((M + 1, 2 * Hp + 3), SENT, device=DEV)
    gu = gu_buf[:M]
    silu = v * torch.sigmoid(v)
    run("swiglu", L.EPI_SWIGLU, silu * u64, 1.1 * tv * u64.abs() + silu.abs() * tu + FN * (silu * u64).abs(),
        bias=bias, bias2=bias2, out2=gu, Hp=Hp)
    worst["swiglu_g"] = check(f"{form} swiglu g", gu[:, :N], v, tv)
    worst["swiglu_u"] = check(f"{form} swiglu u", gu[:, Hp:Hp + N], u64, tu)
    keep = torch.ones_like(gu_buf, dtype=torch.bool)
    keep[:M, :N] = False
    keep[:M, Hp:Hp + N] = False
    assert bool((gu_buf[keep] == SENT).all())
    # accumulate = 1 into a non-zero out: out0 + result, one more rounding (u |out0 + ref|)
    for name, epi, kw, want, tol in (("acc_f32_bias_res", L.EPI_F32, dict(bias=bias, res=res), acc + b64 + r64, g * (S + b64.abs() + r64.abs())),
                                     ("acc_bf16", L.EPI_BF16, {}, acc, g * S)):
        buf, out = out_buf(M, N)
        out0 = randn(M, N, seed=7000 + M + N)
        out.copy_(out0)
        ops_.launch(out, epilogue=epi, accumulate=True, **kw)
        worst[name] = check(f"{form} {name}", out, out0.double() + want, tol + 2 * U * (out0.double() + want).abs())
        assert untouched(buf, M, N)
    record("fp32_kernels.gemm_f32", M=M, N=N, K=K, form=form, mfma=mf[L.EPI_F32], worst_err_over_bound=worst)


@pytest.mark.parametrize("M,N,K", [(129, 130, 33), (1000, 2730, 768), (128, 127, 4100)])
def test_gemm_f32_accumulate_rule_is_the_same_on_both_kernels(M, N, K):
    """accumulate = 1 is defined for FM_EPI_F32 / FM_EPI_BF16 only.  gemm_f32_kernel wrote ``*o = f(v)`` for GELU / TANH / RESIDUAL /
    SWIGLU (ignoring accumulate) while gemm_f32_mfma_kernel added f(v) to out, so the result depended on operand alignment; fm_gemm_f32
    now refuses those combinations on either operand form and leaves out untouched, and the allowed ones agree between the kernels."""
    ops, L = _ops()
    X0, W0 = randn(M, K, seed=71), randn(N, K, scale=K ** -0.5, seed=72)
    bias, res = randn(N, seed=73), randn(M, N, seed=74)
    outs = {}
    for form in ("mfma", "x_offset"):
        o = Operands(form, X0, W0, W0)
        assert o.mfma(L.EPI_F32, L) == (form == "mfma")
        for epi in (L.EPI_GELU, L.EPI_TANH, L.EPI_RESIDUAL, L.EPI_SWIGLU):
            buf, out = out_buf(M, N)
            kw = dict(res=res) if epi == L.EPI_RESIDUAL else (dict(out2=torch.zeros(M, 2 * N + 32, device=DEV), Hp=N + 16) if epi == L.EPI_SWIGLU else {})
            with pytest.raises(RuntimeError, match="accumulate"):
                o.launch(out, epilogue=epi, bias=bias, accumulate=True, **kw)
            torch.cuda.synchronize()
            assert bool((buf == SENT).all()), (form, epi)
        for epi in (L.EPI_F32, L.EPI_BF16):
            out = randn(M, N, seed=75).clone()
            o.launch(out, epilogue=epi, bias=bias, res=res if epi == L.EPI_F32 else None, accumulate=True)
            outs[(form, epi)] = out
    ref_f32 = randn(M, N, seed=75).double() + X0.double() @ W0.double().t() + bias.double() + res.double()
    tol = (K + 6) * U * (randn(M, N, seed=75).double().abs() + X0.abs().double() @ W0.abs().double().t() + bias.double().abs() + res.double().abs())
    for form in ("mfma", "x_offset"):
        check(f"{form} accumulate f32", outs[(form, L.EPI_F32)], ref_f32, tol)
        check(f"{form} accumulate bf16", outs[(form, L.EPI_BF16)], ref_f32 - res.double(), tol)


@pytest.mark.parametrize("M,N,K", [(129, 130, 33), (1000, 2730, 768), (31, 2730, 4100), (128, 128, 128)])
def test_gemm_f32_kernels_bitwise_agreement(M, N, K):
    """Informational (recorded, not asserted beyond the fp32 bound): the fraction of outputs on which gemm_f32_mfma_kernel and
    gemm_f32_kernel agree bit for bit on the same inputs (same K order, fmaf chain vs. v_mfma_f32_32x32x2_f32)."""
    ops, L = _ops()
    X0, W0 = randn(M, K, seed=81), randn(N, K, scale=K ** -0.5, seed=82)
    a, b = Operands("mfma", X0, W0), Operands("x_offset", X0, W0)
    assert a.mfma(L.EPI_F32, L) and not b.mfma(L.EPI_F32, L)
    oa, ob = torch.zeros(M, N, device=DEV), torch.zeros(M, N, device=DEV)
    a.launch(oa, epilogue=L.EPI_F32)
    b.launch(ob, epilogue=L.EPI_F32)
    S = X0.abs().double() @ W0.abs().double().t()
    check("mfma vs fma kernel", oa, ob.double(), 2 * (K + 4) * U * S)
    same = float((oa == ob).double().mean())
    record("fp32_kernels.gemm_f32_bitwise", M=M, N=N, K=K, fraction_bitwise_equal=same,
           max_abs_diff_over_uS=float(((oa.double() - ob.double()).abs() / (U * S + 1e-300)).max()))


def test_gemm_tn_f32():
    """ops.gemm_tn with fp32 operands (X := a^T through sxk, W := b^T, accumulate = 1): the fp32 weight gradient dW += dY^T X of
    the verification path, accumulated into a non-zero buffer; rows not multiples of any tile."""
    ops, L = _ops()
    R, N, K = 1037, 130, 769
    a = randn(R, N + 3, seed=91)[:, :N]
    b = randn(R, K + 1, seed=92)[:, :K]
    fill = randn(N, K, seed=93)
    out = fill.clone()
    ops.gemm_tn(a, b, out)
    ref = fill.double() + a.double().t() @ b.double()
    tol = (R + 4) * U * (a.abs().double().t() @ b.abs().double()) + 2 * U * ref.abs()
    record("fp32_kernels.gemm_tn", worst_err_over_bound=check("gemm_tn f32", out, ref, tol))


def _segments(ops, counts, seed):
    n_heads = len(counts)
    R = sum(counts) + 45
    head = torch.full((R,), -1, dtype=torch.int32)
    idx = torch.randperm(R, generator=torch.Generator().manual_seed(seed))
    o = 0
    for h, c in enumerate(counts):
        head[idx[o:o + c]] = h
        o += c
    head = head.to(DEV)
    Rp = ops.padded_rows(R, n_heads)
    seg_start = torch.zeros(n_heads, dtype=torch.int32, device=DEV)
    seg_count = torch.zeros_like(seg_start)
    perm = torch.zeros(Rp, dtype=torch.int32, device=DEV)
    r2p = torch.zeros(R, dtype=torch.int32, device=DEV)
    tile_group = torch.zeros(Rp // ops.SEG, dtype=torch.int32, device=DEV)
    ops.segment_rows(head, n_heads, seg_start, seg_count, perm, r2p, tile_group)
    assert seg_count.tolist() == counts
    return R, Rp, head, seg_start, seg_count, perm, tile_group


def test_gemm_f32_grouped_heads():
    """The segmented head GEMMs as the fp32 heads run them: logits = Y W_h^T (gemm_nt_grouped, groups + tile_group), dY = dL W_h with
    W_h read transposed through strides (groups transposed=1, engine.py heads backward) and dW_h += dL^T Y (gemm_tn_grouped,
    seg_start / seg_count) at vocabularies 30000 / 16384 / 4096 / 23 plus an empty head, row counts not multiples of ops.SEG.
    Every head's segment equals its float64 matmul within (K + 4) u (|A| @ |B|); pad rows are exact zeros; nothing else is written."""
    ops, L = _ops()
    vocabs, counts, D = [30000, 16384, 4096, 23, 512], [300, 257, 70, 33, 0], 100
    n_heads = len(vocabs)
    R, Rp, head, seg_start, seg_count, perm, tile_group = _segments(ops, counts, seed=95)
    y = randn(R, D, seed=96)
    yp = torch.zeros(Rp, D, device=DEV)
    live = perm >= 0
    yp[live] = y[perm[live].long()]
    ws = [randn(v, D, scale=D ** -0.5, seed=97 + i) for i, v in enumerate(vocabs)]
    ldl = ops.ru(max(vocabs), 64) + 64
    worst = {}
    # forward logits
    logits = torch.full((Rp, ldl), SENT, device=DEV)
    groups = ops.make_groups([dict(W=w, N=v, K=D, ldw=D) for w, v in zip(ws, vocabs)], DEV)
    ops.gemm_nt_grouped(yp, groups, tile_group, logits, max(vocabs), max_K=D)
    covered = torch.zeros(Rp, ldl, dtype=torch.bool, device=DEV)
    for h, (v, c) in enumerate(zip(vocabs, counts)):
        s, n = int(seg_start[h]), ops.ru(c, ops.SEG)
        covered[s:s + n, :v] = True
        if c:
            ref = yp[s:s + c].double() @ ws[h].double().t()
            worst[f"logits{v}"] = check(f"logits head {v}", logits[s:s + c, :v], ref, (D + 4) * U * (yp[s:s + c].abs().double() @ ws[h].abs().double().t()))
            assert float(logits[s + c:s + n, :v].abs().max() if n > c else 0.0) == 0.0
    assert bool((logits[~covered] == SENT).all())
    # dY = dL W_h (W read transposed: n = d with stride 1, k = vocab with stride D)
    dl = torch.zeros(Rp, ldl, device=DEV)
    for h, (v, c) in enumerate(zip(vocabs, counts)):
        s = int(seg_start[h])
        dl[s:s + c, :v] = randn(c, v, scale=v ** -0.5, seed=110 + h) if c else 0.0
    dy = torch.full((Rp, D + 3), SENT, device=DEV)
    gb = ops.make_groups([dict(W=w, N=D, K=v, ldw=D, transposed=1) for w, v in zip(ws, vocabs)], DEV)
    ops.gemm_nt_grouped(dl, gb, tile_group, dy, D)
    covered = torch.zeros_like(dy, dtype=torch.bool)
    for h, (v, c) in enumerate(zip(vocabs, counts)):
        s, n = int(seg_start[h]), ops.ru(c, ops.SEG)
        covered[s:s + n, :D] = True
        if c:
            ref = dl[s:s + c, :v].double() @ ws[h].double()
            worst[f"dy{v}"] = check(f"dY head {v}", dy[s:s + c, :D], ref, (v + 4) * U * (dl[s:s + c, :v].abs().double() @ ws[h].abs().double()))
            assert float(dy[s + c:s + n, :D].abs().max() if n > c else 0.0) == 0.0
    assert bool((dy[~covered] == SENT).all())
    # dW_h += dL^T Y over the head's own rows, into a non-zero fill; the row past V stays the sentinel
    fills = [randn(v, D, seed=120 + h) for h, v in enumerate(vocabs)]
    dws = [torch.cat([f, torch.full((1, D), SENT, device=DEV)]) for f in fills]
    gt = ops.make_groups([dict(out=dw, N=v) for dw, v in zip(dws, vocabs)], DEV)
    ops.gemm_tn_grouped(dl, yp, gt, seg_start, seg_count, n_heads, max(vocabs), Rp, D)
    for h, (v, c) in enumerate(zip(vocabs, counts)):
        s = int(seg_start[h])
        ref = fills[h].double() + (dl[s:s + c, :v].double().t() @ yp[s:s + c].double() if c else 0.0)
        tol = (c + 4) * U * (dl[s:s + c, :v].abs().double().t() @ yp[s:s + c].abs().double() if c else 0.0) + 2 * U * ref.abs()
        worst[f"dw{v}"] = check(f"dW head {v}", dws[h][:v], ref, tol)
        if c == 0:
            assert torch.equal(dws[h][:v], fills[h])
        assert bool((dws[h][v] == SENT).all())
    record("fp32_kernels.gemm_f32_grouped", worst_err_over_bound=worst)


# ------------------------------------------------------------------------------------------------
# attention
# ------------------------------------------------------------------------------------------------
NEG32 = -torch.finfo(torch.float32).max


def attn_masks(kind, B, Nq, Nk, seed):
    """Mask arguments of fm_attn_args and the (B, 1, Nq, Nk) blocked map.  Every kind but "none" has a fully blocked query row
    (keypad: all keys of sample 0; decoder: cs = 0 in row 0; causal + modalities / dense: row 0 blocked outright)."""
    g = torch.Generator().manual_seed(seed)
    out = dict(kpad=None, cs=None, modq=None, modk=None, dense=None, causal=False)
    qi, ki = torch.arange(Nq)[None, :, None], torch.arange(Nk)[None, None, :]
    if kind == "none":
        blk = torch.zeros(B, Nq, Nk, dtype=torch.bool)
    elif kind == "keypad":
        kp = torch.rand(B, Nk, generator=g) < 0.3
        kp[0] = True
        out["kpad"] = kp.to(DEV)
        blk = kp[:, None, :].expand(B, Nq, Nk)
    elif kind in ("decoder", "decoder_nomod"):
        cs = (torch.rand(B, Nq, generator=g) * (Nk + 1)).int().sort(-1).values
        cs[:, 0] = 0
        out["cs"] = cs.to(DEV)
        blk = ki >= cs[:, :, None]
        if kind == "decoder":
            mq = torch.randint(0, 3, (B, Nq), generator=g).short().sort(-1).values
            mk = torch.randint(0, 3, (B, Nk), generator=g).short().sort(-1).values
            out.update(modq=mq.to(DEV), modk=mk.to(DEV))
            blk = blk | (mq[:, :, None] != mk[:, None, :])
    elif kind in ("causal", "causal_mod"):
        out["causal"] = True
        blk = (ki > qi).expand(B, Nq, Nk)
        if kind == "causal_mod":
            mq = torch.randint(0, 3, (B, Nq), generator=g).short().sort(-1).values
            mq[:, 0] = 3                                         # row 0 matches no key's modality
            mk = torch.randint(0, 3, (B, Nk), generator=g).short().sort(-1).values
            out.update(modq=mq.to(DEV), modk=mk.to(DEV))
            blk = blk | (mq[:, :, None] != mk[:, None, :])
    elif kind == "dense":
        d = torch.rand(B, Nq, Nk, generator=g) < 0.4
        d[:, 0] = True
        out["dense"] = d.to(DEV)
        blk = d
    return out, blk[:, None].to(DEV)


ATTN_CASES = [("none", 1, 1, 5, 1), ("keypad", 2, 12, 40, 63), ("dense", 2, 16, 70, 64), ("decoder", 2, 1, 65, 65),
              ("decoder_nomod", 2, 12, 100, 256), ("causal", 1, 16, 200, 256), ("causal_mod", 2, 12, 64, 64), ("keypad", 1, 12, 130, 1030),
              ("dense", 1, 1, 33, 1030), ("none", 2, 16, 30, 65), ("decoder", 1, 12, 64, 1030)]


@pytest.mark.parametrize("zero_attn", [False, True])
@pytest.mark.parametrize("kind,B,H,Nq,Nk", ATTN_CASES)
def test_attention_f32(kind, B, H, Nq, Nk, zero_attn):
    """fm_attn_f32_fwd / _bwd against upstream's rule in float64 (masked_fill(-finfo(float32).max), softmax, optional zero logit
    (softmax1), gradients stopped at blocked scores); q / k / v are column views of packed qkv buffers (ld > H * 64), dK / dV
    accumulate into non-zero buffers.  Fully blocked rows come out uniform, or zero with zero_attn.  Each output is held to 2e-6
    relative (Frobenius) and to a first-order bound per element built from the same float64 quantities (x2 for second-order terms):
      scores  |ds_qk| <= 66 u scale (|q| . |k|)                      (64-term fmaf chain, scale)
      p       relative <= ds_k + max_j ds_j + (|s_k - m| + 2) u + (Nk / 64 + 12) u      (expf, row sum, 1 / sum)
      O       sum_k p_k eps_k |v_k| + (Nk + 2) u (p @ |V|)
      dP, D   65 u (|dO| @ |V|^T),  sum E_O |dO| + 8 u sum |O dO|
      dS      scale (p eps |dp - D| + p (E_dp + E_D)) + 3 u |dS|
      dQ, dK, dV   E_dS @ |K| + (Nk + 1) u (|dS| @ |K|),  E_dS^T @ |Q| + (Nq + 2) u (|dS|^T @ |Q| + |fill|),  (p eps)^T @ |dO| + ..."""
    ops, L = _ops()
    D = H * 64
    scale = 0.125
    qb = randn(B * Nq, 3 * D + 16, seed=201)
    kvb = randn(B * Nk, 3 * D + 16, seed=202)
    q, k, v = qb[:, :D], kvb[:, D:2 * D], kvb[:, 2 * D:3 * D]
    mk, blocked = attn_masks(kind, B, Nq, Nk, seed=203)
    kinds = dict(none=L.MASK_NONE, keypad=L.MASK_KEYPAD, decoder=L.MASK_DECODER, decoder_nomod=L.MASK_DECODER, causal=L.MASK_DECODER,
                 causal_mod=L.MASK_DECODER, dense=L.MASK_DENSE)
    kw = dict(mask_kind=kinds[kind], kpad=mk["kpad"], cs=mk["cs"], modq=mk["modq"], modk=mk["modk"], dense=mk["dense"], causal=mk["causal"],
              zero_attn=zero_attn)
    ob = torch.full((B * Nq, D + 64), SENT, device=DEV)
    o = ob[:, :D]
    ops.attn_fwd(q, k, v, o, B, H, Nq, Nk, scale, **kw)
    assert bool((ob[:, D:] == SENT).all())

    def heads(t, n):
        return t.double().reshape(B, n, H, 64).transpose(1, 2)

    qh, kh, vh = (heads(t, n).requires_grad_(True) for t, n in ((q, Nq), (k, Nk), (v, Nk)))
    s = (qh @ kh.transpose(-1, -2)) * scale
    s = s.masked_fill(blocked, NEG32)
    p = torch.softmax(F.pad(s, (0, 1)), -1)[..., :-1] if zero_attn else torch.softmax(s, -1)
    ref = p @ vh
    # per-element forward bound
    with torch.no_grad():
        sd = s.detach()
        live = ~blocked.expand_as(sd)
        Sabs = (qh.abs() @ kh.abs().transpose(-1, -2)) * scale
        ds = torch.where(live, 66 * U * Sabs, torch.zeros_like(Sabs))
        mx = sd.amax(-1, keepdim=True)
        if zero_attn:
            mx = mx.clamp(min=0.0)
        t = torch.where(live | ~live.any(-1, keepdim=True), (sd - mx).abs(), torch.zeros_like(sd))
        pd = p.detach()
        eps = ds + ds.amax(-1, keepdim=True) + (t + 2) * U + (Nk / 64 + 12) * U
        if zero_attn:
            eps = eps + (mx.abs() + 2) * U
        Vabs = vh.detach().abs()
        E_o = 2 * ((pd * eps) @ Vabs + (Nk + 2) * U * (pd @ Vabs))
    oh = heads(o, Nq)
    fwd_frob = frob(oh, ref.detach())
    assert fwd_frob <= 2e-6, fwd_frob
    worst = dict(o=check("O", oh, ref.detach(), E_o + 1e-300))
    fully = blocked[:, 0].all(-1)                                            # (B, Nq)
    assert bool(fully.any()) == (kind not in ("none", "causal"))
    if bool(fully.any()):
        rows = oh.transpose(1, 2)[fully]                                     # (n, H, 64)
        if zero_attn:
            assert float(rows.abs().max()) == 0.0
        else:
            want = vh.detach().mean(2, keepdim=True).expand(B, H, Nq, 64).transpose(1, 2)[fully]
            worst["uniform_rows"] = check("uniform rows", rows, want, 2 * (Nk + 8) * U * Vabs.mean(2, keepdim=True).expand(B, H, Nq, 64).transpose(1, 2)[fully])
    # backward: dO a column view, dq / dk / dv column views of packed gradient buffers; dK / dV start from a non-zero fill
    do = randn(B * Nq, D + 8, seed=204)[:, :D]
    ref.backward(heads(do, Nq))
    dqb = torch.full((B * Nq, D + 32), SENT, device=DEV)
    dkvb = torch.full((B * Nk, 2 * D + 32), SENT, device=DEV)
    dq, dk, dv = dqb[:, :D], dkvb[:, :D], dkvb[:, D:2 * D]
    rms = lambda x: float(x.pow(2).mean().sqrt()) + 1e-30
    fill_k = randn(B * Nk, D, scale=0.5 * rms(kh.grad), seed=205)
    fill_v = randn(B * Nk, D, scale=0.5 * rms(vh.grad), seed=206)
    dk.copy_(fill_k)
    dv.copy_(fill_v)
    a = ops._attn_args(q, k, v, o, B, H, Nq, Nk, scale, kw["mask_kind"], kw["kpad"], kw["cs"], kw["modq"], kw["modk"], kw["dense"], kw["causal"],
                       None, None, -1, zero_attn)
    a.dO, a.dQ, a.dK, a.dV = ops._p(do), ops._p(dq), ops._p(dk), ops._p(dv)
    a.lddo, a.lddq, a.lddk, a.lddv = do.stride(0), dq.stride(0), dk.stride(0), dv.stride(0)
    L.check(L.attn_f32_bwd(ops.C.byref(a), ops._stream()))               # direct: ops.attn_bwd zeroes dK / dV first
    assert bool((dqb[:, D:] == SENT).all()) and bool((dkvb[:, 2 * D:] == SENT).all())
    with torch.no_grad():
        dOh = heads(do, Nq)
        O = ref.detach()
        dp = dOh @ vh.detach().transpose(-1, -2)
        delta = (O * dOh).sum(-1, keepdim=True)
        E_dp = 65 * U * (dOh.abs() @ Vabs.transpose(-1, -2))
        E_delta = (E_o * dOh.abs()).sum(-1, keepdim=True) + 8 * U * (O * dOh).abs().sum(-1, keepdim=True)
        dS = torch.where(live, pd * (dp - delta) * scale, torch.zeros_like(pd))
        E_dS = torch.where(live, scale * (pd * eps * (dp - delta).abs() + pd * (E_dp + E_delta)) + 3 * U * dS.abs(), torch.zeros_like(pd))
        Kabs, Qabs, dOabs = kh.detach().abs(), qh.detach().abs(), dOh.abs()
        fk, fv = heads(fill_k, Nk), heads(fill_v, Nk)
        E_dq = 2 * (E_dS @ Kabs + (Nk + 1) * U * (dS.abs() @ Kabs))
        E_dk = 2 * (E_dS.transpose(-1, -2) @ Qabs + (Nq + 2) * U * (dS.abs().transpose(-1, -2) @ Qabs + fk.abs()))
        E_dv = 2 * ((pd * eps).transpose(-1, -2) @ dOabs + (Nq + 2) * U * (pd.transpose(-1, -2) @ dOabs + fv.abs()))
    got = dict(dq=heads(dq, Nq), dk=heads(dk, Nk), dv=heads(dv, Nk))
    want = dict(dq=qh.grad, dk=fk + kh.grad, dv=fv + vh.grad)
    frobs = {}
    for n, E in (("dq", E_dq), ("dk", E_dk), ("dv", E_dv)):
        worst[n] = check(n, got[n], want[n], E + 1e-300)
        base = {"dq": 0.0, "dk": fk, "dv": fv}[n]
        if float((want[n] - base).norm()) > 0:                               # (Nk = 1 without a mask: dS = 0 exactly, the bound above holds)
            frobs[n] = float((got[n] - want[n]).norm() / (want[n] - base).norm())
            assert frobs[n] <= 2e-6, (n, frobs[n])
    record("fp32_kernels.attention", kind=kind, B=B, H=H, Nq=Nq, Nk=Nk, zero_attn=zero_attn, o_frob=fwd_frob, grad_frob=frobs,
           worst_err_over_bound=worst)


# ------------------------------------------------------------------------------------------------
# norms
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [64, 384, 768, 1000, 1024, 2048])
def test_layernorm_bwd_f32(D):
    """fm_layernorm_bwd_f32 through ops.layernorm_bwd with fp32 dy: a dy_row_map with -1 entries (rows with no upstream gradient),
    dres, the second output dx2, and dw / db accumulating into non-zero buffers; mean / rstd from a float64 forward (rounded to fp32:
    the reference uses the same fp32 values).  Bound, derived for the kernel's sums (D / 256 sequential terms per thread, 8 tree
    levels) and roundings, x2:
      dx: rs ((D / 256 + 12) u (mean|g| + |xh| mean|g xh|) + 6 u (|g| + |m1| + |xh m2|)) + 2 u |dx|
      dw / db: (R + 4) u sum_r |dy xh| (|dy|) + 2 u |result|   (fp32 atomics over R rows, fill included)"""
    ops, L = _ops()
    R, Rdy = 300, 280
    x = padded(randn(R, D, scale=2.0, seed=301) + 0.7, D + 4)
    w = randn(D, scale=0.5, seed=302) + 1.0
    x64 = x.double()
    mu64 = x64.mean(-1)
    rs64 = 1.0 / torch.sqrt(((x64 - mu64[:, None]) ** 2).mean(-1) + 1e-6)
    mean, rstd = mu64.float(), rs64.float()
    mu, rs = mean.double()[:, None], rstd.double()[:, None]
    dyb = randn(Rdy, D + 8, seed=303)
    dy = dyb[:, :D]
    g = torch.Generator().manual_seed(304)
    rmap = torch.randint(0, Rdy, (R,), generator=g).int()
    rmap[torch.rand(R, generator=g) < 0.2] = -1
    rmap = rmap.to(DEV)
    dxb = torch.full((R, D + 16), SENT, device=DEV)
    dx = dxb[:, :D]
    dres = torch.full((R, D + 16), SENT, device=DEV)[:, :D]                # dres shares dx's row stride (lddx)
    dres.copy_(randn(R, D, seed=305))
    dx2b = torch.full((R, D + 40), SENT, device=DEV)
    dx2 = dx2b[:, :D]
    dw0, db0 = randn(D, seed=306), randn(D, seed=307)
    dw, db = dw0.clone(), db0.clone()
    ops.layernorm_bwd(dy, x, w, mean, rstd, dx, dres=dres, dx_bf16=dx2, dw=dw, db=db, dy_row_map=rmap)
    dyv = torch.where((rmap >= 0)[:, None], dy.double()[rmap.clamp(min=0).long()], torch.zeros(R, D, dtype=torch.float64, device=DEV))
    xh = (x64 - mu) * rs
    gg = dyv * w.double()
    m1, m2 = gg.mean(-1, keepdim=True), (gg * xh).mean(-1, keepdim=True)
    ref = rs * (gg - m1 - xh * m2) + dres.double()
    E = 2 * (rs * ((D / 256 + 12) * U * (gg.abs().mean(-1, keepdim=True) + xh.abs() * (gg * xh).abs().mean(-1, keepdim=True))
                   + 6 * U * (gg.abs() + m1.abs() + (xh * m2).abs())) + 2 * U * ref.abs())
    worst = dict(dx=check("dx", dx, ref, E))
    assert torch.equal(dx2, dx)
    assert torch.equal(dx[rmap < 0], dres[rmap < 0])
    assert bool((dxb[:, D:] == SENT).all()) and bool((dx2b[:, D:] == SENT).all())
    rdw, rdb = dw0.double() + (dyv * xh).sum(0), db0.double() + dyv.sum(0)
    worst["dw"] = check("dw", dw, rdw, 2 * ((R + 4) * U * ((dyv * xh).abs().sum(0) + dw0.double().abs()) + 2 * U * rdw.abs()))
    worst["db"] = check("db", db, rdb, 2 * ((R + 4) * U * (dyv.abs().sum(0) + db0.double().abs()) + 2 * U * rdb.abs()))
    record("fp32_kernels.layernorm_bwd", D=D, worst_err_over_bound=worst, dx_frob=frob(dx, ref))


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("R,H", [(1, 1), (1, 16), (3000, 12), (3000, 16), (37, 1)])
def test_headnorm_f32(R, H, bias):
    """fm_headnorm_f32_fwd / _bwd (per-head LayerNorm of q / k, 64 features, one wave per (row, head)) on the k column block of a
    packed qkv buffer, against float64; the backward uses the stats the forward wrote (as the engine does), dw / db accumulate.
    Bounds (wave_sum = 6 tree levels), x2:
      mean  7 u mean|x|;  rstd  (0.5 E_var / var + FN) rs  with E_var = (2 sum |dv| E_dv + 7 u sum dv^2) / 64 + 2 u var
      y     |w| (rs E_dv + |dv| E_rs) + 3 u |dv rs w| + u |y|;   dx as fm_layernorm_bwd_f32 with D = 64 (8 u sums)
      dw / db  (R H + 4) u sum |.| + 2 u |result|   (fp32 atomics over R H rows)"""
    ops, L = _ops()
    D = H * 64
    qkv = randn(R, 3 * D + 8, scale=1.5, seed=401) + 0.3
    x = qkv[:, D:2 * D]
    w = randn(64, scale=0.3, seed=402) + 1.0
    b = randn(64, seed=403) if bias else None
    yb = torch.full((R, 3 * D), SENT, device=DEV)
    y = yb[:, D:2 * D]
    stats = torch.zeros(R * H, 2, device=DEV)
    ops.headnorm_fwd(x, w, b, y, stats, R, H, 1e-6)
    keep = torch.ones_like(yb, dtype=torch.bool)
    keep[:, D:2 * D] = False
    assert bool((yb[keep] == SENT).all())
    xr = x.double().reshape(R * H, 64)
    mu = xr.mean(-1, keepdim=True)
    dv = xr - mu
    var = (dv * dv).mean(-1, keepdim=True)
    rs = 1.0 / torch.sqrt(var + 1e-6)
    w64 = w.double()
    ref = dv * rs * w64 + (b.double() if bias else 0.0)
    E_mu = 7 * U * xr.abs().mean(-1, keepdim=True)
    E_dv = E_mu + U * dv.abs()
    E_var = (2 * (dv.abs() * E_dv).sum(-1, keepdim=True) + 7 * U * (dv * dv).sum(-1, keepdim=True)) / 64 + 2 * U * var
    E_rs = (0.5 * E_var / (var + 1e-6) + FN) * rs
    E_y = 2 * (w64.abs() * (rs * E_dv + dv.abs() * E_rs) + 3 * U * (dv * rs * w64).abs() + U * ref.abs())
    worst = dict(y=check("y", y.reshape(R * H, 64), ref, E_y))
    worst["mean"] = check("stats mean", stats[:, 0:1], mu, 2 * E_mu)
    worst["rstd"] = check("stats rstd", stats[:, 1:2], rs, 2 * E_rs)
    # backward from the kernel's stats
    dy = randn(R, D + 8, seed=404)[:, :D]
    dxb = torch.full((R, 3 * D), SENT, device=DEV)
    dx = dxb[:, D:2 * D]
    dw0, db0 = randn(64, seed=405), randn(64, seed=406)
    dw, db = dw0.clone(), (db0.clone() if bias else None)
    ops.headnorm_bwd(dy, x, w, stats, dx, dw, db, R, H)
    assert bool((dxb[keep] == SENT).all())
    smu, srs = stats[:, 0:1].double(), stats[:, 1:2].double()
    xh = (xr - smu) * srs
    dyr = dy.double().reshape(R * H, 64)
    gg = dyr * w64
    m1, m2 = gg.mean(-1, keepdim=True), (gg * xh).mean(-1, keepdim=True)
    rdx = srs * (gg - m1 - xh * m2)
    E = 2 * (srs * (12 * U * (gg.abs().mean(-1, keepdim=True) + xh.abs() * (gg * xh).abs().mean(-1, keepdim=True))
                    + 6 * U * (gg.abs() + m1.abs() + (xh * m2).abs())) + 2 * U * rdx.abs())
    worst["dx"] = check("dx", dx.reshape(R * H, 64), rdx, E)
    rdw = dw0.double() + (dyr * xh).sum(0)
    worst["dw"] = check("dw", dw, rdw, 2 * ((R * H + 4) * U * ((dyr * xh).abs().sum(0) + dw0.double().abs()) + 2 * U * rdw.abs()))
    if bias:
        rdb = db0.double() + dyr.sum(0)
        worst["db"] = check("db", db, rdb, 2 * ((R * H + 4) * U * (dyr.abs().sum(0) + db0.double().abs()) + 2 * U * rdb.abs()))
    record("fp32_kernels.headnorm", R=R, H=H, bias=bias, worst_err_over_bound=worst)


# ------------------------------------------------------------------------------------------------
# activation backward, column sums
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,H,Hp", [(1, 1, 16), (37, 2730, 2752), (300, 170, 192)])
def test_swiglu_gelu_bwd_f32(R, H, Hp):
    """fm_swiglu_bwd_f32 and fm_gelu_bwd_f32 on pre-activations uniform in [-12, 12] (the sigmoid / erff tails), strided operands,
    Hp > H; outputs outside [0, H) and [Hp, Hp + H) untouched.  Bounds: FN |ref| (expf / erff / a handful of roundings) plus
      swiglu d/dg: 8 u |da u| sigma(g) (1 + |g|)   (1 - sigma(g) cancels for g > 0; 1 + g (1 - sigma) cancels near g = -1.28)
      gelu:        2^-21 |dh|                       (1 + erff cancels for x << 0; cdf + x pdf cancels near x = -0.75)"""
    ops, L = _ops()
    gub = uniform(R, 2 * Hp + 4, lo=-12.0, hi=12.0, seed=501)
    gu = gub[:, :2 * Hp]
    gu[:, Hp:] = randn(R, Hp, scale=2.0, seed=502)
    da = randn(R, H + 3, seed=503)[:, :H]
    dgub = torch.full((R, 2 * Hp + 8), SENT, device=DEV)
    dgu = dgub[:, :2 * Hp]
    ops.swiglu_bwd(da, gu, dgu, H, Hp)
    g, u, d = gu[:, :H].double(), gu[:, Hp:Hp + H].double(), da.double()
    sg = torch.sigmoid(g)
    rg, ru_ = d * u * sg * (1 + g * (1 - sg)), d * g * sg
    worst = dict(dg=check("swiglu dg", dgu[:, :H], rg, FN * rg.abs() + 8 * U * (d * u).abs() * sg * (1 + g.abs())))
    worst["du"] = check("swiglu du", dgu[:, Hp:Hp + H], ru_, FN * ru_.abs())
    keep = torch.ones_like(dgub, dtype=torch.bool)
    keep[:, :H] = False
    keep[:, Hp:Hp + H] = False
    assert bool((dgub[keep] == SENT).all())
    pre = uniform(R, Hp + 4, lo=-12.0, hi=12.0, seed=504)[:, :H]
    dh = randn(R, H + 1, seed=505)[:, :H]
    dpb = torch.full((R, Hp + 8), SENT, device=DEV)
    dpre = dpb[:, :H]
    ops.gelu_bwd(dh, pre, dpre, H, Hp)
    xx = pre.double()
    rgel = dh.double() * (0.5 * (1 + torch.erf(xx * 0.5 ** 0.5)) + xx * torch.exp(-0.5 * xx * xx) / (2 * torch.pi) ** 0.5)
    worst["gelu"] = check("gelu dpre", dpre, rgel, FN * rgel.abs() + 2.0 ** -21 * dh.double().abs())
    assert bool((dpb[:, H:] == SENT).all())
    record("fp32_kernels.act_bwd", R=R, H=H, worst_err_over_bound=worst)


@pytest.mark.parametrize("N", [1, 255, 257, 2730])
@pytest.mark.parametrize("R", [1, 63, 64, 65, 32768])
def test_colsum_f32(R, N):
    """fm_colsum_f32 (db += column sums; the grid's y extent is min(R, 64), so R = 63 / 64 / 65 switch its shape) into a non-zero db:
    (R + 2) u sum_r |dy| + 2 u |result| (partial sums + fp32 atomics)."""
    ops, L = _ops()
    dy = randn(R, N + 3, seed=600 + R)[:, :N]
    db0 = randn(N + 1, seed=601)
    db = db0.clone()
    ops.colsum(dy, db, N)
    ref = db0[:N].double() + dy.double().sum(0)
    w = check("colsum", db[:N], ref, (R + 2) * U * (dy.double().abs().sum(0) + db0[:N].double().abs()) + 2 * U * ref.abs())
    assert float(db[N]) == float(db0[N])
    record("fp32_kernels.colsum", R=R, N=N, worst_err_over_bound=w)


# ------------------------------------------------------------------------------------------------
# cross-entropy (fp32 logits)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss_type", ["mod", "token"])
def test_cross_entropy_f32(loss_type):
    """fm_cross_entropy_f32 on the production-vocabulary problem of tests/test_kernels_gpu.py (vocabularies 30000 / 16384 / 8192 / 4096 /
    23 and an empty head, confident / tied / shifted rows, targets in the first and last column), fp32 logits, against float64.
    Bound of lse per row, derived for ce_f32_kernel (max exact; t = x - m rounds by u |t|, expf 2 ulp; V / 256 sequential terms per
    thread + 8 tree levels; logf 2 ulp; m + log S rounds by u |lse|), x2:
        E_lse = 2 (sum_c e_c (|t_c| + 3) u / sum_c e_c + (V / 256 + 10) u + 2 u |log S| + 2 u |lse|)
    row_loss adds u |loss|; d(logits) = coef (expf(x - lse) - onehot): coef (p (E_lse + (|x - lse| + 3) u) + u |p - onehot|) + 4 u |ref|
    + (|coef| + 1) eta, eta = 2^-126: probabilities below the fp32 normal range (e^-100 in the confident rows) are flushed to zero.
    Each also within 2e-6 relative (Frobenius)."""
    ops, L = _ops()
    pb = segmented_ce_problem(torch.float32, seed=80)
    logits, n_heads, Rp = pb["logits"], pb["n_heads"], pb["Rp"]
    before = logits.clone()
    gs = 0.5
    ref = ce_reference(pb, loss_type, gs)
    lt = L.LOSS_MOD if loss_type == "mod" else L.LOSS_TOKEN
    row_loss, row_lse = torch.full((Rp,), 9.0, device=DEV), torch.full((Rp,), 9.0, device=DEV)
    head_loss, total = torch.zeros(n_heads, device=DEV), torch.zeros(1, device=DEV)
    args = (pb["perm"], pb["tile_group"], pb["tgt"], pb["vocab_t"], pb["seg_start"], pb["seg_count"], n_heads, max(CE_VOCABS))
    ops.cross_entropy(logits, *args, row_loss, row_lse, head_loss, total, loss_type=lt)
    assert torch.equal(logits, before)
    worst, frobs, E_lses = {}, {}, []
    for h, (v, c) in enumerate(zip(CE_VOCABS, CE_COUNTS)):
        s = int(pb["seg_start"][h])
        if c % ops.SEG:
            assert float(row_loss[s + c:s + ops.ru(c, ops.SEG)].abs().max()) == 0.0 and float(row_lse[s + c:s + ops.ru(c, ops.SEG)].abs().max()) == 0.0
        if c == 0:
            E_lses.append(None)
            assert float(head_loss[h]) == 0.0
            continue
        x, lse = pb["x64"][h], ref["lse"][h]
        m = x.amax(-1, keepdim=True)
        e = torch.exp(x - m)
        E_lse = 2 * ((e * ((x - m).abs() + 3)).sum(-1) * U / e.sum(-1) + (v / 256 + 10) * U + 2 * U * torch.log(e.sum(-1)).abs() + 2 * U * lse.abs())
        E_lses.append(E_lse)
        worst[f"lse{v}"] = check(f"row_lse {v}", row_lse[s:s + c], lse, E_lse)
        worst[f"loss{v}"] = check(f"row_loss {v}", row_loss[s:s + c], ref["loss"][h], E_lse + U * ref["loss"][h].abs())
        frobs[f"lse{v}"] = frob(row_lse[s:s + c], lse)
        assert frobs[f"lse{v}"] <= 2e-6
        hb = float(E_lse.mean()) + (c / 256 + 10) * U * ref["head_loss"][h]
        assert abs(float(head_loss[h]) - ref["head_loss"][h]) <= hb, (v, float(head_loss[h]), ref["head_loss"][h])
    hbs = [float(E.mean()) + (c / 256 + 10) * U * hl if E is not None else 0.0 for E, c, hl in zip(E_lses, CE_COUNTS, ref["head_loss"])]
    w = [1.0] * n_heads if loss_type == "mod" else ref["numel"]
    tb = sum(a * b for a, b in zip(hbs, w)) / sum(w) + 4 * (n_heads + 2) * U * abs(ref["total"])
    assert abs(float(total) - ref["total"]) <= tb, (float(total), ref["total"])
    ops.cross_entropy(logits, *args, row_loss, row_lse, head_loss, total, loss_type=lt, grad_scale=torch.tensor([gs], device=DEV), write_grad=True)
    covered = torch.zeros(Rp, pb["ldl"], dtype=torch.bool, device=DEV)
    for h, (v, c) in enumerate(zip(CE_VOCABS, CE_COUNTS)):
        s = int(pb["seg_start"][h])
        covered[s:s + ops.ru(c, ops.SEG), :v] = True
        if c == 0:
            continue
        x, lse = pb["x64"][h], ref["lse"][h][:, None]
        p_oh, t = ref["grads"][h]
        want = ref["coef"][h] * p_oh
        p = torch.exp(x - lse)
        E = abs(ref["coef"][h]) * (p * (E_lses[h][:, None] + ((x - lse).abs() + 3) * U) + U * p_oh.abs()) + 4 * U * want.abs() + ETA * (abs(ref["coef"][h]) + 1)
        worst[f"grad{v}"] = check(f"d(logits) {v}", logits[s:s + c, :v], want, E)
        frobs[f"grad{v}"] = frob(logits[s:s + c, :v], want)
        assert frobs[f"grad{v}"] <= 2e-6
        assert float(logits[s + c:s + ops.ru(c, ops.SEG), :v].abs().max() if c % ops.SEG else 0.0) == 0.0     # pad rows
    assert torch.equal(logits[~covered], before[~covered])                    # columns >= V and rows outside the segments: untouched
    record(f"fp32_kernels.cross_entropy_f32.{loss_type}", worst_err_over_bound=worst, frob=frobs, total_err=abs(float(total) - ref["total"]))
