"""Thin torch-tensor front end over the C ABI: pointer extraction, shape checks, stream plumbing.
torch is used here for device memory and streams only; every computation is a HIP kernel."""
import contextlib
import ctypes as C
import threading
from typing import Optional

import torch

from . import _lib as L

# Optional per-launch timing (bench.py): an object with .launch(name, flops, bytes) -> context manager
# that brackets the launch with events on the CURRENT stream (the one the kernels are enqueued on).
_PROFILER = None


def set_profiler(p):
    global _PROFILER
    _PROFILER = p


class _Null:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


_NULL = _Null()


def _prof(name, flops=0.0, nbytes=0.0, tag=""):
    return _NULL if _PROFILER is None else _PROFILER.launch(name, flops, nbytes, tag)


def _timed(name):
    """Decorator: the wrapped launch shows up as family ``name`` in bench.py's per-kernel breakdown (events only while a profiler is set)."""
    def deco(fn):
        import functools

        @functools.wraps(fn)
        def wrapped(*a, **k):
            if _PROFILER is None:
                return fn(*a, **k)
            with _PROFILER.launch(name, 0.0, 0.0, ""):
                return fn(*a, **k)
        return wrapped
    return deco


BK = 64          # reduction granularity of the GEMMs (zero padded)
SEG = 256        # row-segment alignment of the grouped head GEMMs (FM_SEG_ROWS)


def ru(x: int, m: int) -> int:
    return (x + m - 1) // m * m


def _p(t: Optional[torch.Tensor]):
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("libfourm_hip ops need device tensors (no CPU fallback exists)")
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ld(t: torch.Tensor) -> int:
    assert t.dim() == 2 and t.stride(1) == 1, "2-D row-major tensor expected"
    return t.stride(0)


# ---------------------------------------------------------------------------------------------
# GEMM
# ---------------------------------------------------------------------------------------------
# split-K scratch of fm_gemm_nt (fm_gemm_nt_args.splitk_ws): one fp32 buffer per (device, stream, graph being captured), shared by the
# launches of that stream in stream order - never across streams or between two captured graphs, which may run at the same time
SPLITK_MAX_OUT = 128 * 128 * 128          # outputs of up to 128 tiles of 128 x 128 can be split (the kernel decides)
_SPLITK_WS = {}


SCRATCH_TAG = None          # set while a hipGraph is being captured: scratch allocated then belongs to THAT graph (torch captures every graph on the same
                            # side stream, so the stream alone would hand one graph's scratch to the next - and two graphs may replay concurrently)


def _splitk_ws(device):
    key = (device, torch.cuda.current_stream(device).cuda_stream, SCRATCH_TAG)          # (launches on different streams must not share partial tiles)
    t = _SPLITK_WS.get(key)
    if t is None:
        t = _SPLITK_WS[key] = torch.empty(16 * SPLITK_MAX_OUT, dtype=torch.float32, device=device)      # 128 MB: 16 slices of the largest output
    return t


_TILING = threading.local()


@contextlib.contextmanager
def fixed_tiling(on=True):
    """Inside the block every dense gemm_nt of this thread runs on ONE kernel and tile configuration (fm_gemm_nt_args.fixed_tiling): a row of
    the result then depends on that row of x alone, bit for bit, whatever the number of rows - slower on large shapes, batch-invariant."""
    prev = getattr(_TILING, "fixed", False)
    _TILING.fixed = bool(on) or prev
    try:
        yield
    finally:
        _TILING.fixed = prev


def gemm_nt(x, w, out, *, epilogue=L.EPI_BF16, bias=None, res=None, w2=None, bias2=None, out2=None, Hp=0, N=None, K=None, M=None, conv=None):
    """out[m][n] = sum_k x[m][k] w[n][k] (+ epilogue).  x: bf16 (M, >=K); w: bf16 (N, >=K).
    fp32 operands select the verification kernel (any strides for w).
    conv = dict(C, H, W, Ho, Wo, stride, up): x is a (B, H >> up, W >> up, C) feature map in rows and the launch is the 3 x 3 convolution
    with the (N, 9 C) weight rows w (taps outermost) as an implicit GEMM (fm_gemm_nt_args.conv_*); M = B Ho Wo and K = 9 C must be given."""
    if x.dtype == torch.float32:
        return _gemm_f32(x, w, out, epilogue=epilogue, bias=bias, res=res, w2=w2, bias2=bias2, out2=out2, Hp=Hp, N=N, K=K, M=M)
    a = L.GemmNTArgs()
    a.W, a.W2, a.X, a.out, a.out2 = _p(w), _p(w2), _p(x), _p(out), _p(out2)
    a.res, a.bias, a.bias2 = _p(res), _p(bias), _p(bias2)
    a.M = x.shape[0] if M is None else M
    a.N = w.shape[0] if N is None else N
    a.K = w.shape[1] if K is None else K
    a.ldw, a.ldx, a.ldo = _ld(w), _ld(x), _ld(out)
    a.ldo2 = _ld(out2) if out2 is not None else 0
    a.ldr = _ld(res) if res is not None else 0
    a.Hp, a.epilogue = Hp, epilogue
    if conv is not None:
        a.conv_C, a.conv_H, a.conv_W, a.conv_Ho, a.conv_Wo = conv["C"], conv["H"], conv["W"], conv["Ho"], conv["Wo"]
        a.conv_stride, a.conv_up = conv.get("stride", 1), conv.get("up", 0)
    if conv is None and getattr(_TILING, "fixed", False):
        a.fixed_tiling = 1
    elif epilogue == L.EPI_BF16 and a.M * a.N <= SPLITK_MAX_OUT and a.K >= 512:       # (only launches that can be split need the scratch)
        ws = _splitk_ws(x.device)
        a.splitk_ws, a.splitk_ws_bytes = ws.data_ptr(), ws.numel() * 4
    two = 2 if epilogue == L.EPI_SWIGLU else 1
    nbytes = 2.0 * a.K * (a.M + two * a.N) + a.M * a.N * two * out.element_size()        # operands once + output once
    nbytes += (a.M * a.N * 4.0 if res is not None and epilogue in (L.EPI_RESIDUAL, L.EPI_F32) else 0.0) + (a.M * a.N * 4.0 if out2 is not None else 0.0)
    with _prof(f"gemm_nt/epi{epilogue}", 2.0 * a.M * a.N * a.K * two, nbytes, tag=f"M{a.M} N{a.N} K{a.K}"):
        L.check(L.gemm_nt(C.byref(a), _stream()))
    return out


def _gemm_f32(x, w, out, *, epilogue=L.EPI_BF16, bias=None, res=None, w2=None, bias2=None, out2=None, Hp=0, N=None, K=None, M=None,
              accumulate=False):
    assert w.dtype == torch.float32 and out.dtype == torch.float32 and x.stride(1) == 1 and out.stride(1) == 1
    a = L.GemmF32Args()
    a.X, a.W, a.W2, a.out, a.out2, a.res, a.bias, a.bias2 = _p(x), _p(w), _p(w2), _p(out), _p(out2), _p(res), _p(bias), _p(bias2)
    a.M = x.shape[0] if M is None else M
    a.N = w.shape[0] if N is None else N
    a.K = min(w.shape[1] if K is None else K, w.shape[1])          # padded reduction widths (Hp) stop at the weight's own width
    a.sxm, a.sxk, a.swn, a.swk = x.stride(0), 1, w.stride(0), w.stride(1)
    if w2 is not None:
        assert w2.stride() == w.stride()
    a.ldo, a.ldo2, a.ldr = out.stride(0), out2.stride(0) if out2 is not None else 0, res.stride(0) if res is not None else 0
    a.Hp, a.epilogue, a.accumulate = Hp, epilogue, 1 if accumulate else 0
    with _prof("gemm_f32", 2.0 * a.M * a.N * a.K * (2 if epilogue == L.EPI_SWIGLU else 1), 4.0 * (a.K * (a.M + a.N) + a.M * a.N), tag=f"M{a.M} N{a.N} K{a.K}"):
        L.check(L.gemm_f32(C.byref(a), _stream()))
    return out


@_timed("heads_gemm_nt (logits, dY)")
def gemm_nt_grouped(x, groups, tile_group, out, max_N, M=None, max_K=0):
    if x.dtype == torch.float32:
        a = L.GemmF32Args()
        a.X, a.out, a.groups, a.tile_group = _p(x), _p(out), _p(groups), _p(tile_group)
        a.M, a.N, a.max_N, a.seg_rows = (x.shape[0] if M is None else M), max_N, max_N, SEG
        a.sxm, a.sxk, a.ldo, a.epilogue = x.stride(0), 1, out.stride(0), L.EPI_BF16
        L.check(L.gemm_f32(C.byref(a), _stream()))
        return out
    a = L.GemmNTArgs()
    a.X, a.out = _p(x), _p(out)
    a.M = x.shape[0] if M is None else M
    a.K = max_K
    a.ldx, a.ldo = _ld(x), _ld(out)
    a.epilogue = L.EPI_BF16
    a.groups, a.tile_group, a.max_N = _p(groups), _p(tile_group), max_N
    L.check(L.gemm_nt(C.byref(a), _stream()))
    return out


def heads_dense_ok(ws, vocabs, out):
    """One dense fm_gemm_nt launch per head (row range read from device memory) can replace the grouped logits GEMM: bf16, every
    vocabulary a multiple of 8, whole-line output rows (the staged epilogue of gemm_nt3)."""
    return (out.dtype == torch.bfloat16 and all(v % 8 == 0 for v in vocabs) and all(w.dtype == torch.bfloat16 and w.shape[1] % 64 == 0 for w in ws)
            and _ld(out) % 64 == 0 and out.data_ptr() % 128 == 0)


@_timed("heads_gemm_nt (logits, dY)")
def gemm_nt_heads(x, ws, vocabs, seg_start, seg_count, out, K):
    """The logits of every modality head as ONE DENSE launch per head on the lock-step kernel (csrc/gemm_nt3.hip, DEVM): head h covers rows
    [seg_start[h], seg_start[h] + roundup(seg_count[h], SEG)) of x / out - read by the kernel from device memory, so the step stays
    capturable - against its own (V_h, K) weight.  Same outputs as gemm_nt_grouped on the rows of the segments (pad rows of x are zero)."""
    for h, (w, v) in enumerate(zip(ws, vocabs)):
        a = L.GemmNTArgs()
        a.W, a.X, a.out = _p(w), _p(x), _p(out)
        a.M, a.N, a.K = x.shape[0], v, K
        a.ldw, a.ldx, a.ldo = _ld(w), _ld(x), _ld(out)
        a.epilogue = L.EPI_BF16
        a.m_dev, a.row0_dev = seg_count.data_ptr() + 4 * h, seg_start.data_ptr() + 4 * h
        L.check(L.gemm_nt(C.byref(a), _stream()))
    return out


def gemm_tn(a_mat, b_mat, out, *, N=None, K=None, R=None, splits=0, force_tr=-1, a_cols=0, b_cols=0):
    """out[n][k] += sum_r a[r][n] b[r][k]; out fp32 (N, >=K)."""
    if a_mat.dtype == torch.float32:        # verification kernel: X := a^T, W := b^T through strides, accumulate
        g = L.GemmF32Args()
        g.X, g.W, g.out = _p(a_mat), _p(b_mat), _p(out)
        g.M = a_mat.shape[1] if N is None else N
        g.N = b_mat.shape[1] if K is None else K
        g.K = a_mat.shape[0] if R is None else R
        g.sxm, g.sxk, g.swn, g.swk = 1, a_mat.stride(0), 1, b_mat.stride(0)
        g.ldo, g.epilogue, g.accumulate = _ld(out), L.EPI_BF16, 1
        L.check(L.gemm_f32(C.byref(g), _stream()))
        return out
    a = L.GemmTNArgs()
    a.A, a.B, a.out = _p(a_mat), _p(b_mat), _p(out)
    a.R = a_mat.shape[0] if R is None else R
    a.N = a_mat.shape[1] if N is None else N
    a.K = b_mat.shape[1] if K is None else K
    a.lda, a.ldb, a.ldo = _ld(a_mat), _ld(b_mat), _ld(out)
    a.a_cols = a_cols or a_mat.shape[1]
    a.b_cols = b_cols or b_mat.shape[1]
    a.splits, a.force_tr = splits, force_tr
    with _prof("gemm_tn", 2.0 * a.R * a.N * a.K, 2.0 * a.R * (a.N + a.K) + 4.0 * a.N * a.K, tag=f"R{a.R} N{a.N} K{a.K}"):
        L.check(L.gemm_tn(C.byref(a), _stream()))
    return out


def gemm_tn_multi(jobs):
    """One launch for a list of dense weight-gradient GEMMs: jobs = [(a_mat, b_mat, out, N, K, R), ...] with gemm_tn's meaning
    per entry (all dW of a transformer layer; csrc/gemm.hip gemm_tn_multi_kernel)."""
    if not jobs:
        return
    if jobs[0][0].dtype == torch.float32:
        for a_mat, b_mat, out, N, K, R in jobs:
            gemm_tn(a_mat, b_mat, out, N=N, K=K, R=R)
        return
    for lo in range(0, len(jobs), L.TN_MAX_JOBS):
        part = jobs[lo:lo + L.TN_MAX_JOBS]
        arr = (L.GemmTNJob * len(part))()
        flops = 0.0
        for j, (a_mat, b_mat, out, N, K, R) in zip(arr, part):
            j.A, j.B, j.out = _p(a_mat), _p(b_mat), _p(out)
            j.R, j.N, j.K = R, N, K
            j.lda, j.ldb, j.ldo = _ld(a_mat), _ld(b_mat), _ld(out)
            j.a_cols, j.b_cols = a_mat.shape[1], b_mat.shape[1]
            flops += 2.0 * R * N * K
        with _prof("gemm_tn_multi", flops, 0.0, tag=f"jobs{len(part)} R{part[0][5]}"):
            L.check(L.gemm_tn_multi(arr, len(part), _stream()))


@_timed("heads_gemm_tn (dW)")
def gemm_tn_grouped(a_mat, b_mat, groups, seg_start, seg_count, n_groups, max_N, max_R, K, *, splits=0, force_tr=-1):
    if a_mat.dtype == torch.float32:
        g = L.GemmF32Args()
        g.X, g.W, g.groups, g.seg_start, g.seg_count = _p(a_mat), _p(b_mat), _p(groups), _p(seg_start), _p(seg_count)
        g.N, g.max_N, g.n_groups = K, max_N, n_groups
        g.sxm, g.sxk, g.swn, g.swk = 1, a_mat.stride(0), 1, b_mat.stride(0)
        g.ldo, g.epilogue, g.accumulate = K, L.EPI_BF16, 1
        L.check(L.gemm_f32(C.byref(g), _stream()))
        return
    a = L.GemmTNArgs()
    a.A, a.B = _p(a_mat), _p(b_mat)
    a.K = K
    a.lda, a.ldb, a.ldo = _ld(a_mat), _ld(b_mat), K
    a.a_cols, a.b_cols = a_mat.shape[1], b_mat.shape[1]
    a.splits, a.force_tr = splits, force_tr
    a.groups, a.seg_start, a.seg_count = _p(groups), _p(seg_start), _p(seg_count)
    a.n_groups, a.max_N, a.max_R = n_groups, max_N, max_R
    L.check(L.gemm_tn(C.byref(a), _stream()))


def make_groups(entries, device):
    """entries: list of dicts(W=tensor|None, out=tensor|None, N, K, ldw) -> device byte tensor of fm_gemm_group."""
    arr = (L.GemmGroup * len(entries))()
    for i, e in enumerate(entries):
        arr[i].W = e["W"].data_ptr() if e.get("W") is not None else None
        arr[i].out = e["out"].data_ptr() if e.get("out") is not None else None
        arr[i].N, arr[i].K, arr[i].ldw = e["N"], e.get("K", 0), e.get("ldw", 0)
        arr[i].pad_ = e.get("transposed", 0)         # fp32 path: W is read as W[k][n] (stride ldw along k)
    host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
    return host.to(device)


# ---------------------------------------------------------------------------------------------
# LayerNorm
# ---------------------------------------------------------------------------------------------
def layernorm_fwd(x, w, b, y, mean=None, rstd=None, row_map=None, eps=1e-6, R=None, delta=None, x_out=None, gamma=None):
    """y = LN(x) - or, with ``delta`` (bf16) and ``x_out`` (f32): x_out = x + delta, y = LN(x_out) in one pass.  ``gamma`` (f32 (D), with
    delta): LayerScale, x_out = x + gamma * delta with the product and the sum rounded separately (fm_layernorm_fwd_res_ls)."""
    R = x.shape[0] if R is None else R
    if gamma is not None:
        assert delta is not None and delta.dtype == torch.bfloat16 and gamma.dtype == torch.float32 and gamma.numel() == w.numel()
        with _prof("layernorm_fwd", 0.0, R * w.numel() * (10 + y.element_size())):
            L.check(L.layernorm_fwd_res_ls(_p(x), _ld(x), _p(delta), _ld(delta), _p(gamma), _p(x_out), _ld(x_out), _p(w), _p(b), _p(y), _ld(y),
                                           1 if y.dtype == torch.float32 else 0, _p(mean), _p(rstd), _p(row_map), R, w.numel(), eps, _stream()))
        return y
    if delta is not None:
        with _prof("layernorm_fwd", 0.0, R * w.numel() * (10 + y.element_size())):
            L.check(L.layernorm_fwd_res(_p(x), _ld(x), _p(delta), _ld(delta), _p(x_out), _ld(x_out), _p(w), _p(b), _p(y), _ld(y),
                                        1 if y.dtype == torch.float32 else 0, _p(mean), _p(rstd), _p(row_map), R, w.numel(), eps, _stream()))
        return y
    with _prof("layernorm_fwd", 0.0, R * w.numel() * (4 + y.element_size())):
        return _ln_fwd(x, w, b, y, mean, rstd, row_map, eps, R)


def _ln_fwd(x, w, b, y, mean, rstd, row_map, eps, R):
    L.check(L.layernorm_fwd(_p(x), _ld(x), _p(w), _p(b), _p(y), _ld(y), 1 if y.dtype == torch.float32 else 0,
                            _p(mean), _p(rstd), _p(row_map), R, w.numel(), eps, _stream()))
    return y


def layernorm_bwd(dy, x, w, mean, rstd, dx, *, dres=None, dx_bf16=None, dw=None, db=None, dy_row_map=None, R=None, h=None):
    """``h`` (optional): the bf16 output the forward norm wrote (bias-free norm, same row order as x) - x_hat is then rebuilt from it
    instead of from the fp32 ``x`` (fm_layernorm_bwd_h: 14 instead of 16 bytes per element)."""
    R = x.shape[0] if R is None else R
    if h is not None and dy.dtype != torch.float32 and db is None and dy_row_map is None:
        with _prof("layernorm_bwd", 0.0, R * w.numel() * (2 + 2 + 4 + 4 + (2 if dx_bf16 is not None else 0))):
            L.check(L.layernorm_bwd_h(_p(dy), _ld(dy), _p(h), _ld(h), _p(x), _ld(x), _p(w), _p(mean), _p(rstd), _p(dres), _p(dx), _ld(dx),
                                      _p(dx_bf16), _ld(dx_bf16) if dx_bf16 is not None else 0, _p(dw), R, w.numel(), _stream()))
        return dx
    with _prof("layernorm_bwd", 0.0, R * w.numel() * (2 + 4 + 4 + 4 + (2 if dx_bf16 is not None else 0))):
        return _ln_bwd(dy, x, w, mean, rstd, dx, dres, dx_bf16, dw, db, dy_row_map, R)


def _ln_bwd(dy, x, w, mean, rstd, dx, dres, dx_bf16, dw, db, dy_row_map, R):
    if dy.dtype == torch.float32:
        L.check(L.layernorm_bwd_f32(_p(dy), _ld(dy), _p(dy_row_map), _p(x), _ld(x), _p(w), _p(mean), _p(rstd), _p(dres), _p(dx), _ld(dx),
                                    _p(dx_bf16), _ld(dx_bf16) if dx_bf16 is not None else 0, _p(dw), _p(db), R, w.numel(), _stream()))
        return dx
    L.check(L.layernorm_bwd(_p(dy), _ld(dy), _p(dy_row_map), _p(x), _ld(x), _p(w), _p(mean), _p(rstd), _p(dres), _p(dx), _ld(dx),
                            _p(dx_bf16), _ld(dx_bf16) if dx_bf16 is not None else 0, _p(dw), _p(db), R, w.numel(), _stream()))
    return dx


@_timed("headnorm")
def headnorm_fwd(x, w, b, y, stats, R, H, eps):
    """Per-head (64 features) LayerNorm of the q / k column block ``x`` -> ``y`` (both bf16 2-D views)."""
    if x.dtype == torch.float32:
        return L.check(L.headnorm_f32_fwd(_p(x), _ld(x), _p(w), _p(b), _p(y), _ld(y), _p(stats), R, H, eps, _stream()))
    L.check(L.headnorm_fwd(_p(x), _ld(x), _p(w), _p(b), _p(y), _ld(y), _p(stats), R, H, eps, _stream()))


@_timed("headnorm")
def headnorm_bwd(dy, x, w, stats, dx, dw, db, R, H):
    if x.dtype == torch.float32:
        return L.check(L.headnorm_f32_bwd(_p(dy), _ld(dy), _p(x), _ld(x), _p(w), _p(stats), _p(dx), _ld(dx), _p(dw), _p(db), R, H, _stream()))
    L.check(L.headnorm_bwd(_p(dy), _ld(dy), _p(x), _ld(x), _p(w), _p(stats), _p(dx), _ld(dx), _p(dw), _p(db), R, H, _stream()))


# ---------------------------------------------------------------------------------------------
# attention
# ---------------------------------------------------------------------------------------------
def _attn_args(q, k, v, o, B, H, Nq, Nk, scale, mask_kind, kpad, cs, modq, modk, dense, causal, stat_m, stat_l, force_tr, zero_attn=False):
    a = L.AttnArgs()
    a.Q, a.K, a.V, a.O = _p(q), _p(k), _p(v), _p(o)
    a.ldq, a.ldk, a.ldv, a.ldo = q.stride(0), k.stride(0), v.stride(0), o.stride(0)
    a.B, a.H, a.Nq, a.Nk, a.head_dim, a.mask_kind = B, H, Nq, Nk, 64, mask_kind
    a.scale, a.causal = scale, 1 if causal else 0
    a.kpad, a.cs, a.modq, a.modk, a.dense = _p(kpad), _p(cs), _p(modq), _p(modk), _p(dense)
    a.stat_m, a.stat_l = _p(stat_m), _p(stat_l)
    a.force_tr, a.zero_attn = force_tr, 1 if zero_attn else 0
    return a


def attn_fwd(q, k, v, o, B, H, Nq, Nk, scale, *, mask_kind=L.MASK_NONE, kpad=None, cs=None, modq=None, modk=None, dense=None,
             causal=False, stat_m=None, stat_l=None, force_tr=-1, kv_batch_rows=0, zero_attn=False):
    """q/k/v/o: 2-D bf16 views whose row t of sample b is row b*N + t; head h occupies columns [64h, 64h+64).
    kv_batch_rows > Nk: k / v are views of a K/V cache whose sample b starts at row b * kv_batch_rows."""
    a = _attn_args(q, k, v, o, B, H, Nq, Nk, scale, mask_kind, kpad, cs, modq, modk, dense, causal, stat_m, stat_l, force_tr, zero_attn)
    a.kv_batch_rows = kv_batch_rows
    if q.dtype == torch.float32:
        L.check(L.attn_f32_fwd(C.byref(a), _stream()))
        return o
    with _prof("attn_fwd", 4.0 * B * H * Nq * Nk * 64):
        L.check(L.attn_fwd(C.byref(a), _stream()))
    return o


@_timed("attn_decode")
def attn_decode(q, k, v, o, B, H, Nk, scale, *, kv_batch_rows=0, k_new_row=-1, q_norm=None, k_norm=None, eps=1e-6, kpad=None, zero_attn=False):
    """One query row per sample against the first Nk rows of its keys / values (fm_attn_decode): q (B, >= 64 H), k / v 2-D views whose
    sample b starts at row b * kv_batch_rows, o (>= B, >= 64 H); all four bf16 or all four fp32.  q_norm / k_norm: (weight, bias | None)
    of the per-head LayerNorm; with q_norm given and k_new_row >= 0 the key in that row of every sample is normalised IN PLACE."""
    a = L.AttnDecodeArgs()
    a.q, a.k, a.v, a.o = _p(q), _p(k), _p(v), _p(o)
    if not (q.dtype == k.dtype == v.dtype == o.dtype) or q.dtype not in (torch.bfloat16, torch.float32):
        raise TypeError("attn_decode: q, k, v, o must share one of bf16 / fp32")
    for w in (q_norm or ()) + (k_norm or ()):
        if w is not None and (w.dtype != torch.float32 or w.numel() != 64 or not w.is_contiguous()):
            raise TypeError("attn_decode: norm vectors are contiguous fp32 (64)")
    a.q_w, a.q_b = (_p(q_norm[0]), _p(q_norm[1])) if q_norm is not None else (None, None)
    a.k_w, a.k_b = (_p(k_norm[0]), _p(k_norm[1])) if k_norm is not None else (None, None)
    if kpad is not None and (kpad.dtype not in (torch.bool, torch.uint8) or kpad.shape != (B, Nk) or not kpad.is_contiguous()):
        raise TypeError("attn_decode: kpad is a contiguous (B, Nk) bool / uint8 tensor")
    a.kpad = _p(kpad)
    a.ldq, a.ldk, a.ldv, a.ldo = _ld(q), _ld(k), _ld(v), _ld(o)
    a.B, a.H, a.Nk, a.kv_batch_rows, a.k_new_row = B, H, Nk, kv_batch_rows, k_new_row
    a.is_f32, a.zero_attn, a.scale, a.eps = int(q.dtype == torch.float32), 1 if zero_attn else 0, scale, eps
    L.check(L.attn_decode(C.byref(a), _stream()))
    return o


def attn_bwd(q, k, v, o, do, dq, dk, dv, B, H, Nq, Nk, scale, stat_m, stat_l, *, mask_kind=L.MASK_NONE, kpad=None, cs=None,
             modq=None, modk=None, dense=None, causal=False, force_tr=-1, zero_attn=False):
    a = _attn_args(q, k, v, o, B, H, Nq, Nk, scale, mask_kind, kpad, cs, modq, modk, dense, causal, stat_m, stat_l, force_tr, zero_attn)
    a.dO, a.dQ, a.dK, a.dV = _p(do), _p(dq), _p(dk), _p(dv)
    a.lddo, a.lddq, a.lddk, a.lddv = do.stride(0), dq.stride(0), dk.stride(0), dv.stride(0)
    if q.dtype == torch.float32:
        dk.zero_(); dv.zero_()                      # the verification kernel ACCUMULATES dK / dV (in query order with stat_m / stat_l as scratch, else by atomics)
        L.check(L.attn_f32_bwd(C.byref(a), _stream()))
        return
    with _prof("attn_bwd", 10.0 * B * H * Nq * Nk * 64):
        L.check(L.attn_bwd(C.byref(a), _stream()))


# ---------------------------------------------------------------------------------------------
# heads / loss
# ---------------------------------------------------------------------------------------------
def padded_rows(R: int, n_heads: int) -> int:
    return ru(R, SEG) + SEG * (n_heads - 1)


@_timed("heads_misc")
def segment_rows(head_of_row, n_heads, seg_start, seg_count, perm, row_to_padded, tile_group):
    L.check(L.segment_rows(_p(head_of_row), head_of_row.numel(), n_heads, _p(seg_start), _p(seg_count), _p(perm),
                           _p(row_to_padded), _p(tile_group), perm.numel(), _stream()))


@_timed("heads_misc")
def gather_rows(src, perm, dst, D):
    L.check(L.gather_rows(_p(src), _ld(src), _p(perm), _p(dst), _ld(dst), perm.numel(), D, _stream()))


@_timed("cross_entropy")
def cross_entropy(logits, perm, tile_group, target_ids, vocab, seg_start, seg_count, n_heads, max_vocab, row_loss, row_lse, head_loss,
                  total_loss, *, loss_type=L.LOSS_MOD, grad_scale=None, write_grad=False):
    """write_grad=False: forward (losses + row_lse); write_grad=True: in-place d(logits) from the saved row_lse."""
    fn = L.cross_entropy_f32 if logits.dtype == torch.float32 else L.cross_entropy
    L.check(fn(_p(logits), _ld(logits), _p(perm), _p(tile_group), _p(target_ids), _p(vocab), _p(seg_start),
                            _p(seg_count), _p(grad_scale), loss_type, n_heads, perm.numel(), max_vocab, _p(row_loss), _p(row_lse),
                            _p(head_loss), _p(total_loss), 1 if write_grad else 0, _stream()))


# ---------------------------------------------------------------------------------------------
# element-wise
# ---------------------------------------------------------------------------------------------
@_timed("swiglu_bwd")
def swiglu_bwd(da, gu, dgu, H, Hp, R=None):
    if da.dtype == torch.float32:
        return L.check(L.swiglu_bwd_f32(_p(da), _ld(da), _p(gu), _ld(gu), _p(dgu), _ld(dgu), da.shape[0] if R is None else R, H, Hp, _stream()))
    L.check(L.swiglu_bwd(_p(da), _ld(da), _p(gu), _ld(gu), _p(dgu), _ld(dgu), da.shape[0] if R is None else R, H, Hp, _stream()))


@_timed("gelu_bwd")
def gelu_bwd(dh, pre, dpre, H, Hp, R=None):
    if dh.dtype == torch.float32:
        return L.check(L.gelu_bwd_f32(_p(dh), _ld(dh), _p(pre), _ld(pre), _p(dpre), _ld(dpre), dh.shape[0] if R is None else R, H, _stream()))
    L.check(L.gelu_bwd(_p(dh), _ld(dh), _p(pre), _ld(pre), _p(dpre), _ld(dpre), dh.shape[0] if R is None else R, H, Hp, _stream()))


@_timed("gelu_bwd")
def quick_gelu_bwd(da, pre, dpre, H, Hp, R=None):
    """dpre = da * d/du (u sigmoid(1.702 u)) at the saved pre-activation u (CLIP's MLP)."""
    R = da.shape[0] if R is None else R
    if da.dtype == torch.float32:
        return L.check(L.quick_gelu_bwd_f32(_p(da), _ld(da), _p(pre), _ld(pre), _p(dpre), _ld(dpre), R, H, _stream()))
    L.check(L.quick_gelu_bwd(_p(da), _ld(da), _p(pre), _ld(pre), _p(dpre), _ld(dpre), R, H, Hp, _stream()))


def tap_add(g, dtap, g_bf=None, row_scale=None, rows_per_sample=0, R=None):
    """g[:R] += row_scale[r // rows_per_sample] * dtap[:R] (f32), then g_bf = bf16(g) when a bf16 copy is given."""
    R = g.shape[0] if R is None else R
    L.check(L.tap_add(_p(g), _ld(g), _p(g_bf), _ld(g_bf) if g_bf is not None else 0, _p(dtap), _ld(dtap), _p(row_scale), rows_per_sample, R, g.shape[1],
                      _stream()))
    return g


def feat_distance(pred, tgt, B, T, mode, loss, dpred):
    """loss[b] += the tap's per-sample feature distance / B; dpred = its gradient with respect to pred (fm_feat_distance)."""
    L.check(L.feat_distance(_p(pred), _ld(pred), _p(tgt), _ld(tgt), B, T, pred.shape[1], mode, _p(loss), _p(dpred), _ld(dpred), _stream()))
    return loss


# ---- LPIPS perceptual loss (csrc/lpips.hip): rows are bf16 or f32, the dtype of the row tensor selects the kernel ----------------------
def _is_f32(t):
    if t.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"feature rows are bf16 or f32, got {t.dtype}")
    return 1 if t.dtype == torch.float32 else 0


def lpips_stem(img, mul, add, w, bias, out, B, H, W):
    """out rows (B H W, 64) = relu(conv1_1(fma(img, mul, add)) + bias): ScalingLayer + the 3 -> 64 convolution (fm_lpips_stem)."""
    esz = out.element_size()
    with _prof("lpips_stem", 2.0 * B * H * W * 64 * 27, B * H * W * (12.0 + 64 * esz), tag=f"B{B} {H}x{W}"):
        L.check(L.lpips_stem(_p(img), _p(mul), _p(add), _p(w), _p(bias), _p(out), _ld(out), _is_f32(out), B, H, W, _stream()))
    return out


def lpips_stem_bwd(d, w, mul, row_scale, dimg, B, H, W):
    """dimg (B, 3, H, W) f32 = conv1_1^T(d) * mul[c] * row_scale[b] from the masked pre-activation gradient rows d (fm_lpips_stem_bwd)."""
    with _prof("lpips_stem_bwd", 2.0 * B * H * W * 64 * 27, B * H * W * (12.0 + 64 * d.element_size()), tag=f"B{B} {H}x{W}"):
        L.check(L.lpips_stem_bwd(_p(d), _ld(d), _is_f32(d), _p(w), _p(mul), _p(row_scale), _p(dimg), B, H, W, _stream()))
    return dimg


def maxpool2x2_nhwc(x, y, B, H, W, C):
    """y rows (B H/2 W/2, C) = the 2 x 2 max-pool of x rows (B H W, C) (fm_maxpool2x2_nhwc)."""
    with _prof("maxpool2x2_nhwc", 0.0, 1.25 * B * H * W * C * x.element_size(), tag=f"B{B} {H}x{W} C{C}"):
        L.check(L.maxpool2x2_nhwc(_p(x), _ld(x), _p(y), _ld(y), _is_f32(x), B, H, W, C, _stream()))
    return y


def lpips_distance_scratch(B, P):
    """Number of f32 values fm_lpips_distance needs as scratch."""
    return B * ((P + L.LPIPS_CHUNK - 1) // L.LPIPS_CHUNK)


def lpips_distance(pred, tgt, w, B, P, loss, dpred, scratch):
    """loss[b] += mean over the P pixels of sum_c w_c (p^ - t^)^2; dpred (f32 rows or None) = its gradient with respect to pred."""
    C_ = pred.shape[1]
    assert scratch.dtype == torch.float32 and scratch.numel() >= lpips_distance_scratch(B, P) and _is_f32(pred) == _is_f32(tgt)
    with _prof("lpips_distance", 0.0, B * P * C_ * (2.0 * pred.element_size() + (4.0 if dpred is not None else 0.0)), tag=f"B{B} P{P} C{C_}"):
        L.check(L.lpips_distance(_p(pred), _ld(pred), _p(tgt), _ld(tgt), _is_f32(pred), _p(w), B, P, C_, _p(loss), _p(dpred),
                                 _ld(dpred) if dpred is not None else 0, _p(scratch), _stream()))
    return loss


def lpips_tap_bwd(act, d, B, H, W, din=None, dtap=None, dpool=None):
    """d = [act > 0] (din + dtap + dpool routed to the first maximum of each 2 x 2 window); din may be d itself (fm_lpips_tap_bwd)."""
    C_ = act.shape[1]
    f = _is_f32(act)
    assert _is_f32(d) == f and (din is None or _is_f32(din) == f) and (dpool is None or _is_f32(dpool) == f) and (dtap is None or dtap.dtype == torch.float32)
    n_in = (din is not None) + (dpool is not None) * 0.25
    with _prof("lpips_tap_bwd", 0.0, B * H * W * C_ * ((2.0 + n_in) * act.element_size() + (4.0 if dtap is not None else 0.0)), tag=f"B{B} {H}x{W} C{C_}"):
        L.check(L.lpips_tap_bwd(_p(act), _ld(act), _p(din), _ld(din) if din is not None else 0, _p(dtap), _ld(dtap) if dtap is not None else 0,
                                _p(dpool), _ld(dpool) if dpool is not None else 0, _p(d), _ld(d), f, B, H, W, C_, _stream()))
    return d


def cast_pad(src, dst):
    """dst (rows, ld>=cols) bf16 <- src (rows, cols) f32, padding zeroed."""
    s2 = src.reshape(src.shape[0], -1)
    L.check(L.cast_pad(_p(s2), s2.stride(0), _p(dst), _ld(dst), s2.shape[0], s2.shape[1], _stream()))
    return dst


def transpose_cast_pad(src, dst):
    """dst (cols, width>=rows) bf16 <- src(rows, cols)^T, columns [rows, width) zeroed (dst may be a
    column slice of a wider buffer)."""
    s2 = src.reshape(src.shape[0], -1)
    L.check(L.transpose_cast_pad(_p(s2), s2.stride(0), _p(dst), _ld(dst), dst.shape[1], s2.shape[0], s2.shape[1], _stream()))
    return dst


def shadow_jobs_table(jobs, device):
    """jobs: list of (src f32 2-D view, dst bf16 | f32 2-D view, transpose[, col_scale f32 (cols,) | None]) ->
    (device byte tensor of fm_shadow_desc, total tiles)."""
    arr = (L.ShadowDesc * len(jobs))()
    tiles = 0
    for i, job in enumerate(jobs):
        src, dst, tr = job[:3]
        scale = job[3] if len(job) > 3 else None
        rows, cols = src.shape
        need = (cols, rows) if tr else (rows, cols)
        assert src.dtype == torch.float32 and dst.dtype in (torch.bfloat16, torch.float32) and src.stride(1) == 1 and dst.stride(1) == 1
        assert dst.shape[0] >= need[0] and dst.shape[1] >= need[1], (tuple(dst.shape), need)
        d = arr[i]
        d.src, d.dst, d.ld_src, d.ld_dst = src.data_ptr(), dst.data_ptr(), src.stride(0), dst.stride(0)
        d.rows, d.cols, d.transpose, d.tile_start = rows, cols, 1 if tr else 0, tiles
        d.dst_f32 = 1 if dst.dtype == torch.float32 else 0
        if scale is not None:
            assert scale.dtype == torch.float32 and scale.numel() == cols and scale.is_contiguous()
            d.col_scale = scale.data_ptr()
        tiles += ((rows + 63) // 64) * ((cols + 63) // 64)
    raw = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(device)
    return raw, tiles


@_timed("fold_colscale_grad")
def fold_colscale_grad(jobs):
    """jobs = [(dWp f32 (rows, cols) view, W f32 master, gamma f32 (cols,), gW f32 | None, ggamma f32 (cols,) | None)]:
    gW += dWp * gamma[None, :];  ggamma += sum_r dWp * W  (csrc/elementwise.hip fold_colscale_grad_kernel)."""
    for lo in range(0, len(jobs), L.FOLD_MAX_JOBS):
        part = jobs[lo:lo + L.FOLD_MAX_JOBS]
        arr = (L.FoldGradJob * len(part))()
        for j, (dwp, w, gamma, gw, gg) in zip(arr, part):
            rows, cols = w.shape[0], w[0].numel()
            assert w.is_contiguous() and (gw is None or gw.is_contiguous()) and dwp.stride(1) == 1
            j.dWp, j.W, j.gamma, j.gW, j.ggamma = _p(dwp), _p(w), _p(gamma), _p(gw), _p(gg)
            j.rows, j.cols, j.ld_dwp = rows, cols, dwp.stride(0)
        L.check(L.fold_colscale_grad(arr, len(part), _stream()))


@_timed("shadow_refresh")
def shadow_refresh(table, n_jobs, tiles):
    L.check(L.shadow_refresh(_p(table), n_jobs, tiles, _stream()))


@_timed("colsum")
def colsum(dy, db, N, R=None):
    if dy.dtype == torch.float32:
        return L.check(L.colsum_f32(_p(dy), _ld(dy), _p(db), dy.shape[0] if R is None else R, N, _stream()))
    L.check(L.colsum(_p(dy), _ld(dy), _p(db), dy.shape[0] if R is None else R, N, _stream()))


@_timed("casts")
def f32_to_bf16(src, dst):
    if dst.dtype == torch.float32:
        return dst.copy_(src)
    L.check(L.f32_to_bf16(_p(src), _p(dst), src.numel(), _stream()))
    return dst


@_timed("casts")
def bf16_to_f32_scaled(src, dst, scale=1.0):
    L.check(L.bf16_to_f32_scaled(_p(src), _p(dst), src.numel(), float(scale), _stream()))
    return dst


@_timed("drop_path")
def scale_rows_bf16(x, scale, rows_per_sample, R, N=None):
    """x[r] *= scale[r // rows_per_sample] (bf16, in place): DropPath on a branch output / on the gradient entering the branch."""
    L.check(L.scale_rows_bf16(_p(x), _ld(x), _p(scale), rows_per_sample, R, x.shape[1] if N is None else N, _stream()))
    return x


@_timed("casts")
def add_bf16_to_f32(x, delta, out, R=None):
    """out[:R] = x[:R] + delta[:R] (contiguous (rows, D) buffers of equal width)."""
    R = x.shape[0] if R is None else R
    assert x.is_contiguous() and delta.is_contiguous() and out.is_contiguous() and x.shape[1] == delta.shape[1] == out.shape[1]
    L.check(L.add_bf16_f32(_p(x), _p(delta), _p(out), R * x.shape[1], _stream()))
    return out


@_timed("casts")
def layerscale_add(x, delta, gamma, out, R=None, D=None):
    """out[:R, :D] = x + gamma * float(delta) (delta bf16 or f32; product and sum rounded separately; out may be x): fm_layerscale_add."""
    R = x.shape[0] if R is None else R
    D = gamma.numel() if D is None else D
    assert delta.dtype in (torch.bfloat16, torch.float32) and x.dtype == out.dtype == gamma.dtype == torch.float32 and gamma.numel() == D
    L.check(L.layerscale_add(_p(x), _ld(x), _p(delta), _ld(delta), 1 if delta.dtype == torch.float32 else 0, _p(gamma), _p(out), _ld(out), R, D, _stream()))
    return out


def cls_pos_embed(patches, cls, reg, pos, out, B, G, D):
    """DINOv2's token assembly (fm_cls_pos_embed): out (B * (1 + n_reg + G), D) f32 from patch rows (bf16 / f32), the class token, the register
    rows (or None) and the position table (1 + G, D) of this grid."""
    n_reg = 0 if reg is None else reg.shape[-2]
    assert cls.dtype == pos.dtype == out.dtype == torch.float32 and pos.is_contiguous() and pos.numel() == (1 + G) * D and cls.numel() == D
    assert reg is None or (reg.dtype == torch.float32 and reg.is_contiguous() and reg.shape[-1] == D)
    L.check(L.cls_pos_embed(_p(patches), _ld(patches), 1 if patches.dtype == torch.float32 else 0, _p(cls), _p(reg), n_reg, _p(pos), _p(out), _ld(out),
                            B, G, D, _stream()))
    return out


@_timed("adamw")
def adamw(p, g, m, v, n, lr, beta1, beta2, eps, wd, step, grad_mult=None, hyper=None, sumsq=None):
    L.check(L.adamw(_p(p), _p(g), _p(m), _p(v), n, lr, beta1, beta2, eps, wd, step, _p(grad_mult), _p(hyper), _p(sumsq), _stream()))


ADAMW_CHUNK = 8192   # FM_ADAMW_CHUNK


def adamw_jobs_table(jobs, device):
    """jobs: list of dicts(p, g, m, v: fp32 tensors of one (rows, cols) matrix; plain / t: bf16 2-D destinations or None)
    -> (device byte tensor of fm_adamw_job, total tiles)."""
    arr = (L.AdamWJob * len(jobs))()
    tiles = 0
    for i, j in enumerate(jobs):
        p = j["p"]
        rows, cols = p.shape[0], p[0].numel()
        d = arr[i]
        for k in ("p", "g", "m", "v"):
            t = j[k]
            assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == rows * cols, (k, t.dtype, tuple(t.shape))
            setattr(d, k, t.data_ptr())
        pl, tr = j.get("plain"), j.get("t")
        if pl is not None:
            assert pl.dtype == torch.bfloat16 and pl.stride(1) == 1 and pl.shape[0] >= rows and pl.shape[1] >= cols
            d.dst_plain, d.ld_plain = pl.data_ptr(), pl.stride(0)
        assert tr is None, "transposed shadows are refreshed by fm_shadow_refresh"
        d.rows, d.cols, d.tile_start = rows, cols, tiles
        tiles += (rows * cols + ADAMW_CHUNK - 1) // ADAMW_CHUNK
    raw = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(device)
    return raw, tiles


@_timed("adamw")
def adamw_shadow(table, n_jobs, tiles, lr, beta1, beta2, eps, wd, step, grad_mult=None, hyper=None, sumsq=None):
    L.check(L.adamw_shadow(_p(table), n_jobs, tiles, lr, beta1, beta2, eps, wd, step, _p(grad_mult), _p(hyper), _p(sumsq), _stream()))


@_timed("grad_norm")
def sumsq(x, out):
    L.check(L.sumsq(_p(x), x.numel(), _p(out), _stream()))


@_timed("grad_norm")
def clip_coef(ss, max_norm, norm_out, coef_out):
    L.check(L.clip_coef(_p(ss), float(max_norm or 0.0), _p(norm_out), _p(coef_out), _stream()))


def dense_decoder_mask(cs, mod, B, M, causal, use_sep):
    out = torch.empty(B, M, M, dtype=torch.bool, device=(cs if cs is not None else mod).device)
    L.check(L.dense_decoder_mask(_p(cs), _p(mod), _p(out), B, M, 1 if causal else 0, 1 if cs is not None else 0,
                                 1 if use_sep else 0, _stream()))
    return out


# ---------------------------------------------------------------------------------------------
# dense ViT front end (csrc/vit_embed.hip)
# ---------------------------------------------------------------------------------------------
def vit_patch_rows(pixels, rows, P):
    """rows[(b, gy, gx)][(py, px, c)] <- pixels (B, C, H, W) fp32: every patch in grid order; rows bf16 or fp32, pad columns zeroed."""
    B, C, H, W = pixels.shape
    assert pixels.dtype == torch.float32 and pixels.is_contiguous() and rows.dtype in (torch.bfloat16, torch.float32)
    assert rows.shape[0] >= B * (H // P) * (W // P)
    with _prof("vit_patch_rows", 0.0, pixels.numel() * 4.0 + B * (H // P) * (W // P) * _ld(rows) * rows.element_size()):
        L.check(L.vit_patch_rows(_p(pixels), _p(rows), _ld(rows), B, C, H, W, P, 1 if rows.dtype == torch.float32 else 0, _stream()))
    return rows


def vit_emb_rows(pos, mod_emb, x, B, Np):
    """x[(b, n)] = pos[n] + mod_emb (fp32): the rows the patch projection is added onto (gemm_nt, EPI_RESIDUAL in place)."""
    D = mod_emb.numel()
    pos, mod_emb = pos.detach(), mod_emb.detach()
    assert pos.dtype == mod_emb.dtype == x.dtype == torch.float32 and pos.is_contiguous() and pos.numel() == Np * D and x.shape[0] >= B * Np
    with _prof("vit_emb_rows", 0.0, 4.0 * B * Np * D):
        L.check(L.vit_emb_rows(_p(pos), _p(mod_emb), _p(x), _ld(x), B, Np, D, _stream()))
    return x


# ---------------------------------------------------------------------------------------------
# low-rank adapters (csrc/lora.hip)
# ---------------------------------------------------------------------------------------------
def _f32_flag(t):
    if t.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"bf16 or fp32 tensor expected, got {t.dtype}")
    return 1 if t.dtype == torch.float32 else 0


@_timed("lora_apply")
def lora_apply(x, down, up, y, scale, p_out, R, K, N, backward=False):
    """P = x down^T, y += scale P up^T, P -> p_out, with down (r, K) / up (N, r) fp32 masters.  backward: the roles are exchanged -
    x is dY (R, K = out_features), y is dX (R, N = in_features), ``down`` is still lora_down.weight (r, N) and ``up`` lora_up.weight (K, r):
    dX += scale (dY up) down and p_out receives Q = dY up."""
    down, up = down.detach(), up.detach()
    assert down.dtype == up.dtype == p_out.dtype == torch.float32 and down.is_contiguous() and up.is_contiguous() and p_out.is_contiguous()
    r = down.shape[0]
    assert up.shape[1] == r and p_out.shape[1] == r and p_out.shape[0] >= R
    if backward:
        assert tuple(up.shape) == (K, r) and tuple(down.shape) == (r, N)
        a, a_sr, a_sk, b, b_sn, b_sr = up, 1, r, down, 1, N
    else:
        assert tuple(down.shape) == (r, K) and tuple(up.shape) == (N, r)
        a, a_sr, a_sk, b, b_sn, b_sr = down, K, 1, up, r, 1
    assert x.shape[0] >= R and y.shape[0] >= R and x.shape[1] >= K and y.shape[1] >= N
    L.check(L.lora_apply(_p(x), _ld(x), _p(a), a_sr, a_sk, _p(b), b_sn, b_sr, _p(y), _ld(y), float(scale), _p(p_out), R, K, N, r,
                         _f32_flag(x), _f32_flag(y), _stream()))


@_timed("lora_grad")
def lora_grad(a, b, out, scale, R, n, transposed=False, accumulate=True):
    """out (+)= scale a^T b over the first R rows: out (n, r), or (r, n) with ``transposed`` (lora_down.weight's layout)."""
    out = out.detach()
    r = b.shape[1]
    assert b.dtype == out.dtype == torch.float32 and b.is_contiguous() and out.is_contiguous() and b.shape[0] >= R and a.shape[0] >= R
    assert tuple(out.shape) == ((r, n) if transposed else (n, r)) and a.shape[1] >= n
    sn, sr = (1, n) if transposed else (r, 1)
    L.check(L.lora_grad(_p(a), _ld(a), _p(b), _p(out), sn, sr, float(scale), 1 if accumulate else 0, R, n, r, _f32_flag(a), _stream()))


def vit_colsum(dy, db, ws, R=None):
    """db[n] += sum_r dy[r][n] (fp32 dy and db), every column summed in double in a fixed order and rounded once.  ``ws``: float64 scratch
    of at least 64 * N elements."""
    R, N = dy.shape[0] if R is None else R, db.numel()
    assert dy.dtype == db.dtype == torch.float32 and ws.dtype == torch.float64 and db.is_contiguous() and dy.shape[0] >= R and dy.shape[1] >= N
    with _prof("colsum", 0.0, 4.0 * R * N):
        L.check(L.vit_colsum(_p(dy), _ld(dy), _p(db), R, N, _p(ws), ws.numel() * 8, _stream()))
    return db


# ---------------------------------------------------------------------------------------------
# tokenizer training objective (csrc/train_objective.hip)
# ---------------------------------------------------------------------------------------------
def reconst_loss(x, target, mode, grad=None):
    """-> loss (1,) f32 of fm_reconst_loss on x (B, C, H, W) f32 contiguous; ``grad`` (x's shape or None) receives d loss / d x."""
    B, C_ = x.shape[0], x.shape[1]
    HW = x.numel() // (B * C_)
    assert x.dtype == torch.float32 and x.is_contiguous() and target.is_contiguous() and (grad is None or (grad.dtype == torch.float32 and grad.is_contiguous()))
    assert target.dtype == (torch.int64 if mode == L.LOSS_CE_INDEX else torch.float32)
    n = L.reconst_loss_scratch(mode, B, C_, HW)
    L.check(min(n, 0))
    scratch = torch.empty(n, dtype=torch.float32, device=x.device)
    loss = torch.empty(1, dtype=torch.float32, device=x.device)
    with _prof("reconst_loss", 0.0, 4.0 * x.numel() * (2.0 + (grad is not None))):
        L.check(L.reconst_loss(_p(x), _p(target), mode, B, C_, HW, _p(grad), _p(scratch), _p(loss), _stream()))
    return loss


def scale_f32(x, scale):
    """x *= scale[0] in place (scale: a one-element f32 device tensor; exactly 1 leaves x alone) - fm_scale_f32."""
    assert x.dtype == scale.dtype == torch.float32 and x.is_contiguous() and scale.numel() == 1
    L.check(L.scale_f32(_p(x), _p(scale), x.numel(), _stream()))
    return x


def mask_out_samples(clean, valid_u8, mask_value, out):
    """clean (B, C, H, W) f32 overwritten in place where valid_u8 (B, 1, H, W) is 0; out (B, C + 1, H, W) = [clean | valid * 2 - 1]."""
    B, C_ = clean.shape[0], clean.shape[1]
    HW = clean.numel() // (B * C_)
    assert clean.dtype == out.dtype == torch.float32 and clean.is_contiguous() and out.is_contiguous() and out.numel() == B * (C_ + 1) * HW
    assert valid_u8.dtype == torch.uint8 and valid_u8.is_contiguous() and valid_u8.numel() == B * HW
    L.check(L.mask_out_samples(_p(clean), _p(valid_u8), float(mask_value), _p(out), B, C_, HW, _stream()))
    return out


def ema_jobs_table(pairs, device):
    """pairs: [(ema, model)] f32 contiguous device tensors of equal sizes -> (device byte tensor of fm_ema_job, total chunks)."""
    arr = (L.EmaJob * len(pairs))()
    chunks = 0
    for i, (e, m) in enumerate(pairs):
        assert e.dtype == m.dtype == torch.float32 and e.is_contiguous() and m.is_contiguous() and e.numel() == m.numel() > 0 and e.device == m.device == device
        arr[i].ema, arr[i].model, arr[i].n, arr[i].first_chunk = e.data_ptr(), m.data_ptr(), e.numel(), chunks
        chunks += (e.numel() + L.EMA_CHUNK - 1) // L.EMA_CHUNK
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(device), chunks


def ema_update(table, n_jobs, chunks, decay):
    """ema = ema * float(decay) + float(1 - decay) * model over the job list, one launch (1 - decay in double first, as Python forms it)."""
    with _prof("ema_update", 0.0, 12.0 * chunks * L.EMA_CHUNK):
        L.check(L.ema_update(_p(table), n_jobs, chunks, float(decay), float(1.0 - decay), _stream()))


def diffusion_pair(clean, noise, timesteps, sqrt_alpha, sqrt_sigma, noisy, velocity=None):
    B = clean.shape[0]
    assert clean.dtype == noise.dtype == noisy.dtype == torch.float32 and clean.is_contiguous() and noise.is_contiguous() and noisy.is_contiguous()
    assert timesteps.dtype == torch.int64 and timesteps.is_contiguous() and timesteps.numel() == B and sqrt_alpha.numel() == sqrt_sigma.numel()
    assert velocity is None or (velocity.dtype == torch.float32 and velocity.is_contiguous())
    L.check(L.diffusion_pair(_p(clean), _p(noise), _p(timesteps), _p(sqrt_alpha), _p(sqrt_sigma), sqrt_alpha.numel(), _p(noisy), _p(velocity), B,
                             clean.numel() // B, _stream()))
    return noisy, velocity


def token_usage(tokens, n_windows, window, K, counts, bad):
    """counts[w] (int32) = distinct tokens of window w; bad[0] (int32) = tokens outside [0, K)."""
    assert tokens.dtype in (torch.int16, torch.int32, torch.int64) and tokens.is_contiguous() and tokens.numel() >= n_windows * window
    assert counts.dtype == bad.dtype == torch.int32 and counts.numel() >= n_windows
    L.check(L.token_usage(_p(tokens), tokens.element_size(), n_windows, window, K, _p(counts), _p(bad), _stream()))
    return counts


# ---------------------------------------------------------------------------------------------
# tokenizer validation metrics (csrc/metrics.hip)
# ---------------------------------------------------------------------------------------------
def _image_pair(x, y, c_use):
    assert x.dtype == y.dtype == torch.float32 and x.dim() == y.dim() == 4 and x.is_contiguous() and y.is_contiguous()
    assert x.shape[0] == y.shape[0] and x.shape[2:] == y.shape[2:] and 0 < c_use <= min(x.shape[1], y.shape[1])
    return x.shape[0], x.shape[1], y.shape[1], x.shape[2], x.shape[3]


def metric_sums(pred, target, c_use, transform, sums, counts, iou=False, threshold=0.5):
    """sums (2,) f64 += [sum d^2, sum |d|] and counts (5,) int64 += [tp, fp, fn, n, bad targets] (tp, fp, fn, bad only with ``iou``) over the
    first ``c_use`` channels of pred / target (B, C, H, W) f32, converted by ``transform`` in the loads - fm_metric_sums."""
    B, Cp, Ct, H, W = _image_pair(pred, target, c_use)
    assert sums.dtype == torch.float64 and sums.numel() == 2 and counts.dtype == torch.int64 and counts.numel() == 5 and sums.is_contiguous() and counts.is_contiguous()
    n = L.metric_sums_scratch(B, c_use, H * W)
    L.check(min(n, 0))
    scratch = torch.empty(n, dtype=torch.float64, device=pred.device)
    with _prof("metric_sums", 0.0, 8.0 * B * c_use * H * W):
        L.check(L.metric_sums(_p(pred), _p(target), B, Cp, Ct, c_use, H * W, transform, int(bool(iou)), float(threshold), _p(scratch), _p(sums), _p(counts), _stream()))


def ssim_scale(x, y, c_use, transform, window, c1, c2, ssim, cs):
    """ssim (B,), cs (B,) f64 = the per-image means of SSIM and of its contrast-structure term at one scale, window (k,) f32 taps - fm_ssim_scale."""
    B, Cx, Cy, H, W = _image_pair(x, y, c_use)
    assert window.dtype == torch.float32 and window.dim() == 1 and window.is_contiguous()
    assert ssim.dtype == cs.dtype == torch.float64 and ssim.numel() == cs.numel() == B and ssim.is_contiguous() and cs.is_contiguous()
    n = L.ssim_scale_scratch(B, c_use, H, W, window.numel())
    L.check(min(n, 0))
    scratch = torch.empty(n, dtype=torch.float64, device=x.device)
    with _prof("ssim_scale", 0.0, 8.0 * B * c_use * H * W):
        L.check(L.ssim_scale(_p(x), _p(y), B, Cx, Cy, c_use, H, W, transform, _p(window), window.numel(), float(c1), float(c2), _p(scratch), _p(ssim), _p(cs), _stream()))


def avgpool2x2_pair(x, y, c_use, transform, xo=None, yo=None):
    """-> (xo, yo) (B, c_use, H // 2, W // 2) f32: the 2 x 2 means of the converted first ``c_use`` channels of both images - fm_avgpool2x2_pair."""
    B, Cx, Cy, H, W = _image_pair(x, y, c_use)
    if xo is None:
        xo = torch.empty(B, c_use, H // 2, W // 2, dtype=torch.float32, device=x.device)
        yo = torch.empty_like(xo)
    assert xo.dtype == yo.dtype == torch.float32 and xo.is_contiguous() and yo.is_contiguous() and xo.numel() == yo.numel() == B * c_use * (H // 2) * (W // 2)
    L.check(L.avgpool2x2_pair(_p(x), _p(y), B, Cx, Cy, c_use, H, W, transform, _p(xo), _p(yo), _stream()))
    return xo, yo


def token_histogram(tokens, K, hist, bad):
    """hist (K,) int64 += occurrences of every token value; bad[0] (int32) = tokens outside [0, K) - fm_token_histogram."""
    assert tokens.dtype in (torch.int16, torch.int32, torch.int64) and tokens.is_contiguous()
    assert hist.dtype == torch.int64 and hist.numel() == K and hist.is_contiguous() and bad.dtype == torch.int32
    L.check(L.token_histogram(_p(tokens), tokens.element_size(), tokens.numel(), K, _p(hist), _p(bad), _stream()))
    return hist


# ---------------------------------------------------------------------------------------------
# image resize, forward and adjoint (csrc/resize.hip)
# ---------------------------------------------------------------------------------------------
def resize_axis_table(n_in, n_out, mode):
    """fm_resize_axis_table on the host -> dict of CPU tensors: start, count int32 (n_out), weights f32 and weights_f64 (n_out, taps), t_start,
    t_count int32 (n_in), and the ints taps and t_taps (the largest count / t_count).  No GPU call."""
    taps = L.resize_axis_table(n_in, n_out, mode, None, None, None, None, None, None)
    L.check(min(taps, 0))
    start, count = torch.empty(n_out, dtype=torch.int32), torch.empty(n_out, dtype=torch.int32)
    w32, w64 = torch.empty(n_out, taps, dtype=torch.float32), torch.empty(n_out, taps, dtype=torch.float64)
    ts, tc = torch.empty(n_in, dtype=torch.int32), torch.empty(n_in, dtype=torch.int32)

    def ptr(t, ct):
        return C.cast(t.data_ptr(), C.POINTER(ct))
    got = L.resize_axis_table(n_in, n_out, mode, ptr(start, C.c_int32), ptr(count, C.c_int32), ptr(w32, C.c_float), ptr(w64, C.c_double), ptr(ts, C.c_int32),
                              ptr(tc, C.c_int32))
    L.check(min(got, 0))
    assert got == taps
    return dict(start=start, count=count, weights=w32, weights_f64=w64, t_start=ts, t_count=tc, taps=taps, t_taps=int(tc.max()))


def _resize_axis_ok(t, n_in, n_out):
    return (t["start"].dtype == t["count"].dtype == t["t_start"].dtype == t["t_count"].dtype == torch.int32 and t["weights"].dtype == torch.float32
            and t["start"].numel() == t["count"].numel() == n_out and t["weights"].numel() == n_out * t["taps"] and t["t_start"].numel() == t["t_count"].numel() == n_in
            and all(t[k].is_contiguous() for k in ("start", "count", "weights", "t_start", "t_count")))


def _resize_affine(scale, shift, C_):
    for v in (scale, shift):
        assert v is None or (v.dtype == torch.float32 and v.is_contiguous() and v.numel() == C_)


def resize_bilinear_fwd(x, y, th, tw, scale=None, shift=None):
    """y (B, C, H_out, W_out) = scale[c] * R(x) + shift[c] for x (B, C, H_in, W_in) f32 - fm_resize_bilinear_fwd.  th, tw: the axis tables
    on x's device (dicts as resize_axis_table returns them, for the rows and the columns)."""
    B, C_, Hi, Wi = x.shape
    Ho, Wo = y.shape[2], y.shape[3]
    assert x.dtype == y.dtype == torch.float32 and x.is_contiguous() and y.is_contiguous() and y.shape[:2] == x.shape[:2]
    assert _resize_axis_ok(th, Hi, Ho) and _resize_axis_ok(tw, Wi, Wo) and (scale is None) == (shift is None)
    _resize_affine(scale, shift, C_)
    with _prof("resize_bilinear_fwd", 0.0, 4.0 * (x.numel() + y.numel())):
        L.check(L.resize_bilinear_fwd(_p(x), _p(y), B * C_, Hi, Wi, Ho, Wo, _p(th["start"]), _p(th["count"]), _p(th["weights"]), th["taps"],
                                      _p(tw["start"]), _p(tw["count"]), _p(tw["weights"]), tw["taps"], _p(scale), _p(shift), C_, _stream()))
    return y


def resize_bilinear_bwd(dy, dx, th, tw, scale=None):
    """dx (B, C, H_in, W_in) = scale[c] * R^T(dy) for dy (B, C, H_out, W_out) f32: the adjoint of resize_bilinear_fwd as a gather, no atomics -
    fm_resize_bilinear_bwd."""
    B, C_, Hi, Wi = dx.shape
    Ho, Wo = dy.shape[2], dy.shape[3]
    assert dx.dtype == dy.dtype == torch.float32 and dx.is_contiguous() and dy.is_contiguous() and dy.shape[:2] == dx.shape[:2]
    assert _resize_axis_ok(th, Hi, Ho) and _resize_axis_ok(tw, Wi, Wo)
    _resize_affine(scale, None, C_)
    with _prof("resize_bilinear_bwd", 0.0, 4.0 * (dx.numel() + dy.numel())):
        L.check(L.resize_bilinear_bwd(_p(dy), _p(dx), B * C_, Hi, Wi, Ho, Wo, _p(th["start"]), _p(th["count"]), _p(th["weights"]), th["taps"],
                                      _p(th["t_start"]), _p(th["t_count"]), _p(tw["start"]), _p(tw["count"]), _p(tw["weights"]), tw["taps"],
                                      _p(tw["t_start"]), _p(tw["t_count"]), _p(scale), C_, _stream()))
    return dx


def resize_nearest(x, y, index_h, index_w):
    """y (..., H_out, W_out) = x (..., H_in, W_in) gathered at (index_h[oh], index_w[ow]) for f32 or int64 elements - fm_resize_nearest."""
    assert x.dtype == y.dtype and x.dtype in (torch.float32, torch.int64) and x.is_contiguous() and y.is_contiguous() and x.dim() == y.dim() >= 3
    assert x.shape[:-2] == y.shape[:-2] and index_h.dtype == index_w.dtype == torch.int32 and index_h.is_contiguous() and index_w.is_contiguous()
    Hi, Wi, Ho, Wo = x.shape[-2], x.shape[-1], y.shape[-2], y.shape[-1]
    assert index_h.numel() == Ho and index_w.numel() == Wo
    L.check(L.resize_nearest(_p(x), _p(y), x.element_size(), x.numel() // (Hi * Wi), Hi, Wi, Ho, Wo, _p(index_h), _p(index_w), _stream()))
    return y


# ---------------------------------------------------------------------------------------------
# CLIP text tower and CLIP score (csrc/clip_text.hip)
# ---------------------------------------------------------------------------------------------
def clip_text_embed(ids, tok, pos, out, eot_row, bad, eot_map=None):
    """out[b Lc + t] = tok[ids[b, t]] + pos[t] (f32 rows), eot_row (B,) int32 = b Lc + argmax_t ids[b, t] (first maximum), eot_map (B Lc,) int32
    (optional) = the same pick as a LayerNorm row map, bad (1,) int32 = ids outside the table (their rows are zeros) - fm_clip_text_embed."""
    B, Lc = ids.shape
    V, D = tok.shape
    assert ids.dtype == torch.int64 and ids.is_contiguous() and tok.dtype == pos.dtype == out.dtype == torch.float32 and tok.is_contiguous() and pos.is_contiguous()
    assert tuple(pos.shape) == (Lc, D) and out.dim() == 2 and out.shape[0] >= B * Lc and out.shape[1] >= D
    assert eot_row.dtype == torch.int32 and eot_row.numel() == B and bad.dtype == torch.int32 and bad.numel() == 1
    assert eot_map is None or (eot_map.dtype == torch.int32 and eot_map.numel() == B * Lc and eot_map.is_contiguous())
    with _prof("clip_text_embed", 0.0, 8.0 * B * Lc * D):
        L.check(L.clip_text_embed(_p(ids), _p(tok), _p(pos), _p(out), _ld(out), _p(eot_row), _p(eot_map), _p(bad), B, Lc, D, V, _stream()))
    return out


def clip_pair_score(img, txt, score, total, count=None):
    """score (B,) f32 = 100 cos(img[b], txt[b]); total (1,) f64 += their sum (fixed order), count (1,) int64 += B - fm_clip_pair_score."""
    B, E = img.shape
    assert img.dtype == txt.dtype == score.dtype == torch.float32 and tuple(txt.shape) == (B, E) and img.stride(1) == 1 and txt.stride(1) == 1
    assert score.numel() == B and score.is_contiguous() and total.dtype == torch.float64 and total.numel() == 1
    assert count is None or (count.dtype == torch.int64 and count.numel() == 1)
    n = L.clip_pair_score_scratch(B)
    L.check(min(n, 0))
    scratch = torch.empty(n, dtype=torch.float64, device=img.device)
    L.check(L.clip_pair_score(_p(img), img.stride(0), _p(txt), txt.stride(0), _p(score), _p(scratch), _p(total), _p(count), B, E, _stream()))
    return score


def l2_normalize_rows(x, y=None, factor=1.0, factor_dev=None):
    """y[r] = x[r] * factor * factor_dev[0] / |x[r]| for f32 rows (R, E); y None: in place; a zero row stays zero - fm_l2_normalize_rows."""
    y = x if y is None else y
    R, E = x.shape
    assert x.dtype == y.dtype == torch.float32 and tuple(y.shape) == (R, E) and x.stride(1) == 1 and y.stride(1) == 1
    assert factor_dev is None or (factor_dev.dtype == torch.float32 and factor_dev.numel() == 1)
    L.check(L.l2_normalize_rows(_p(x), x.stride(0), _p(y), y.stride(0), R, E, _p(factor_dev), float(factor), _stream()))
    return y
