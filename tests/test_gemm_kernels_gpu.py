"""Every route of fm_gemm_nt / fm_gemm_tn a default build takes (csrc/gemm.hip, gemm_nt3.hip, gemm_nt4.hip, gemm_nt_flat.hip,
gemm_skinny.hip), element by element against a float64 reference.

The route restatement, the case tables, the reference and the per-element bounds live in tests/gemm_f64_util.py;
tests/test_gemm_ref_cpu.py proves on the CPU that the bounds hold for a faithful restatement of the kernels' rounding points, reject
subtly wrong ones, and that every row reaches the route it states.  Here, per row:
  * X has guard rows up to the next multiple of 256 and W up to the next multiple of 384; the guard rows and the columns behind K hold
    NaN, as do bias[N ..) and the surplus of every other input;
  * out / out2 are column views of sentinel-filled buffers with a guard row: everything outside [0, M) x [0, roundup4(N)) is
    unchanged after the call ([N, roundup4(N)) is don't-care, except that the tiled SwiGLU kernels write zeros there);
  * every output passes ``within`` - no element is excluded - and a second launch gives the same bits (NT only: TN adds atomically).
Which kernel a row reaches follows from the dispatch with its defaults on all 256 CUs - hence the skip below.

Out of scope: the implicit convolutions and FM_EPI_RELU / FM_EPI_RELU_BWD (tests/test_divae_kernels_gpu.py, test_lpips_kernels_gpu.py),
gemm_nt3's lab-only variants (fm_lab_set 3 bits 16, 256, 1024, 131072), fm_gemm_tn_multi's large lists and the grouped TN."""
import contextlib
import os

import pytest
import torch

from tests import gemm_f64_util as G
from tests.gemm_f64_util import NT_CASES, TN_CASES, check_nt, ru, within
from tests.parity_log import record

pytestmark = pytest.mark.gpu

_ENV = [k for k in os.environ if k.startswith(("FOURM_NT", "FOURM_TN")) or k in ("FOURM_RESERVED_CUS", "FOURM_HEADS_NT_CFG", "FOURM_CONV_K32")]
if _ENV:
    pytest.skip(f"{_ENV} change the dispatch the case table assumes", allow_module_level=True)
if torch.cuda.is_available() and torch.cuda.get_device_properties(0).multi_processor_count != 256:
    pytest.skip("the case table assumes the dispatch of a whole MI355X (256 CUs)", allow_module_level=True)

DEV = "cuda:0"
NAN = float("nan")
SENT16 = 0x5A5A                                           # bf16 sentinel bit pattern
SENT32 = 0x5A5A5A5A                                       # fp32 sentinel bit pattern


def _ops():
    from fourm.hip import _lib as L
    from fourm.hip import ops
    return ops, L


@contextlib.contextmanager
def settings(lab=(), nt_cfg=None, tn_cfg=None):
    """fm_lab_set / fm_set_gemm_nt_config / fm_set_gemm_tn_config for the block; the defaults come back whatever happens."""
    ops, L = _ops()
    try:
        for k, v in lab:
            L.lib.fm_lab_set(k, v)
        if nt_cfg is not None:
            L.lib.fm_set_gemm_nt_config(nt_cfg)
        if tn_cfg is not None:
            L.lib.fm_set_gemm_tn_config(tn_cfg)
        yield
    finally:
        for k, v in G.LAB_DEFAULT.items():
            L.lib.fm_lab_set(k, v)
        L.lib.fm_set_gemm_nt_config(G.NT_DEFAULT)
        L.lib.fm_set_gemm_tn_config(G.TN_DEFAULT)


def nan_padded(t, rows, cols, fill=NAN):
    """``t`` in the top-left corner of a (rows, cols) buffer that holds ``fill`` everywhere else; -> buffer."""
    buf = torch.full((rows, cols), fill, dtype=t.dtype, device=DEV)
    buf[:t.shape[0], :t.shape[1]] = t
    return buf


def sentinel(rows, ld, f32):
    """(rows + 1 guard row, ld) buffer of sentinel bits."""
    if f32:
        return torch.empty(rows + 1, ld, dtype=torch.int32, device=DEV).fill_(SENT32).view(torch.float32)
    return torch.empty(rows + 1, ld, dtype=torch.int16, device=DEV).fill_(SENT16).view(torch.bfloat16)


def bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def untouched(buf, rows, spans):
    """Every element of ``buf`` outside rows [0, rows) x the column spans [(c0, c1), ...] still holds the sentinel."""
    b = bits(buf).clone()
    s = SENT32 if buf.dtype == torch.float32 else SENT16
    for c0, c1 in spans:
        b[:rows, c0:c1] = s
    return bool((b == s).all())


_DEV_IN = {}


def dev_inputs(c):
    key = c.math_key
    if key not in _DEV_IN:
        for k in [k for k in _DEV_IN if k[0] > 30000]:     # (the large operands are not kept)
            del _DEV_IN[k]
        _DEV_IN[key] = G.nt_inputs(c).to(DEV)
    return _DEV_IN[key]


EPI = dict(bf16="EPI_BF16", gelu="EPI_GELU", res="EPI_RESIDUAL", swiglu="EPI_SWIGLU", f32="EPI_F32", tanh="EPI_TANH", swiglu_bwd="EPI_SWIGLU_BWD",
           gelu_bwd="EPI_GELU_BWD")


class Launch:
    """The buffers of one row (inputs NaN-padded, outputs sentinel-filled) and its launch."""

    def __init__(self, c, inp, w_override=None):
        M, N, K = c.M, c.N, c.K
        self.c, self.n4 = c, ru(N, 4)
        self.x = nan_padded(inp.x, ru(M, 256), K + c.ldx_pad)[:M, :K]
        self.w = nan_padded(inp.w if w_override is None else w_override, ru(N, 384), K + c.ldw_pad)[:N, :K]
        self.w2 = nan_padded(inp.w2, ru(N, 384), K + c.ldw_pad)[:N, :K] if c.epi == "swiglu" else None
        self.bias = nan_padded(inp.bias[None], 1, ru(N, 384))[0] if c.bias else None
        self.bias2 = nan_padded(inp.bias2[None], 1, ru(N, 384))[0] if (c.bias and c.epi == "swiglu") else None
        self.res = self.res_buf = None
        if c.res == "sep":
            if c.epi in ("swiglu_bwd", "gelu_bwd"):
                sv = inp.saved.clone()
                if c.epi == "swiglu_bwd":                     # the pad columns [N, Hp) of both halves are never read
                    sv[:, N:c.Hp] = NAN
                    sv[:, c.Hp + N:] = NAN
                self.res_buf = nan_padded(sv, M + 1, c.ld_res)
                self.res = self.res_buf[:M, :sv.shape[1]]
            else:
                self.res_buf = nan_padded(inp.res32, M + 1, c.ld_res)
                self.res = self.res_buf[:M, :self.n4]
        self.fresh()

    def fresh(self):
        c, M = self.c, self.c.M
        assert c.col0 + c.width <= c.ld_out
        self.out_buf = sentinel(M, c.ld_out, c.out_f32)
        self.out = self.out_buf[:M, c.col0:c.col0 + c.width]
        if c.res == "inplace":
            self.out_buf[:M, c.col0:c.col0 + c.N] = dev_inputs(c).res32
            self.res = self.out
        self.out2_buf = self.out2 = None
        if c.out2:
            self.out2_buf = sentinel(M, c.ld_out2, False)
            self.out2 = self.out2_buf[:M, :(2 * c.Hp if c.epi == "swiglu" else self.n4)]

    def run(self):
        ops, L = _ops()
        c = self.c
        with settings(c.lab, c.cfg), (ops.fixed_tiling() if c.fixed else contextlib.nullcontext()):
            ops.gemm_nt(self.x, self.w, self.out, epilogue=getattr(L, EPI[c.epi]), bias=self.bias, res=self.res, w2=self.w2, bias2=self.bias2,
                        out2=self.out2, Hp=c.Hp, N=c.N, K=c.K, M=c.M)
        torch.cuda.synchronize()

    def check_untouched(self):
        c, M, N, n4 = self.c, self.c.M, self.c.N, self.n4
        c0 = c.col0
        spans = [(c0, c0 + n4), (c0 + c.Hp, c0 + c.Hp + n4)] if c.epi == "swiglu_bwd" else [(c0, c0 + n4)]      # (in place: the residual sits in the span)
        assert untouched(self.out_buf, M, spans), f"{c.id}: wrote outside out"
        if c.out2:
            spans2 = [(0, n4), (c.Hp, c.Hp + n4)] if c.epi == "swiglu" else [(0, n4)]
            assert untouched(self.out2_buf, M, spans2), f"{c.id}: wrote outside out2"

    def outputs(self):
        c, M, N = self.c, self.c.M, self.c.N
        o = self.out
        if c.epi == "swiglu":
            r = {"act": o[:, :N].contiguous()}
            if c.out2:
                r["g"], r["u"] = self.out2[:, :N].contiguous(), self.out2[:, c.Hp:c.Hp + N].contiguous()
            return r
        if c.epi == "swiglu_bwd":
            return {"dg": o[:, :N].contiguous(), "du": o[:, c.Hp:c.Hp + N].contiguous()}
        r = {"out": o[:, :N].contiguous()}
        if c.out2:
            r["pre"] = self.out2[:, :N].contiguous()
        return r

    def all_bits(self):
        return [bits(self.out_buf).clone()] + ([bits(self.out2_buf).clone()] if self.out2_buf is not None else [])


@pytest.mark.parametrize("c", NT_CASES, ids=lambda c: c.id)
def test_nt_route(c):
    assert G.case_route(c, cus=torch.cuda.get_device_properties(0).multi_processor_count) == c.route
    inp = dev_inputs(c)
    run = Launch(c, inp)
    run.run()
    run.check_untouched()
    got = run.outputs()
    ratios = check_nt(c, inp, got)
    if c.epi == "swiglu" and run.n4 > c.N and not c.route.startswith("skinny"):
        assert bool((run.out[:, c.N:run.n4] == 0).all()), "SwiGLU: the columns [N, roundup4(N)) of act must be zero"
    first = run.all_bits()
    run.fresh()
    run.run()
    for a, b in zip(first, run.all_bits()):
        assert torch.equal(a, b), f"{c.id}: a second launch gives other bits ({int((a != b).sum())} elements)"
    print(c.id, c.route, {k: round(v, 3) for k, v in ratios.items()})
    record("gemm.kernels", case=c.id, route=c.route, **{k: round(v, 4) for k, v in ratios.items()})


def test_the_check_rejects_a_kernel_run_with_one_weight_changed():
    """The harness on the real gemm_nt3 kernel: the same launch with ONE element of W changed after the reference was built must fall
    outside the bounds, the first failing index in that weight's column - the row / column mapping of the comparison has teeth."""
    c = next(c for c in NT_CASES if c.route == "nt3.256.staged")
    inp = dev_inputs(c)
    n0, k0 = 77, 101
    w = inp.w.clone()
    w[n0, k0] += 1.0
    run = Launch(c, inp, w_override=w)
    run.run()
    with pytest.raises(AssertionError, match=rf"out: \d+ of \d+ outside the bound.*first at \[\d+, {n0}\]"):
        check_nt(c, inp, run.outputs())
    ok = run.outputs()["out"].clone()
    ref, tol = G.nt_reference(c, inp)["out"]
    ok[:, n0] = ref[:, n0].bfloat16()
    within("every other column", ok, ref, tol)


def test_fixed_tiling_rows_do_not_depend_on_the_batch():
    """Under ops.fixed_tiling() a row computed alone has the bits it has in the batch (both fixed_tiling rows of the table)."""
    ops, L = _ops()
    for c in [c for c in NT_CASES if c.fixed]:
        inp = dev_inputs(c)
        batch = torch.zeros(c.M, c.N, dtype=torch.bfloat16, device=DEV)
        single = torch.ones(c.M, c.N, dtype=torch.bfloat16, device=DEV)
        with ops.fixed_tiling():
            ops.gemm_nt(inp.x, inp.w, batch)
            for m in range(c.M):
                ops.gemm_nt(inp.x[m:m + 1], inp.w, single[m:m + 1])
        torch.cuda.synchronize()
        assert torch.equal(bits(batch), bits(single)), (c.id, int((bits(batch) != bits(single)).sum()))


# ---- device-side row ranges (gemm_nt3 DEVM) through ops.gemm_nt_heads ---------------------------------------------------------------
def test_nt_heads_device_rows():
    """One dense gemm_nt3 launch per head with the row range read from device memory: per element per head against float64, pad rows
    exactly zero (zero inputs), nothing written outside the heads' segments, same bits on a second run."""
    ops, L = _ops()
    vocabs, counts, D = G.HEADS_VOCABS, G.HEADS_COUNTS, G.HEADS_D
    assert {G.nt_route(4096, v, D, "bf16", ldo=1024, m_dev=True) for v in vocabs} == {"nt3.devm.256", "nt3.devm.192"}
    n_heads, R = len(vocabs), sum(counts) + 40
    head = torch.full((R,), -1, dtype=torch.int32)
    idx = torch.randperm(R, generator=torch.Generator().manual_seed(5))
    o = 0
    for h, cnt in enumerate(counts):
        head[idx[o:o + cnt]] = h
        o += cnt
    head = head.to(DEV)
    Rp = ops.padded_rows(R, n_heads)
    seg_start = torch.zeros(n_heads, dtype=torch.int32, device=DEV)
    seg_count = torch.zeros_like(seg_start)
    perm = torch.zeros(Rp, dtype=torch.int32, device=DEV)
    r2p = torch.zeros(R, dtype=torch.int32, device=DEV)
    tile_group = torch.zeros(Rp // ops.SEG, dtype=torch.int32, device=DEV)
    ops.segment_rows(head, n_heads, seg_start, seg_count, perm, r2p, tile_group)
    g = torch.Generator().manual_seed(112)
    y = (torch.randn(R, D, generator=g) + (torch.arange(D) % 7).float()[None] * 0.05).bfloat16().to(DEV)
    ypb = torch.full((Rp, D + 8), NAN, dtype=torch.bfloat16, device=DEV)
    yp = ypb[:, :D]
    yp.zero_()
    live = perm >= 0
    yp[live] = y[perm[live].long()]
    ws = [nan_padded(((torch.randn(v, D, generator=g) * 0.3 + (torch.arange(v) % 11).float()[:, None] * 0.02).bfloat16()).to(DEV), ru(v, 384), D + 8)[:v, :D]
          for v in vocabs]
    ldl = ru(max(vocabs), 64) + 64
    runs = []
    for rep in range(2):
        got = sentinel(Rp, ldl, False)
        view = got[:Rp, :ldl - 64]
        assert ops.heads_dense_ok(ws, vocabs, view)
        ops.gemm_nt_heads(yp, ws, vocabs, seg_start, seg_count, view, D)
        torch.cuda.synchronize()
        runs.append(bits(got).clone())
    assert torch.equal(runs[0], runs[1])
    spans_left = bits(got).clone()
    worst = {}
    for h, (v, cnt) in enumerate(zip(vocabs, counts)):
        s, n = int(seg_start[h]), ru(cnt, ops.SEG)
        if cnt:
            x = yp[s:s + cnt].contiguous()
            ref, S, t = G.acc_ref(x, ws[h].contiguous())
            worst[f"head{h}"] = within(f"head {h}", got[s:s + cnt, :v].contiguous(), ref, G.tol_bf16(ref, t))
            assert bool((got[s + cnt:s + n, :v] == 0).all()), f"head {h}: pad rows must be exactly zero"
        spans_left[s:s + n, :v] = SENT16
    assert bool((spans_left == SENT16).all()), "written outside the heads' segments"
    record("gemm.kernels", case="heads-devm", route="nt3.devm.256+192", **{k: round(v, 4) for k, v in worst.items()})


# ---- grouped NT ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", G.GROUP_KS)
def test_nt_grouped(K):
    """ops.gemm_nt_grouped: row tiles of 256 select their group's weight; a tile with tile_group = -1 is left untouched."""
    ops, L = _ops()
    Ns = G.GROUP_NS
    assert G.nt_route(1280, max(Ns), K, "bf16", grouped=True) == ("grouped.k64pp" if K >= 1536 else "grouped.k32")
    tg = [0, 1, -1, 2, 1]
    g = torch.Generator().manual_seed(900 + K)
    kr = (torch.arange(K) % 13).float() * 0.03 - 0.15
    x = (torch.randn(len(tg) * 256, K, generator=g) * 0.7 + kr[None]).bfloat16().to(DEV)
    xb = nan_padded(x, x.shape[0], K + 8)
    xv = xb[:, :K]
    ws = [nan_padded((torch.randn(n, K, generator=g) * 0.1 + (torch.arange(n) % 11).float()[:, None] * 0.01).bfloat16().to(DEV), ru(n, 384), K + 8)
          for n in Ns]
    groups = ops.make_groups([dict(W=w, N=n, K=K, ldw=K + 8) for w, n in zip(ws, Ns)], DEV)
    tile_group = torch.tensor(tg, dtype=torch.int32, device=DEV)
    ld = ru(max(Ns), 64) + 64
    runs = []
    for rep in range(2):
        buf = sentinel(x.shape[0], ld, False)
        ops.gemm_nt_grouped(xv, groups, tile_group, buf[:x.shape[0], :ld - 64], max(Ns), max_K=K)
        torch.cuda.synchronize()
        runs.append(bits(buf).clone())
    assert torch.equal(runs[0], runs[1])
    left = bits(buf).clone()
    worst = {}
    for t, gi in enumerate(tg):
        if gi < 0:
            continue
        n = Ns[gi]
        rows = slice(t * 256, (t + 1) * 256)
        ref, S, tt = G.acc_ref(x[rows], ws[gi][:n, :K].contiguous())
        worst[f"tile{t}"] = within(f"tile {t} (group {gi})", buf[rows, :n].contiguous(), ref, G.tol_bf16(ref, tt))
        left[rows, :ru(n, 4)] = SENT16
    assert bool((left == SENT16).all()), "written outside the groups' columns, or into the skipped tile"
    record("gemm.kernels", case=f"grouped-K{K}", route="grouped", **{k: round(v, 4) for k, v in worst.items()})


# ---- TN ------------------------------------------------------------------------------------------------------------------------------
def tn_buffers(R, N, K, seed=0):
    a, b, out0 = G.tn_inputs(R, N, K, seed)
    Rb = ru(R, 64)
    ab = torch.full((Rb, N + 16), NAN, dtype=torch.bfloat16, device=DEV)
    bb = torch.full((Rb, K + 16), NAN, dtype=torch.bfloat16, device=DEV)
    av, bv = ab[:, 8:8 + N], bb[:, 8:8 + K]
    av[:R], bv[:R] = a.to(DEV), b.to(DEV)
    av[R:] = 1e4                                          # rows past R: never part of the reduction
    ob = sentinel(N, K + 8, True)
    ob[:N, :K] = out0.to(DEV)
    return a.to(DEV), b.to(DEV), out0.to(DEV), av, bv, ob


@pytest.mark.parametrize("c", TN_CASES, ids=lambda c: c.id)
def test_tn_route(c):
    ops, L = _ops()
    assert G.tn_route(c.R, c.N, c.K, c.force_tr, c.cfg, c.splits, cus=torch.cuda.get_device_properties(0).multi_processor_count) == c.route
    a, b, out0, av, bv, ob = tn_buffers(c.R, c.N, c.K)
    with settings(tn_cfg=c.cfg):
        ops.gemm_tn(av, bv, ob[:c.N, :c.K], R=c.R, splits=c.splits, force_tr=c.force_tr)
    torch.cuda.synchronize()
    assert untouched(ob, c.N, [(0, c.K)]), "wrote outside out"
    ref, tol = G.tn_reference(a, b, out0, c.R, c.route[3])
    ratio = within(c.id, ob[:c.N, :c.K].contiguous(), ref, tol)
    record("gemm.kernels", case="tn-" + c.id, route=str(c.route), out=round(ratio, 4))


@pytest.mark.parametrize("cfg", [1, 3])
@pytest.mark.parametrize("name", sorted(G.TN_MULTI_LISTS))
def test_tn_multi(name, cfg):
    """fm_gemm_tn_multi on its default configuration and on 128 x 256 list tiles: every job per element; a tile is touched by at most
    R / 64 + 1 workgroups (one atomic addition each)."""
    ops, L = _ops()
    jobs, keep = [], []
    for i, (R, N, K) in enumerate(G.TN_MULTI_LISTS[name]):
        a, b, out0, av, bv, ob = tn_buffers(R, N, K, seed=10 + i)
        # (ops.gemm_tn_multi passes a_cols = the view's width; R rows are passed explicitly)
        jobs.append((av, bv, ob[:N, :K], N, K, R))
        keep.append((a, b, out0, ob, R, N, K))
    with settings(tn_cfg=cfg):
        ops.gemm_tn_multi(jobs)
    torch.cuda.synchronize()
    worst = {}
    for i, (a, b, out0, ob, R, N, K) in enumerate(keep):
        assert untouched(ob, N, [(0, K)]), f"job {i}: wrote outside out"
        ref, tol = G.tn_reference(a, b, out0, R, R // 64 + 1)
        worst[f"job{i}"] = within(f"{name} job {i}", ob[:N, :K].contiguous(), ref, tol)
    record("gemm.kernels", case=f"tn-multi-{name}-cfg{cfg}", route="tn_multi", **{k: round(v, 4) for k, v in worst.items()})


def test_the_settings_are_back_at_their_defaults():
    ops, L = _ops()
    assert L.lib.fm_get_gemm_nt_config() == 9 and L.lib.fm_get_gemm_tn_config() == G.TN_DEFAULT
