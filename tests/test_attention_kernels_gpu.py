"""Every route of fm_attn_fwd / fm_attn_bwd (csrc/attention.hip), element by element against a float64 reference.

The case table, the reference and the per-element bounds live in tests/attn_f64_util.py; tests/test_attention_ref_cpu.py proves on
the CPU that the bounds hold for a faithful restatement of the kernels' rounding points and reject subtly wrong ones.  Here:
  * q / k / v / dO are column views of wider buffers whose surplus columns (and, for a K/V cache, surplus rows) hold NaN;
  * o / dq / dk / dv are column views of sentinel-filled buffers with a guard row, stat_m / stat_l carry a guard element: every
    byte outside the result is unchanged after the call;
  * O, stat_m, stat_l, dQ, dK, dV pass ``within`` per element; the backward is fed the forward's own o and statistics, and its
    reference is the float64 value of the backward AS A FUNCTION OF THOSE INPUTS;
  * where the reference is structurally zero (dQ of a fully blocked query, dK of a key no query may see, dV of such a key in a sample
    without fully blocked rows) the bound is exactly zero: the kernel must write zero.
Which kernel a case reaches follows from the dispatch rule (restated by attn_f64_util.fwd_route / bwd_route; the table's comments
name the kernel per row) - valid only with no FOURM_ATTN_* variable set, hence the skip below."""
import ctypes as C
import os

import pytest
import torch

from tests import attn_f64_util as A
from tests.attn_f64_util import B, H, heads, within
from tests.parity_log import record

pytestmark = pytest.mark.gpu

if any(k.startswith("FOURM_ATTN_") for k in os.environ):
    pytest.skip("FOURM_ATTN_* variables change the dispatch the case table assumes", allow_module_level=True)

DEV = "cuda:0"
D = H * A.HD
SENT16 = 0x5A5A                                           # bf16 sentinel bit pattern of the output buffers
SENTF = -12345.0                                          # guard value of stat_m / stat_l


def _ops():
    from fourm.hip import _lib as L
    from fourm.hip import ops
    return ops, L


def nan_wide(x, width, col0, rows=None):
    """``x`` (R, D) as the column view [col0, col0 + D) of a (rows, width) buffer that holds NaN everywhere else."""
    buf = torch.full((rows or x.shape[0], width), float("nan"), dtype=torch.bfloat16, device=DEV)
    buf[:x.shape[0], col0:col0 + x.shape[1]] = x.to(DEV)
    return buf


def out_view(rows, layout):
    """A sentinel-filled (rows + 1 guard row, width) bf16 buffer and its (rows, D) column view.  layout 0: rows 16-byte aligned;
    1: ld % 8 == 4 (every other row 8 bytes off); 2: ld % 8 == 0 but the first column 8 bytes off."""
    width, col0 = {0: (D + 16, 8), 1: (D + 12, 4), 2: (D + 16, 4)}[layout]
    buf = torch.empty(rows + 1, width, dtype=torch.int16, device=DEV).fill_(SENT16).view(torch.bfloat16)
    view = buf[:rows, col0:col0 + D]
    assert (view.stride(0) % 8 == 0 and view.data_ptr() % 16 == 0) == (layout == 0)
    return buf, view, col0


def untouched(buf, rows, col0):
    """Every element of ``buf`` outside [0, rows) x [col0, col0 + D) still holds the sentinel."""
    bits = buf.view(torch.int16).clone()
    bits[:rows, col0:col0 + D] = SENT16
    return bool((bits == SENT16).all())


def stat_buf(n):
    return torch.full((n + 1,), SENTF, dtype=torch.float32, device=DEV)


_GPU_FIX = {}


def gpu_fixture(c):
    """The case's inputs in their wide NaN-padded device buffers (built once per shape / mask / ramp / cache layout)."""
    key = (c.Nq, c.Nk, c.mask, c.ramp, c.kvr)
    if key not in _GPU_FIX:
        fx = A.fixture(c)
        if c.Nq == c.Nk and not c.kvr:                    # q, k, v from one 3 D-wide qkv buffer
            qkv = nan_wide(torch.cat([fx.q, fx.k, fx.v], 1), 3 * D + 8, 0)
            q2, k2, v2 = qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:3 * D]
        else:
            q2 = nan_wide(fx.q, D + 8, 8)[:, 8:8 + D]
            kvr = c.kvr or c.Nk
            kv = torch.cat([fx.k, fx.v], 1).reshape(B, c.Nk, 2 * D)
            kvb = torch.full((B, kvr, 2 * D + 8), float("nan"), dtype=torch.bfloat16, device=DEV)      # cache rows >= Nk: NaN
            kvb[:, :c.Nk, :2 * D] = kv.to(DEV)
            kvb = kvb.reshape(B * kvr, 2 * D + 8)
            k2, v2 = kvb[:, :D], kvb[:, D:2 * D]
        do2 = nan_wide(fx.do, D + 16, 8)[:, 8:8 + D]
        mk = fx.mask.to(DEV)
        dev = {n: getattr(fx, n).to(DEV) for n in ("q", "k", "v", "do")}
        _GPU_FIX[key] = (fx, q2, k2, v2, do2, mk, dev)
    return _GPU_FIX[key]


def mask_kwargs(L, mk):
    kind = dict(none=L.MASK_NONE, keypad=L.MASK_KEYPAD, decoder=L.MASK_DECODER, dense=L.MASK_DENSE)[mk.kind]
    return dict(mask_kind=kind, kpad=mk.kpad, cs=mk.cs, modq=mk.modq, modk=mk.modk, dense=mk.dense, causal=mk.causal)


@pytest.mark.parametrize("c", A.CASES, ids=lambda c: c.id)
def test_attention_route(c):
    ops, L = _ops()
    fx, q2, k2, v2, do2, mk, dev = gpu_fixture(c)
    Nq, Nk, scale = c.Nq, c.Nk, fx.scale
    sh = (B, H, Nq, Nk, scale)
    blk = mk.blocked
    kw = mask_kwargs(L, mk)

    # ---- forward ------------------------------------------------------------------------------------------------------------------
    obuf, o2, ocol = out_view(B * Nq, c.o_layout)
    smb, slb = stat_buf(B * H * Nq), stat_buf(B * H * Nq)
    sm, sl = smb[:-1].view(B, H, Nq), slb[:-1].view(B, H, Nq)
    ops.attn_fwd(q2, k2, v2, o2, B, H, Nq, Nk, scale, stat_m=sm, stat_l=sl, force_tr=c.tr, kv_batch_rows=c.kvr, zero_attn=c.zero_attn, **kw)
    torch.cuda.synchronize()
    assert untouched(obuf, B * Nq, ocol), "forward wrote outside o"
    assert float(smb[-1]) == SENTF and float(slb[-1]) == SENTF, "forward wrote past stat_m / stat_l"
    ref = A.ref_forward(dev["q"], dev["k"], dev["v"], *sh, blk, c.zero_attn)
    tO, tm, tl = A.fwd_bounds(dev["q"], dev["k"], dev["v"], *sh, ref, blk)
    o = o2.contiguous()
    ratios = dict(O=within("O", heads(o, B, Nq, H), ref["O"], tO), stat_m=within("stat_m", sm, ref["m"], tm),
                  stat_l=within("stat_l", sl, ref["l"], tl))
    if blk is not None:
        full = blk.all(-1)[:, None].expand(B, H, Nq)
        if c.zero_attn:                                   # a fully blocked row under softmax1: O = 0, m = 0, l = 1, exactly
            assert bool((heads(o, B, Nq, H)[full] == 0).all()) and bool((sm[full] == 0).all()) and bool((sl[full] == 1).all())
        else:                                             # ... and without it the marker the backward keys on
            assert bool((sm[full] < -1e38).all())

    # ---- backward, fed the forward's own o and statistics ---------------------------------------------------------------------------
    if c.bwd != "-":
        bufs = [out_view(B * n, c.g_layout) for n in (Nq, Nk, Nk)]
        (qb, dq2, qc), (kb, dk2, kc), (vb, dv2, vc) = bufs
        sm_in, sl_in = smb.clone(), slb.clone()
        ops.attn_bwd(q2, k2, v2, o2, do2, dq2, dk2, dv2, B, H, Nq, Nk, scale, sm, sl, force_tr=c.tr, zero_attn=c.zero_attn, **kw)
        torch.cuda.synchronize()
        assert untouched(qb, B * Nq, qc) and untouched(kb, B * Nk, kc) and untouched(vb, B * Nk, vc), "backward wrote outside dq / dk / dv"
        assert untouched(obuf, B * Nq, ocol) and torch.equal(o2, o) and torch.equal(smb, sm_in) and torch.equal(slb, sl_in), "backward changed its inputs"
        rb = A.ref_backward(dev["q"], dev["k"], dev["v"], o, dev["do"], sm, sl, *sh, blk)
        tq, tk, tv = A.bwd_bounds(dev["q"], dev["k"], dev["v"], o, dev["do"], sm, sl, *sh, rb, blk)
        if blk is not None:                               # the structural zeros carry a zero bound (test_attention_ref_cpu.py checks the same on the CPU)
            dead = blk.all(-2)[:, None].expand(B, H, Nk)
            assert bool((tk[dead] == 0).all())
            if not c.zero_attn:
                assert bool((tq[blk.all(-1)[:, None].expand(B, H, Nq)] == 0).all())
        ratios.update(dQ=within("dQ", heads(dq2.contiguous(), B, Nq, H), rb["dQ"], tq), dK=within("dK", heads(dk2.contiguous(), B, Nk, H), rb["dK"], tk),
                      dV=within("dV", heads(dv2.contiguous(), B, Nk, H), rb["dV"], tv))
    print(c.id, c.fwd, c.bwd, {k: round(v, 3) for k, v in ratios.items()})
    record("attention.kernels", case=c.id, fwd=c.fwd, bwd=c.bwd, **{k: round(v, 4) for k, v in ratios.items()})


def test_the_check_rejects_a_kernel_run_with_one_key_unblocked():
    """The harness on the real kernel: the same call with ONE blocked (b, q, k) of the dense mask cleared must fall outside the bounds
    of the unchanged reference - the head / row mapping of the comparison and the bounds have teeth on the device too."""
    ops, L = _ops()
    c = next(c for c in A.CASES if c.id == "130x65-dense-tr1")
    fx, q2, k2, v2, do2, mk, dev = gpu_fixture(c)
    sh = (B, H, c.Nq, c.Nk, fx.scale)
    wrong = mk.dense.clone()
    b, q = B - 1, 77
    assert not bool(wrong[b, q].all())
    t0 = heads(dev["k"], B, c.Nk, H)[b, 0] @ heads(dev["q"], B, c.Nq, H)[b, 0, q]
    k = int(torch.where(wrong[b, q], t0, torch.full_like(t0, -float("inf"))).argmax())      # the blocked key head 0 would attend to most
    wrong[b, q, k] = False
    obuf, o2, ocol = out_view(B * c.Nq, 0)
    sm, sl = (torch.zeros(B, H, c.Nq, device=DEV) for _ in range(2))
    ops.attn_fwd(q2, k2, v2, o2, *sh, mask_kind=L.MASK_DENSE, dense=wrong, stat_m=sm, stat_l=sl, force_tr=1)
    ref = A.ref_forward(dev["q"], dev["k"], dev["v"], *sh, mk.blocked)
    tO, tm, tl = A.fwd_bounds(dev["q"], dev["k"], dev["v"], *sh, ref, mk.blocked)
    with pytest.raises(AssertionError, match=rf"stat_l: \d+ of \d+ outside the bound.*first at \({b}, 0, {q}\)"):
        within("stat_l", sl, ref["l"], tl)
    with pytest.raises(AssertionError, match=rf"O: \d+ of \d+ outside the bound.*first at \({b}, \d, {q}, \d+\)"):
        within("O", heads(o2.contiguous(), B, c.Nq, H), ref["O"], tO)


def test_every_route_of_the_tables_is_reached():
    """The case table reaches every kernel and template branch the dispatch can select with its defaults (a statement about the
    table; the route strings restate fm_attn_fwd / fm_attn_bwd)."""
    fwd, bwd = {c.fwd for c in A.CASES}, {c.bwd for c in A.CASES}
    assert fwd == {"attn_fwd128_kernel", "attn_fwdt_kernel", "attn_fwd_kernel<true,.>", "attn_fwd_kernel<false,.>"}
    want = {"attn_bwd128_kernel", "attn_bwd128o_kernel"} | {f"attn_bwd_kernel<{t},.,{v}>" for t in ("true", "false")
                                                             for v in ("false,true", "false,false", "true,false")}
    assert bwd - {"-"} == want
    # the fall-back from the 128 x 128 backward when the gradient rows are not 16-byte aligned
    assert any(c.g_layout and (c.Nq, c.Nk, c.tr) == (128, 128, 1) and c.bwd == "attn_bwd_kernel<true,.,false,true>" for c in A.CASES)
    # both o16 states of the two 128-tile forwards
    for kern in ("attn_fwd128_kernel", "attn_fwdt_kernel"):
        assert {bool(c.o_layout) for c in A.CASES if c.fwd == kern} == {False, True}


# ------------------------------------------------------------------------------------------------
# argument checks: each returns -1 before anything is launched, and fm_last_error names the problem
# ------------------------------------------------------------------------------------------------
def _args(L, ops, bwd=False):
    N = 32
    t = {n: torch.ones(B * N, D, dtype=torch.bfloat16, device=DEV) for n in ("q", "k", "v", "o", "do", "dq", "dk", "dv")}
    st = {n: torch.zeros(B * H * N, device=DEV) for n in ("m", "l")}
    a = L.AttnArgs()
    a.Q, a.K, a.V, a.O = (ops._p(t[n]) for n in ("q", "k", "v", "o"))
    a.ldq = a.ldk = a.ldv = a.ldo = D
    a.B, a.H, a.Nq, a.Nk, a.head_dim, a.mask_kind, a.scale, a.force_tr = B, H, N, N, 64, L.MASK_NONE, 0.125, -1
    a.stat_m, a.stat_l = ops._p(st["m"]), ops._p(st["l"])
    if bwd:
        a.dO, a.dQ, a.dK, a.dV = (ops._p(t[n]) for n in ("do", "dq", "dk", "dv"))
        a.lddo = a.lddq = a.lddk = a.lddv = D
    return a, (t, st)


BAD_ARGS = [
    ("head_dim", lambda a, L, x: setattr(a, "head_dim", 32), "head_dim=32"),
    ("ldq", lambda a, L, x: setattr(a, "ldq", D + 4), "leading dims"),
    ("keypad_without_kpad", lambda a, L, x: setattr(a, "mask_kind", L.MASK_KEYPAD), "needs kpad"),
    ("dense_without_dense", lambda a, L, x: setattr(a, "mask_kind", L.MASK_DENSE), "needs dense"),
    ("modq_without_modk", lambda a, L, x: (setattr(a, "mask_kind", L.MASK_DECODER), setattr(a, "modq", x)), "modq and modk go together"),
    ("kv_batch_rows_below_Nk", lambda a, L, x: setattr(a, "kv_batch_rows", 16), "kv_batch_rows=16 < Nk=32"),
]


@pytest.mark.parametrize("bwd", [False, True], ids=["fwd", "bwd"])
@pytest.mark.parametrize("name,mutate,text", BAD_ARGS, ids=[b[0] for b in BAD_ARGS])
def test_argument_checks(name, mutate, text, bwd):
    ops, L = _ops()
    a, keep = _args(L, ops, bwd)
    aux = torch.zeros(B * 32, dtype=torch.int16, device=DEV)
    mutate(a, L, ops._p(aux))
    rc = (L.attn_bwd if bwd else L.attn_fwd)(C.byref(a), ops._stream())
    assert rc == -1
    msg = L.lib.fm_last_error().decode()
    assert text in msg and ("fm_attn_bwd" if bwd else "fm_attn_fwd") in msg, msg
    torch.cuda.synchronize()
    assert all(bool((t == 1).all()) for t in keep[0].values())        # nothing ran: o / dq / dk / dv still hold their ones


def test_argument_checks_of_one_entry_point():
    ops, L = _ops()
    a, keep = _args(L, ops)
    a.stat_l = None                                       # one of stat_m / stat_l missing
    assert L.attn_fwd(C.byref(a), ops._stream()) == -1
    assert "stat_m and stat_l go together" in L.lib.fm_last_error().decode()
    a, keep = _args(L, ops, bwd=True)
    a.stat_l = None
    assert L.attn_bwd(C.byref(a), ops._stream()) == -1
    assert "fm_attn_bwd: null pointer" in L.lib.fm_last_error().decode()
    a, keep = _args(L, ops, bwd=True)
    a.kv_batch_rows = 48                                  # a K/V cache is a forward-only option
    assert L.attn_bwd(C.byref(a), ops._stream()) == -1
    assert "kv_batch_rows is a forward-only" in L.lib.fm_last_error().decode()
    torch.cuda.synchronize()
    assert all(bool((t == 1).all()) for t in keep[0].values())
