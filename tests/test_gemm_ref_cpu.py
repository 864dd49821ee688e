"""CPU validation of tests/gemm_f64_util.py (no GPU):
  1. a faithful fp32 restatement of every epilogue (blocked K accumulation in two block orders, the kernels' rounding points, an fp32
     emulation of the split-K partial sums and their reduction pass) stays inside the per-element bounds at every table shape;
  2. each deliberately wrong variant is rejected, the first failing index inside the mutated region;
  3. the route every row states is what the restated dispatch gives at 256 CUs, the table covers the explicit route list, and the
     restatement reproduces the accept / decline facts of fm_launch_nt4 that tests/test_kernels_gpu.py documents."""
import pytest
import torch

from tests import gemm_f64_util as G
from tests.gemm_f64_util import NT_CASES, TN_CASES, NTCase, case_route, check_nt, emu_nt, nt_inputs, nt_route, tn_route, within


def _splits(c):
    return int(c.route.split(".")[1]) if c.route.startswith("splitk") else 0


def _first(rows, **kw):
    for c in rows:
        if all(getattr(c, k) == v for k, v in kw.items()):
            return c
    raise KeyError(kw)


# ---- 1. the faithful restatement is inside the bounds --------------------------------------------------------------------------------
@pytest.mark.parametrize("c", NT_CASES, ids=lambda c: c.id)
def test_faithful_restatement_is_within_the_bounds(c):
    inp = nt_inputs(c)
    for order in (0, 1):
        got = emu_nt(c, inp, order=order, splits=_splits(c))
        worst = check_nt(c, inp, got, f" order {order}")
        assert max(worst.values()) <= 1.0


@pytest.mark.parametrize("c", TN_CASES, ids=lambda c: c.id)
def test_tn_faithful_restatement_is_within_the_bounds(c):
    a, b, out0 = G.tn_inputs(c.R, c.N, c.K)
    pp, kb, masked, splits = c.route
    ref, tol = G.tn_reference(a, b, out0, c.R, splits)
    within(c.id, G.emu_tn(a, b, out0, c.R, kb, splits), ref, tol)


# ---- 2. mutations --------------------------------------------------------------------------------------------------------------------
def _rejected(c, mut, region, splits=0):
    """emu_nt with the mutation fails ``within``; -> the failing output's first index, asserted inside region = (r0, r1, c0, c1)."""
    inp = nt_inputs(c)
    check_nt(c, inp, emu_nt(c, inp, splits=splits))                  # the unmutated run passes
    with pytest.raises(G.OutsideBound) as e:
        check_nt(c, inp, emu_nt(c, inp, mut=mut, splits=splits))
    i, j = e.value.index
    r0, r1, c0, c1 = region
    assert r0 <= i < r1 and c0 <= j < c1, (e.value.index, region)
    return e.value


def test_rejects_a_dropped_last_k_tile_in_one_output_tile():
    c = _first(NT_CASES, M=200, N=132, K=1536)
    _rejected(c, dict(drop_tile=(128, 200, 128, 132)), (128, 200, 128, 132))
    c = _first(NT_CASES, M=2050, N=256, K=128, bias=False)          # 2 K-tiles: half of the sum missing in the ragged last row tile
    _rejected(c, dict(drop_tile=(2048, 2050, 0, 256)), (2048, 2050, 0, 256))


def test_rejects_two_swapped_rows_in_the_ragged_last_row_tile():
    c = _first(NT_CASES, M=2050, N=256, K=128, bias=False)
    _rejected(c, dict(swap_rows=2048), (2048, 2050, 0, 256))
    c = _first(NT_CASES, M=200, N=130, K=128)
    _rejected(c, dict(swap_rows=198), (198, 200, 0, 130))


@pytest.mark.parametrize("key", [dict(M=200, N=132, K=128), dict(M=2050, N=256, K=128, bias=False), dict(M=200, N=320, K=128, epi="gelu"),
                                 dict(M=192, N=170, K=128, out2=True)])
def test_rejects_truncation_to_bf16(key):
    c = _first(NT_CASES, **key)
    _rejected(c, dict(truncate=True), (0, c.M, 0, c.N))


@pytest.mark.parametrize("key", [dict(M=200, N=132, K=576, bias=True), dict(M=2050, N=192, K=128, bias=True), dict(M=200, N=320, K=128, epi="f32", res=""),
                                 dict(M=32, N=42, K=128, epi="bf16", bias=True)])
def test_rejects_a_bias_skipped_on_the_last_column_group(key):
    c = _first(NT_CASES, **key)
    n4 = G.ru(c.N, 4) - 4
    _rejected(c, dict(bias_skip_last4=True), (0, c.M, n4, c.N), splits=_splits(c))


@pytest.mark.parametrize("K", [576, 4096])
def test_rejects_a_split_k_slice_added_twice(K):
    c = _first(NT_CASES, M=200, N=132, K=K, bias=False)
    assert _splits(c) >= 2
    _rejected(c, dict(slice_twice=True), (0, c.M, 0, c.N), splits=_splits(c))


@pytest.mark.parametrize("key", [dict(M=2050, N=256, K=128, bias=True), dict(M=200, N=132, K=576, bias=True)])
def test_rejects_an_unrounded_bias_in_a_bf16_epilogue(key):
    c = _first(NT_CASES, **key)
    _rejected(c, dict(bias_unrounded=True), (0, c.M, 0, c.N), splits=_splits(c))


@pytest.mark.parametrize("key", [dict(M=192, N=170, K=128, out2=True), dict(M=192, N=170, K=128, out2=False), dict(M=2050, N=128, K=128, epi="swiglu"),
                                 dict(M=7, N=44, K=64, epi="swiglu", bias=True)])
def test_rejects_exchanged_swiglu_operands(key):
    c = _first(NT_CASES, **key)
    _rejected(c, dict(swap_gu=True), (0, c.M, 0, c.N))


@pytest.mark.parametrize("c", [c for c in TN_CASES if c.R % 64], ids=lambda c: c.id)
def test_tn_rejects_the_first_masked_row(c):
    """Row R of A holds 1e4 and of B NaN in the GPU test; here B's row is finite so that the failure is a wrong VALUE, not a NaN."""
    a, b, out0 = G.tn_inputs(c.R + 1, c.N, c.K, seed=1)
    a[c.R] = 1e4
    pp, kb, masked, splits = c.route
    ref, tol = G.tn_reference(a, b, out0, c.R, splits)
    within(c.id, G.emu_tn(a, b, out0, c.R, kb, splits), ref, tol)
    with pytest.raises(G.OutsideBound):
        within(c.id, G.emu_tn(a, b, out0, c.R, kb, splits, include_row_R=True), ref, tol)
    b[c.R] = float("nan")
    with pytest.raises(G.OutsideBound):
        within(c.id, G.emu_tn(a, b, out0, c.R, kb, splits, include_row_R=True), ref, tol)


# ---- 3. routes -----------------------------------------------------------------------------------------------------------------------
# every kernel / variant a default build reaches through fm_gemm_nt (the table rows plus the two entry points with their own tests)
NT_ROUTES = {
    "skinny.bf16", "skinny.res", "skinny.swiglu",
    "small128.k32", "small128.k64", "splitk.2.short_last", "splitk.6", "splitk.16",
    "tiled.m128", "tiled.cfg11", "tiled.cfg10", "tiled.swiglu.cfg12", "tiled.cfg12", "tiled.cfg11.gtcus", "tiled.cfg10.wrap", "tiled.fixed",
    "nt3.256.staged", "nt3.192.staged", "nt3.256.unstaged", "nt3.256.staged.bias", "nt3.192.staged.bias", "nt3.swiglu.staged",
    "nt3.swiglu.unstaged", "nt3.swiglu_bwd", "nt3.256.staged.wrap", "nt3.devm.256", "nt3.devm.192",
    "grouped.k32", "grouped.k64pp",
    "nt4.384.staged", "nt4.384.staged.wrap", "nt4.384.staged.forced", "nt4.384.unstaged.forced", "nt4.256.staged",
    "flat.bf16", "flat.swiglu",
}


def _special_routes():
    r = {nt_route(4096, v, G.HEADS_D, "bf16", ldo=1024, m_dev=True) for v in G.HEADS_VOCABS}
    r |= {nt_route(1280, max(G.GROUP_NS), k, "bf16", grouped=True) for k in G.GROUP_KS}
    return r


@pytest.mark.parametrize("c", NT_CASES, ids=lambda c: c.id)
def test_every_row_reaches_the_route_it_states(c):
    assert case_route(c, cus=256) == c.route


@pytest.mark.parametrize("c", TN_CASES, ids=lambda c: c.id)
def test_every_tn_row_states_its_route(c):
    assert tn_route(c.R, c.N, c.K, c.force_tr, c.cfg, c.splits, cus=256) == c.route
    pp, kb, masked, splits = c.route
    assert pp == (c.cfg == 1 and c.force_tr == 1) and kb == (64 if pp else 32) and masked == (c.R % kb != 0)
    if c.splits:
        assert splits == c.splits
    if (c.R, c.splits) == (1030, 0):
        assert splits == (2 if pp else 4)              # 17 K-steps of 64 / 33 of 32, at least 8 per workgroup


def test_the_table_covers_the_route_list():
    assert {c.route for c in NT_CASES} | _special_routes() == NT_ROUTES
    assert {c.route[:3] for c in TN_CASES} == {(True, 64, False), (True, 64, True), (False, 32, False), (False, 32, True)}
    assert {c.route[3] for c in TN_CASES} >= {1, 2, 3}


def test_the_rows_that_switch_the_small_grid_policy_off_need_to():
    """A row carries (9, 0) only where the policy would take the launch: with the policy on, its route is a small-grid one."""
    for c in NT_CASES:
        if (9, 0) in c.lab and c.epi == "bf16":
            on = NTCase(**{**c.__dict__, "lab": tuple(kv for kv in c.lab if kv[0] != 9)})
            assert case_route(on).startswith(("small128", "splitk")), c.id


def test_nt4_accepts_and_declines_as_documented():
    shapes = [(32768, 768, 768), (4096, 2304, 768), (2048, 1536, 1024), (8192, 768, 4096), (2304, 384, 192), (6144, 768, 2048)]
    for mode in (1, 5):
        took = [G.nt4_takes(*s, mode) is not None for s in shapes]
        assert took == [True, False, False, False, False, False], (mode, took)
    for mode in (9, 13):
        assert all(G.nt4_takes(*s, mode) is not None for s in shapes)
    # in front of fm_launch_nt4 the small-grid policy takes four of the six shapes; with it off the launch reaches nt4 (modes 9, 13)
    policy = [nt_route(*s, "bf16", ldo=s[1], splitk_ws_bytes=G.lends_splitk(*s, "bf16")).split(".")[0] for s in shapes]
    assert policy == ["nt4", "nt3", "small128", "small128", "small128", "small128"], policy
    for mode in (9, 13):
        assert all(nt_route(*s, "bf16", ldo=s[1], lab={9: 0, 4: mode}).startswith("nt4.384") for s in shapes)
    # the flat tests' shapes: nt3 / nt4 / the policy sit in front of the flat kernel until they are switched off
    for s in [(32768, 768, 768), (6000, 2304, 768), (2048, 128, 512), (4100, 768, 4096), (33000, 1536, 1024)]:
        assert not nt_route(*s, "bf16", ldo=s[1], nt_config=G.NT_FLAT, splitk_ws_bytes=G.lends_splitk(*s, "bf16")).startswith("flat")
        assert nt_route(*s, "bf16", ldo=s[1], nt_config=G.NT_FLAT, lab={2: 0, 4: 0, 9: 0}) == "flat.bf16"
    for M, Hd, K, save in [(32768, 2048, 768, True), (5000, 448, 768, True), (4096, 2048, 768, False)]:
        kw = dict(out2=save, ldo=Hd, ldo2=2 * Hd, Hp=Hd, nt_config=G.NT_FLAT)
        assert nt_route(M, Hd, K, "swiglu", **kw).startswith("nt3.swiglu")
        assert nt_route(M, Hd, K, "swiglu", lab={2: 0, 4: 0}, **kw) == "flat.swiglu"
        assert nt_route(M, Hd, K, "swiglu", lab={2: 0, 4: 0}, **{**kw, "nt_config": G.NT_DEFAULT}).startswith("tiled.swiglu.cfg12")


def test_route_depends_on_the_cu_count():
    """The table is valid on a whole MI355X only (the GPU module skips otherwise): with 16 CUs reserved N = 768 leaves nt4."""
    assert nt_route(32768, 768, 768, "bf16", ldo=768, cus=256).startswith("nt4")
    assert nt_route(32768, 768, 768, "bf16", ldo=768, cus=240).startswith("nt3")
