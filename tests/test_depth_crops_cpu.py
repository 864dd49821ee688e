"""Pillow-exact 16-bit depth crops without a GPU: the restatement (tests/pil_resize16_util.py) against Pillow (live and through
tests/golden/depth_crops.npz) and against upstream's recorded truncated_depth_standardization, fm_pil_axis_table_f64 against the restatement,
decode_depth, the ABI additions, and every refusal that happens before a launch.  The kernels are tested on the GPU
(tests/test_depth_crops_gpu.py)."""
import ctypes
import io
import os
import re

import numpy as np
import pytest
import torch

from tests import pil_resize16_util as U
from tests import pil_resize_util as U8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "depth_crops.npz")
NEW = ["fm_pil_axis_table_f64", "fm_pil_crop_resize16", "fm_depth_standardize"]
P32, P64 = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)
PLAIN_CLAMP_DIFFERS = ("edge_up_bicubic", "edge_up_bicubic_flip", "checkerboard_up")


@pytest.fixture(scope="module")
def fx():
    f = np.load(GOLDEN)
    return {k: f[k] for k in f.files}


def _header():
    return open(os.path.join(ROOT, "include", "fourm_hip.h")).read()


def _c_table_f64(n, S, fid):
    from fourm.hip import _lib as L
    taps = L.pil_axis_table_f64(n, S, fid, None, None, None)
    assert taps >= 1, L.lib.fm_last_error()
    st, ct, cf = np.zeros(S, np.int32), np.zeros(S, np.int32), np.full((S, taps), np.nan)
    assert L.pil_axis_table_f64(n, S, fid, st.ctypes.data_as(P32), ct.ctypes.data_as(P32), cf.ctypes.data_as(P64)) == taps
    return st, ct, cf


def _c_table_i32(n, S, fid):
    from fourm.hip import _lib as L
    taps = L.pil_axis_table(n, S, fid, None, None, None)
    assert taps >= 1, L.lib.fm_last_error()
    st, ct, cf = np.zeros(S, np.int32), np.zeros(S, np.int32), np.zeros((S, taps), np.int32)
    assert L.pil_axis_table(n, S, fid, st.ctypes.data_as(P32), ct.ctypes.data_as(P32), cf.ctypes.data_as(P32)) == taps
    return st, ct, cf


def _edge_image():
    edge = np.zeros((40, 48), np.uint16)
    edge[:, :24] = 65535
    return edge


def test_restatement_equals_pillow_live():
    pytest.importorskip("PIL")
    rng = np.random.default_rng(0)
    edge = _edge_image()
    fixed = [(edge, (10, 20, 6, 8, 0), 33, "bicubic"), (edge, (0, 17, 9, 12, 1), 16, "bicubic")]          # upscales over the 65535 | 0 edge
    noise = rng.integers(0, 65536, (80, 96), dtype=np.uint16)
    for filt in U.FILTERS:
        fixed += [(noise, (0, 0, 80, 96, 1), 8, filt), (noise, (3, 5, 16, 41, 0), 16, filt), (noise, (3, 5, 41, 16, 1), 16, filt),
                  (noise, (7, 9, 16, 16, 1), 16, filt), (noise, (5, 17, 60, 1, 0), 16, filt), (noise, (33, 4, 1, 70, 1), 16, filt)]
    for img, st, S, filt in fixed:
        assert np.array_equal(U.crop_resize16(img, st, S, filt), U.pillow_crop_resize16(img, st, S, filt)), (st, S, filt)
    for img, st, S, filt in fixed[:2]:          # the trap: a plain 0 .. 65535 clamp is not what Pillow does
        assert not np.array_equal(U.crop_resize16(img, st, S, filt, plain_clamp=True), U.pillow_crop_resize16(img, st, S, filt)), (st, S)
    for it in range(120):
        H, W = int(rng.integers(1, 60)), int(rng.integers(1, 60))
        img = rng.integers(0, 65536, (H, W), dtype=np.uint16) if it % 3 else (rng.integers(0, 2, (H, W)) * 65535).astype(np.uint16)
        h, w = int(rng.integers(1, H + 1)), int(rng.integers(1, W + 1))
        st = (int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1)), h, w, int(rng.integers(0, 2)))
        S, filt = int(rng.choice([2, 3, 7, 16, 33])), U.FILTERS[int(rng.integers(0, 3))]
        assert np.array_equal(U.crop_resize16(img, st, S, filt), U.pillow_crop_resize16(img, st, S, filt)), (img.shape, st, S, filt)


def test_restatement_equals_the_fixture(fx):
    assert len(fx["cases"]) >= 40 and str(fx["pillow_version"])
    src = [fx[f"src_{k}"] for k in range(5)]
    assert all(s.shape[0] <= 96 and s.shape[1] <= 96 and s.dtype == np.uint16 for s in src)
    names = fx["names"].tolist()
    seen = set()
    for i, (k, top, left, h, w, flip, S, f) in enumerate(fx["cases"].tolist()):
        got = U.crop_resize16(src[k], (top, left, h, w, flip), S, U.FILTERS[f])
        assert got.dtype == np.uint16 and np.array_equal(got, fx[f"out_{i}"]), names[i]
        seen.add((f, flip))
        if names[i] in PLAIN_CLAMP_DIFFERS:          # the per-byte clamp decides these: a plain 16-bit clamp gives other values
            plain = U.crop_resize16(src[k], (top, left, h, w, flip), S, U.FILTERS[f], plain_clamp=True)
            assert not np.array_equal(plain, fx[f"out_{i}"]), names[i]
            # and only in the low byte: an overshoot r > 65535 is stored as 0xff00 | (r % 256), a negative r as 0 either way
            assert 0 < np.abs(plain.astype(np.int64) - fx[f"out_{i}"].astype(np.int64)).max() <= 255, names[i]
    assert seen == {(f, flip) for f in range(3) for flip in (0, 1)}
    for must in PLAIN_CLAMP_DIFFERS + tuple(f"{n}_{f}" for n in ("down_10x", "h_eq_S", "w_eq_S", "both_eq_S", "one_wide", "one_high") for f in U.FILTERS):
        assert must in names, must
    for name in ("nearest_8_to_7", "nearest_15_to_7_flip"):          # the 8-bit path's repeated-addition index would give other values
        i = names.index(name)
        k, top, left, h, w, flip, S, f = fx["cases"][i].tolist()
        wrong = src[k][top:top + h, left:left + w][U8.nearest_index(h, S)][:, U8.nearest_index(w, S)]
        assert not np.array_equal(wrong[:, ::-1] if flip else wrong, fx[f"out_{i}"]), name
    k, top, left, h, w, flip, S, f = fx["cases"][names.index("down_10x_bicubic")].tolist()
    assert h >= 8 * S and w >= 8 * S


def test_axis_table_f64_equals_the_restatement_double_for_double():
    rng = np.random.default_rng(1)
    pairs = [(int(rng.integers(1, 700)), int(rng.integers(1, 260))) for _ in range(80)]
    pairs += [(5, 16), (7, 16), (90, 8), (17, 8), (16, 16), (1, 1), (1, 9), (9, 1), (640, 224), (480, 224), (2, 3), (3, 2), (4000, 224)]
    for n, S in pairs:
        for fid, filt in enumerate(U.FILTERS):
            st, ct, cf = _c_table_f64(n, S, fid)
            s2, c2, k2 = U.axis_table_f64(n, S, filt)
            assert cf.shape == k2.shape and np.array_equal(st, s2) and np.array_equal(ct, c2), (n, S, filt)
            assert np.all(cf == k2), (n, S, filt)          # ==, double for double
            assert np.all(st >= 0) and np.all(ct >= 1) and np.all(st + ct <= n)
            # the int32 table is the same computation, quantised: still equal to its own restatement, and to the doubles rounded to 2^22
            si, ci, ki = _c_table_i32(n, S, fid)
            s8, c8, k8 = U8.axis_table(n, S, filt)
            assert np.array_equal(si, s8) and np.array_equal(ci, c8) and np.array_equal(ki, k8), (n, S, filt)
            assert np.array_equal(ci, ct) and np.array_equal(ki, U.quantise(cf)), (n, S, filt)
            assert np.array_equal(si, st) or filt == "nearest", (n, S, filt)          # nearest: another index table, see the next test
    for fid in range(3):
        st, ct, cf = _c_table_f64(16, 16, fid)
        assert np.array_equal(st, np.arange(16)) and np.all(ct == 1) and cf.shape == (16, 1) and np.all(cf == 1.0)
    st, ct, cf = _c_table_f64(37, 16, 0)
    assert np.array_equal(st, U.nearest_index16(37, 16)) and np.all(ct == 1) and np.all(cf == 1.0)
    from fourm.hip import _lib as L
    assert L.pil_axis_table_f64(0, 4, 1, None, None, None) == -1 and L.pil_axis_table_f64(4, 4, 3, None, None, None) == -1
    assert L.pil_axis_table_f64(1 << 20, 2, 2, None, None, None) == -1 and b"FM_PIL_MAX_TAPS" in L.lib.fm_last_error()


def test_nearest_index_of_the_16_bit_path_is_the_closed_form():
    """Pillow resizes I;16 with NEAREST through its generic affine transform (a coordinate per pixel in closed form), 8-bit images through
    the affine scaler (repeated addition): two index tables that differ on some axes.  The 16-bit table function gives the first, the 8-bit
    one still the second, and Pillow (where installed) agrees with each on the axes where they differ."""
    differs = [(n, S) for n in range(1, 400) for S in (7, 24, 33, 224) if not np.array_equal(U8.nearest_index(n, S), U.nearest_index16(n, S))]
    assert len(differs) >= 10 and (8, 7) in differs
    for n, S in differs[:40]:
        assert np.array_equal(_c_table_f64(n, S, 0)[0], U.nearest_index16(n, S)), (n, S)
        assert np.array_equal(_c_table_i32(n, S, 0)[0], U8.nearest_index(n, S)), (n, S)
    pytest.importorskip("PIL")
    for n, S in differs[:40]:
        ramp = ((np.arange(n) * 37) % 65536).astype(np.uint16)
        wide, tall = ramp[None, :].repeat(2, 0), ramp[:, None].repeat(2, 1)
        assert np.array_equal(U.pillow_crop_resize16(wide, (0, 0, 2, n, 0), S, "nearest")[0], ramp[U.nearest_index16(n, S)]), (n, S)
        assert np.array_equal(U.pillow_crop_resize16(tall, (0, 0, n, 2, 0), S, "nearest")[:, 0], ramp[U.nearest_index16(n, S)]), (n, S)
        assert not np.array_equal(ramp[U8.nearest_index(n, S)], ramp[U.nearest_index16(n, S)]), (n, S)


def test_axis_table_f64_cache_layout():
    from fourm.data import crops
    tab, taps = crops.pil_axis_table_f64(90, 8, "bicubic")
    st, ct, cf = U.axis_table_f64(90, 8, "bicubic")
    assert taps == cf.shape[1] and tab.dtype == np.int32 and tab.size == 8 * (2 + 2 * taps) and tab.size % 2 == 0
    assert np.array_equal(tab[:8], st) and np.array_equal(tab[8:16], ct) and np.array_equal(tab[16:].view(np.float64).reshape(8, taps), cf)
    assert crops.pil_axis_table_f64(90, 8, "bicubic")[0] is tab


def test_standardisation_restatement_against_upstreams_recorded_output(fx):
    """Upstream sums the truncated values in fp32; the restatement's statistics are exact.  The allowed distance is 4 x the figure the make
    script measured (std_bound_units, in units of 2^-24 max|x| before the amplification by 1 / s): the margin covers upstream's summation
    order, which varies with torch's thread count and vectorisation."""
    names = fx["std_names"].tolist()
    bound = float(fx["std_bound_units"])
    assert 0.0 < bound < 16.0          # a few fp32 roundings of the sums, not a different formula
    for want in [f"{c}_S{S}" for c in ("uniform", "saturated", "constant", "band50") for S in (2, 3, 16, 33)]:
        assert want in names
    for i, name in enumerate(names):
        crop = fx[f"std_in_{i}"]
        got, (mean32, var32) = U.standardize(crop)
        s = float(np.sqrt(np.float32(var32 + np.float32(1e-6))))
        allowed = 4.0 * bound * 2.0 ** -24 * float(U.unit_f32(crop).max()) / s
        err = float(np.max(np.abs(got.astype(np.float64) - fx[f"std_out_{i}"].astype(np.float64))))
        print(f"{name}: max|upstream - restatement| {err:.3e}, allowed {allowed:.3e}")
        assert got.dtype == np.float32 and got.shape == crop.shape and err <= allowed, (name, err, allowed)
        if name.startswith("constant"):
            assert np.all(got == 0.0) and var32 == 0.0, name
        if name.startswith("one_run"):          # every value inside the truncated range is the same: exact 0 there, the outliers far away
            assert var32 == 0.0 and np.all(got[crop == 777] == 0.0) and np.all(got[crop == 5] < -10) and np.all(got[crop == 60000] > 900), name
    for name in ("saturated_S16", "saturated_S33"):          # ties straddle both rank boundaries
        v = np.sort(fx[f"std_in_{names.index(name)}"].reshape(-1))
        lo, hi = U.rank_range(v.size)
        assert v[lo - 1] == v[lo] == 0 and v[hi - 1] == v[hi] == 65535, name
    assert U.rank_range(4) == (0, 3) and U.rank_range(9) == (0, 8) and U.rank_range(256) == (25, 230) and U.rank_range(224 * 224) == (5017, 45158)


def test_standardisation_restatement_against_torch_in_double():
    """The formula itself, independent of upstream's fp32 sums: sort, slice, mean and unbiased variance in float64 torch."""
    rng = np.random.default_rng(4)
    for S in (2, 3, 16, 33):
        crop = rng.integers(0, 65536, (S, S), dtype=np.uint16)
        x = torch.from_numpy(crop.astype(np.float64) / 65535.0)
        t = torch.sort(x.reshape(-1))[0]
        t = t[int(0.1 * t.shape[0]): int((1 - 0.1) * t.shape[0])]
        mean32, var32 = U.truncated_stats(crop)
        assert abs(float(mean32) - t.mean().item()) <= 2.0 ** -24 * t.mean().item() * 1.01
        assert abs(float(var32) - t.var().item()) <= 2.0 ** -24 * t.var().item() * 1.01


def test_decode_depth_through_an_in_memory_png():
    Image = pytest.importorskip("PIL.Image")
    from fourm.data.crops import decode_depth
    rng = np.random.default_rng(2)
    depth = rng.integers(0, 65536, (13, 17), dtype=np.uint16)
    buf = io.BytesIO()
    Image.frombytes("I;16", (17, 13), depth.astype("<u2").tobytes()).save(buf, format="PNG")
    buf.seek(0)
    got = decode_depth(buf)
    assert got.dtype == np.uint16 and got.shape == (13, 17) and np.array_equal(got, depth)
    for mode, arr in (("L", np.zeros((4, 5), np.uint8)), ("RGB", np.zeros((4, 5, 3), np.uint8)), ("I", np.zeros((4, 5), np.int32)), ("F", np.zeros((4, 5), np.float32))):
        buf = io.BytesIO()
        pil = Image.fromarray(arr)
        assert pil.mode == mode
        pil.save(buf, format="TIFF")
        buf.seek(0)
        with pytest.raises(ValueError, match=f"mode '{mode}'"):
            decode_depth(buf)


def test_crop_resize_depth_refuses_before_anything_runs(monkeypatch):
    from fourm.data import crops
    from fourm.hip import _lib as L

    def boom(*a, **k):
        raise AssertionError("reached a launch")
    monkeypatch.setattr(L, "pil_crop_resize16", boom)
    monkeypatch.setattr(L, "depth_standardize", boom)
    img = np.zeros((20, 30), np.uint16)
    ok = [np.array([[0, 0, 5, 5, 0]])]
    for bad in ([0, 0, 21, 5, 0], [0, 26, 5, 5, 0], [-1, 0, 5, 5, 0], [0, 0, 0, 5, 0], [18, 0, 3, 5, 1], [0, 0, 5, 5, 2]):
        with pytest.raises(ValueError, match="leaves the 20 x 30 image|flip"):
            crops.crop_resize_depth([img], [np.array([[0, 0, 5, 5, 0], bad])], 8)
    with pytest.raises(ValueError, match="resample"):
        crops.crop_resize_depth([img], ok, 8, resample="lanczos")
    with pytest.raises(ValueError, match="out "):
        crops.crop_resize_depth([img], ok, 8, out="uint8")
    with pytest.raises(ValueError, match="out "):
        crops.crop_resize_depth([img], ok, 8, out=())
    with pytest.raises(ValueError, match="fewer than two elements"):
        crops.crop_resize_depth([img], ok, 1)
    with pytest.raises(ValueError, match="return_stats"):
        crops.crop_resize_depth([img], ok, 8, standardize=False, return_stats=True)
    with pytest.raises(ValueError, match="size"):
        crops.crop_resize_depth([img], ok, 0)
    with pytest.raises(ValueError, match="one settings array per image"):
        crops.crop_resize_depth([img, img], ok, 8)
    with pytest.raises(ValueError, match=r"\(n, 5\)"):
        crops.crop_resize_depth([img], [np.array([0, 0, 5, 5, 0])], 8)
    with pytest.raises(ValueError, match="integers"):
        crops.crop_resize_depth([img], [np.array([[0, 0, 5.5, 5, 0]])], 8)
    with pytest.raises(TypeError, match="uint16"):
        crops.crop_resize_depth([img.astype(np.uint8)], ok, 8)
    with pytest.raises(ValueError, match=r"\(H, W\)"):
        crops.crop_resize_depth([np.zeros((4, 5, 3), np.uint16)], ok, 8)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU path"):
            crops.crop_resize_depth([img], ok, 8)
        with pytest.raises(RuntimeError, match="no CPU path"):          # size 1 is fine without the standardisation
            crops.crop_resize_depth([img], ok, 1, standardize=False)


def test_crop_modalities_refuses_before_anything_runs(monkeypatch):
    from fourm.data import multimodal_crops as M

    def boom(*a, **k):
        raise AssertionError("reached a crop call")
    monkeypatch.setattr(M, "crop_resize", boom)
    monkeypatch.setattr(M, "crop_resize_depth", boom)
    st = [np.array([[0, 0, 5, 5, 0]])]
    rgb = [np.zeros((8, 8, 3), np.uint8)]
    with pytest.raises(NotImplementedError, match="mask_pool_size"):
        M.crop_modalities({"rgb": rgb}, st, 4, mask_pool_size=2)
    with pytest.raises(ValueError, match="sam_instance"):
        M.crop_modalities({"rgb": rgb, "sam_instance": rgb}, st, 4)
    with pytest.raises(ValueError, match="2 samples for 1 settings"):
        M.crop_modalities({"rgb": rgb, "depth": [np.zeros((8, 8), np.uint16)] * 2}, st, 4)
    with pytest.raises(ValueError, match="no modalities"):
        M.crop_modalities({}, st, 4)
    assert np.array_equal(M._mask_u8(np.array([[True, False]]), 0), np.array([[255, 0]], np.uint8))
    with pytest.raises(TypeError, match="mask_valid 0"):
        M._mask_u8(np.zeros((2, 2), np.float32), 0)


def test_library_refuses_bad_arguments_before_any_launch():
    """fm_pil_crop_resize16 validates the host copy of every job first, fm_depth_standardize its rank range: -1 and nothing is launched (the
    device pointers are never dereferenced).  Every job also carries a wrong first workgroup, the last field checked, so that none of these
    calls can reach a launch whatever the checks in front of it decide."""
    from fourm.hip import _lib as L
    fake = ctypes.c_void_p(1 << 20)

    def call(edit, S=8):
        j = (L.PilCropJob * 1)()
        j[0].H, j[0].W, j[0].h, j[0].w, j[0].taps_w, j[0].taps_h, j[0].tab_h, j[0].blk_rows = 20, 30, 5, 6, 1, 1, 8 * 4, 7
        edit(j[0])
        rc = L.pil_crop_resize16(j, fake, 1, fake, 2 * 20 * 30, fake, 2 * 8 * 4, fake, 2 * 5 * S, S, fake, None, 1, None)
        return rc, L.lib.fm_last_error().decode()

    for edit, msg in [(lambda j: setattr(j, "top", 16), "leaves the 20 x 30 image"), (lambda j: setattr(j, "left", 25), "leaves the 20 x 30 image"),
                      (lambda j: setattr(j, "h", 0), "leaves"), (lambda j: setattr(j, "src_off", 2), "outside the source buffer"),
                      (lambda j: setattr(j, "src_off", 1), "outside the source buffer"), (lambda j: setattr(j, "tab_w", 34), "tables outside"),
                      (lambda j: setattr(j, "tab_h", 31), "tables outside"), (lambda j: setattr(j, "mid_off", 2), "outside the scratch"),
                      (lambda j: setattr(j, "out_slot", 1), "output slot"), (lambda j: setattr(j, "flip", 2), "flip"), (lambda j: None, "first workgroups")]:
        rc, err = call(edit)
        assert rc == -1 and msg in err, (rc, err)
    for n, lo, hi in [(1, 0, 1), (4, 0, 1), (4, -1, 3), (4, 0, 5), (16, 3, 4), ((1 << 28) + 1, 0, 8)]:
        assert L.depth_standardize(fake, 1, n, lo, hi, fake, fake, None) == -1, (n, lo, hi)
        assert "fm_depth_standardize" in L.lib.fm_last_error().decode()
    assert L.depth_standardize(fake, 1, 16, 1, 14, None, None, None) == -1


def test_abi_additions_are_declared_exported_and_built():
    from fourm.hip import _lib
    import importlib.util
    header = _header()
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib.EXPORTS and hasattr(_lib.lib, name), name
    assert _lib.lib.fm_abi_version() == _lib.ABI_VERSION == int(re.search(r"#define FM_ABI_VERSION (\d+)", header).group(1)) == 11
    assert "Pillow-exact 16-bit depth crops" in header
    assert ctypes.sizeof(_lib.PilCropJob) == 88          # the 8-bit job struct is reused as it is (its layout is pinned by tests/test_pil_crops_cpu.py)
    spec = importlib.util.spec_from_file_location("build_ext", os.path.join(ROOT, "ml-4m_amd", "build_ext.py"))
    be = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(be)
    assert "pil_resize16.hip" in be.SOURCES and "-ffp-contract=off" in be.EXTRA_FLAGS["pil_resize16.hip"]
