"""Pillow-exact crops without a GPU: the numpy restatement against Pillow (live and through the fixture), fm_pil_axis_table against the
restatement, the crop settings, the job struct's layout, the ABI additions, and the parser and refusals of save_vq_tokens.py.  The kernels are
tested on the GPU (tests/test_pil_crops_gpu.py).

tests/golden/save_vq_tokens_flags.json records the flags of upstream's save_vq_tokens.py (name -> default, type, action), read off its source
with ``upstream_flags``:  python -c "from tests.test_pil_crops_cpu import write_flags; write_flags('<checkout>/save_vq_tokens.py')"."""
import ast
import ctypes
import json
import os
import random
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import pil_resize_util as U
from tests.golden.ref_stubs import REFERENCE_ROOT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "pil_crops.npz")
FLAGS = os.path.join(ROOT, "tests", "golden", "save_vq_tokens_flags.json")
REFERENCE = os.path.join(REFERENCE_ROOT, "save_vq_tokens.py")          # an upstream checkout, where there is one
NEW = ["fm_pil_axis_table", "fm_pil_crop_resize"]
P32 = ctypes.POINTER(ctypes.c_int32)


def _header():
    return open(os.path.join(ROOT, "include", "fourm_hip.h")).read()


def _c_table(n, S, fid):
    from fourm.hip import _lib as L
    taps = L.pil_axis_table(n, S, fid, None, None, None)
    assert taps >= 1, L.lib.fm_last_error()
    st, ct, cf = np.zeros(S, np.int32), np.zeros(S, np.int32), np.zeros((S, taps), np.int32)
    assert L.pil_axis_table(n, S, fid, st.ctypes.data_as(P32), ct.ctypes.data_as(P32), cf.ctypes.data_as(P32)) == taps
    return st, ct, cf


def _random_case(rng, it):
    C = int(rng.choice([1, 3, 4]))
    H, W = int(rng.integers(1, 97)), int(rng.integers(1, 97))
    img = rng.integers(0, 256, (H, W, C), dtype=np.uint8) if it % 3 else (rng.integers(0, 2, (H, W, C)) * 255).astype(np.uint8)          # every third saturated
    h, w = int(rng.integers(1, H + 1)), int(rng.integers(1, W + 1))
    setting = (int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1)), h, w, int(rng.integers(0, 2)))
    return img, setting, int(rng.choice([1, 2, 7, 8, 16, 24, 33])), U.FILTERS[int(rng.integers(0, 3))]


def test_restatement_equals_pillow_on_random_cases():
    pytest.importorskip("PIL")
    rng = np.random.default_rng(0)
    for it in range(300):
        img, setting, S, filt = _random_case(rng, it)
        assert np.array_equal(U.crop_resize(img, setting, S, filt, (0,)), U.pillow_crop_resize(img, setting, S, filt, (0,))), (img.shape, setting, S, filt)
    for n, S in [(640, 224), (479, 224), (333, 224), (1000, 7)]:          # nearest on longer axes: the index table through a ramp image
        ramp = (np.arange(n) % 251).astype(np.uint8)[None, :, None].repeat(3, 0)
        assert np.array_equal(U.pillow_crop_resize(ramp, (0, 0, 3, n, 0), S, "nearest")[0, :, 0], ramp[0, U.nearest_index(n, S), 0]), (n, S)


def test_restatement_equals_the_fixture():
    fx = np.load(GOLDEN)
    assert len(fx["cases"]) >= 36 and str(fx["pillow_version"])
    src = [fx[f"src_{k}"] for k in range(6)]
    assert all(s.shape[0] <= 96 and s.shape[1] <= 96 for s in src)
    seen = set()
    for i, (k, top, left, h, w, flip, S, f, inv) in enumerate(fx["cases"].tolist()):
        got = U.crop_resize(src[k], (top, left, h, w, flip), S, U.FILTERS[f], (0,) if inv else ())
        assert np.array_equal(got, fx[f"out_{i}"]), str(fx["names"][i])
        seen.add((f, src[k].shape[2], flip))
    assert seen >= {(f, C, flip) for f in range(3) for C in (1, 3, 4) for flip in (0, 1)}
    i = fx["names"].tolist().index("checkerboard_up")          # both clamps are hit, and by overshoot
    k, top, left, h, w, flip, S, f, inv = fx["cases"][i].tolist()
    stats = {}
    U.crop_resize(src[k], (top, left, h, w, flip), S, U.FILTERS[f], (), stats)
    assert stats["lo"] < 0 and stats["hi"] > 255 and fx[f"out_{i}"].min() == 0 and fx[f"out_{i}"].max() == 255


def test_axis_table_equals_the_restatement_entry_for_entry():
    rng = np.random.default_rng(1)
    pairs = [(int(rng.integers(1, 700)), int(rng.integers(1, 260))) for _ in range(150)]
    pairs += [(5, 16), (7, 16), (90, 8), (17, 8), (16, 16), (1, 1), (1, 9), (9, 1), (640, 224), (480, 224), (2, 3), (3, 2), (4000, 224)]
    differs = [(n, S) for n in range(1, 400) for S in (7, 24, 33, 224) if not np.array_equal(U.nearest_index(n, S), U.nearest_index_closed_form(n, S))]
    assert len(differs) >= 10          # the axes on which the closed-form nearest index is not Pillow's
    for n, S in pairs + differs[:40]:
        for fid, filt in enumerate(U.FILTERS):
            st, ct, cf = _c_table(n, S, fid)
            s2, c2, k2 = U.axis_table(n, S, filt)
            assert cf.shape == k2.shape and np.array_equal(st, s2) and np.array_equal(ct, c2) and np.array_equal(cf, k2), (n, S, filt)
            assert np.all(st >= 0) and np.all(ct >= 1) and np.all(st + ct <= n)
    for n, S in differs[:40]:
        assert not np.array_equal(_c_table(n, S, 0)[0], U.nearest_index_closed_form(n, S)), (n, S)
    from fourm.hip import _lib as L
    assert L.pil_axis_table(0, 4, 1, None, None, None) == -1 and L.pil_axis_table(4, 4, 3, None, None, None) == -1
    assert L.pil_axis_table(1 << 20, 2, 2, None, None, None) == -1 and b"FM_PIL_MAX_TAPS" in L.lib.fm_last_error()


def test_pil_axis_table_cache_layout():
    from fourm.data import crops
    tab, taps = crops.pil_axis_table(90, 8, "bicubic")
    st, ct, cf = U.axis_table(90, 8, "bicubic")
    assert taps == cf.shape[1] and tab.dtype == np.int32 and np.array_equal(tab, np.concatenate([st, ct, cf.reshape(-1)]))
    assert crops.pil_axis_table(90, 8, "bicubic")[0] is tab


def test_crop_settings():
    from fourm.data import crops
    assert crops.center_crop_settings(480, 640) == (0, 80, 480, 480) and crops.center_crop_settings(641, 480) == (80, 0, 480, 480)
    assert crops.center_crop_settings(7, 7) == (0, 0, 7, 7)
    for H, W, n, smin in [(480, 640, 10, 0.2), (97, 31, 6, 0.8), (33, 500, 12, 0.2), (1, 1, 3, 0.5)]:
        torch.manual_seed(5)
        random.seed(5)
        a = crops.make_crop_settings(H, W, n, smin)
        torch.manual_seed(5)
        random.seed(5)
        b = crops.make_crop_settings(H, W, n, smin)
        assert np.array_equal(a, b) and a.shape == (n, 5) and np.issubdtype(a.dtype, np.integer)
        assert tuple(a[0]) == (*crops.center_crop_settings(H, W), 0)
        top, left, h, w, flip = a.T
        assert np.all(top >= 0) and np.all(left >= 0) and np.all(h >= 1) and np.all(w >= 1) and np.all(top + h <= H) and np.all(left + w <= W)
        assert set(flip.tolist()) <= {0, 1}
    torch.manual_seed(9)
    random.seed(9)
    H, W = 480, 640
    rows = np.array([crops.random_crop_settings(H, W, scale=(0.2, 1.0), ratio=(0.75, 1.3333)) for _ in range(300)])
    top, left, h, w, flip = rows.T
    # area and ratio are drawn in range, then w and h are rounded to integers: half a pixel each, a relative 0.5 / w + 0.5 / h to first
    # order; twice that bounds the second-order terms and the fp32 rounding of the draws
    area, ratio = h * w / (H * W), w / h
    slack = 1.0 / w + 1.0 / h
    assert np.all(area >= 0.2 * (1 - slack)) and np.all(area <= 1.0)
    assert np.all(ratio >= 0.75 * (1 - slack)) and np.all(ratio <= 1.3333 * (1 + slack))
    assert 0 < flip.sum() < 300 and len({tuple(r) for r in rows.tolist()}) > 250
    # an image no ratio in range fits: ten failed attempts, then the central fallback at the nearest allowed ratio
    torch.manual_seed(1)
    assert crops.random_crop_settings(10, 1000, scale=(0.9, 1.0), hflip=0.0) == (0, 493, 10, 13, 0)
    assert crops.random_crop_settings(1000, 10, scale=(0.9, 1.0), hflip=0.0) == (493, 0, 13, 10, 0)


def test_crop_resize_refuses_before_anything_runs():
    from fourm.data import crops
    img = np.zeros((20, 30, 3), np.uint8)
    for bad in ([0, 0, 21, 5, 0], [0, 26, 5, 5, 0], [-1, 0, 5, 5, 0], [0, 0, 0, 5, 0], [18, 0, 3, 5, 1], [0, 0, 5, 5, 2]):
        with pytest.raises(ValueError, match="leaves the 20 x 30 image|flip"):
            crops.crop_resize([img], [np.array([bad])], 8)
    with pytest.raises(ValueError, match="resample"):
        crops.crop_resize([img], [np.array([[0, 0, 5, 5, 0]])], 8, resample="lanczos")
    with pytest.raises(ValueError, match="int64"):
        crops.crop_resize([img], [np.array([[0, 0, 5, 5, 0]])], 8, out="int64")
    with pytest.raises(ValueError, match="channels"):
        crops.crop_resize([img, img[:, :, :1]], [np.array([[0, 0, 5, 5, 0]])] * 2, 8)
    with pytest.raises(TypeError, match="uint8"):
        crops.crop_resize([img.astype(np.float32)], [np.array([[0, 0, 5, 5, 0]])], 8)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU path"):
            crops.crop_resize([img], [np.array([[0, 0, 5, 5, 0]])], 8)
    lut = crops.normalize_lut(3, (0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
    want = (torch.arange(256, dtype=torch.float32) / 255 - 0.456) / 0.224
    assert lut.shape == (3, 256) and lut.dtype == torch.float32 and torch.equal(lut[1], want)


def test_library_refuses_a_bad_job_list_before_any_launch():
    """fm_pil_crop_resize validates the host copy of every job first: with a job that cannot be accepted it returns -1 and nothing is launched
    (the device pointers below are never dereferenced - there may be no device at all).  Every job here also carries a wrong first workgroup,
    the last field checked, so that none of these calls can reach a launch whatever the checks in front of it decide."""
    from fourm.hip import _lib as L
    fake = ctypes.c_void_p(1 << 20)

    def call(edit, C=3, S=8, out_i64=None):
        j = (L.PilCropJob * 1)()
        j[0].H, j[0].W, j[0].h, j[0].w, j[0].taps_w, j[0].taps_h, j[0].tab_h, j[0].blk_rows = 20, 30, 5, 6, 1, 1, 8 * 3, 7
        edit(j[0])
        rc = L.pil_crop_resize(j, fake, 1, fake, 20 * 30 * C, fake, 2 * 8 * 3, fake, 5 * S * C, C, S, 0, None, None if out_i64 else fake, None, out_i64, 1, None)
        return rc, L.lib.fm_last_error().decode()

    for edit, msg in [(lambda j: setattr(j, "top", 16), "leaves the 20 x 30 image"), (lambda j: setattr(j, "left", 25), "leaves the 20 x 30 image"),
                      (lambda j: setattr(j, "h", 0), "leaves"), (lambda j: setattr(j, "src_off", 1), "outside the source buffer"),
                      (lambda j: setattr(j, "tab_w", 25), "tables outside"), (lambda j: setattr(j, "mid_off", 1), "outside the scratch"),
                      (lambda j: setattr(j, "out_slot", 1), "output slot"), (lambda j: setattr(j, "blk_cols", 1), "first workgroups"),
                      (lambda j: setattr(j, "flip", 2), "flip")]:
        rc, err = call(edit)
        assert rc == -1 and msg in err, (rc, err)
    assert call(lambda j: None, C=5)[0] == -1 and call(lambda j: None, out_i64=fake)[0] == -1


def test_abi_additions_are_declared_exported_and_built():
    from fourm.hip import _lib
    import importlib.util
    header = _header()
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib.EXPORTS and hasattr(_lib.lib, name), name
    assert _lib.lib.fm_abi_version() == _lib.ABI_VERSION == int(re.search(r"#define FM_ABI_VERSION (\d+)", header).group(1))
    for name, val in dict(FM_PIL_NEAREST=_lib.PIL_NEAREST, FM_PIL_BILINEAR=_lib.PIL_BILINEAR, FM_PIL_BICUBIC=_lib.PIL_BICUBIC, FM_PIL_MAX_TAPS=_lib.PIL_MAX_TAPS).items():
        assert re.search(rf"{name}\s*(=|\s)\s*{val}\b", header), name
    assert U.FILTERS == ("nearest", "bilinear", "bicubic")
    spec = importlib.util.spec_from_file_location("build_ext", os.path.join(ROOT, "ml-4m_amd", "build_ext.py"))
    be = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(be)
    assert "pil_resize.hip" in be.SOURCES and "-ffp-contract=off" in be.EXTRA_FLAGS["pil_resize.hip"]


def test_crop_job_mirror_matches_the_header_layout(tmp_path):
    """sizeof and every field offset of fm_pil_crop_job as gcc lays it out against the ctypes mirror (the method of
    tests/test_model_cpu.py::test_ctypes_mirrors_match_the_header_layout)."""
    from fourm.hip import _lib
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    body = re.search(r"typedef struct fm_pil_crop_job \{(.*?)\} fm_pil_crop_job;", _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.search(r"([A-Za-z_][A-Za-z0-9_]*)\s*$", d.strip()).group(1) for d in body.split(";") if d.strip()]
    assert names == [f[0] for f in _lib.PilCropJob._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "fourm_hip.h"', 'int main(void) {', '  printf("size %zu\\n", sizeof(fm_pil_crop_job));']
    lines += [f'  printf("{n} %zu\\n", offsetof(fm_pil_crop_job, {n}));' for n in names] + ["  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert ctypes.sizeof(_lib.PilCropJob) == int(out["size"]) == 88
    for n in names:
        assert getattr(_lib.PilCropJob, n).offset == int(out[n]), n


# ---- the script -------------------------------------------------------------------------------------------------------------------------------
def upstream_flags(path):
    """{flag: [default, type name, action]} of every parser.add_argument(...) in a script, parser.set_defaults applied; read off the source."""
    flags, dests = {}, {}
    for node in ast.walk(ast.parse(open(path).read())):
        if not (isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute)):
            continue
        kw = {k.arg: k.value for k in node.keywords}
        if node.func.attr == "add_argument":
            name = ast.literal_eval(node.args[0])
            action = ast.literal_eval(kw["action"]) if "action" in kw else None
            default = ast.literal_eval(kw["default"]) if "default" in kw else {"store_true": False, "store_false": True}.get(action)
            flags[name] = [default, kw["type"].id if "type" in kw else None, action]
            dests[ast.literal_eval(kw["dest"]) if "dest" in kw else name.lstrip("-")] = name
        elif node.func.attr == "set_defaults":
            for k, v in kw.items():
                for name, spec in flags.items():
                    if dests.get(k) == name or name.lstrip("-") == k:
                        spec[0] = ast.literal_eval(v)
    return flags


def write_flags(path):
    with open(FLAGS, "w") as f:
        json.dump(upstream_flags(path), f, indent=1, sort_keys=True)
        f.write("\n")


def _our_flags():
    """The same description read off this package's parser object: {flag: [default, type name, action]}."""
    import argparse
    import save_vq_tokens as S
    kinds = {argparse._StoreTrueAction: "store_true", argparse._StoreFalseAction: "store_false", argparse._StoreAction: None}
    flags = {}
    for act in S.build_parser()._actions:
        if type(act) in kinds:
            flags[act.option_strings[0]] = [act.default, act.type.__name__ if act.type is not None else None, kinds[type(act)]]
    return flags, S


def test_parser_takes_upstreams_flags_and_defaults():
    ours, S = _our_flags()
    want = json.load(open(FLAGS))
    assert len(want) >= 25 and {"--n_crops", "--min_crop_scale", "--input_size", "--resample_mode", "--batch_size", "--batch_size_dataloader",
                                "--force_load_crop", "--dryrun", "--folder_suffix", "--tokenizer_id", "--tokenizers_root"} <= set(want)
    assert set(ours) - set(want) == {"--tokenizer_ckpt"}
    conv = {"int": int, "float": float, "str": str}
    for name, (default, typ, action) in want.items():
        if isinstance(default, str) and typ is not None:          # argparse passes a string default through the type (upstream's --n_crops '1')
            default = conv[typ](default)
        assert ours[name] == [default, typ, action], (name, ours[name], [default, typ, action])
    a = S.get_args([])
    assert a.n_crops == 1 and isinstance(a.n_crops, int) and a.min_crop_scale == 0.8 and a.input_size == 224 and a.resample_mode is None and a.task == "rgb"
    assert a.pin_mem is True and a.tokenizer_ckpt is None and a.folder_suffix == "dvae_BUa_224" and a.batch_size == a.batch_size_dataloader == 64
    a = S.get_args("--task normal --n_crops 10 --min_crop_scale 0.2 --force_load_crop --dryrun --no_pin_mem --resample_mode bilinear".split())
    assert (a.task, a.n_crops, a.min_crop_scale, a.force_load_crop, a.dryrun, a.pin_mem, a.resample_mode) == ("normal", 10, 0.2, True, True, False, "bilinear")


@pytest.mark.skipif(not os.path.exists(REFERENCE), reason="needs_ref: no upstream checkout on this machine")
def test_recorded_flags_are_the_reference_checkouts():
    assert upstream_flags(REFERENCE) == json.load(open(FLAGS))


def test_refusals_launch_nothing(monkeypatch):
    import save_vq_tokens as S
    import fourm.data.crops as crops
    import fourm.vq as vq

    def boom(*a, **k):
        raise AssertionError("reached past the refusal")
    for mod, name in ((crops, "crop_resize"), (vq, "get_image_tokenizer"), (vq, "tokenize_sub_batches"), (S, "find_samples"), (S, "load_tokenizer")):
        monkeypatch.setattr(mod, name, boom)
    for argv, msg in [("--task depth", "16-bit"), ("--task sam_instance", "SAM instances"), ("--task CLIP-B16", "feature extractor"),
                      ("--task DINOv2-B14", "feature extractor"), ("--task DINOv2-B14-global", "feature extractor"), ("--task ImageBind-H14", "feature extractor"),
                      ("--task rgb --mask_value 0.0", "--mask_value"), ("--task rgb --corrupt_samples_log x.log", "--corrupt_samples_log"),
                      ("--task human_poses", "not supported")]:
        with pytest.raises(NotImplementedError, match=msg):
            S.main(S.get_args(argv.split()))
    with pytest.raises(ValueError, match="--resample_mode lanczos"):
        S.main(S.get_args("--resample_mode lanczos".split()))
    a = S.get_args([])
    assert S.task_config(a) == ("RGB", (0.5, 0.5, 0.5), (0.5, 0.5, 0.5), (), "float32", None, 0)
    assert S.task_config(S.get_args("--task normal --resample_mode bilinear".split()))[3:6] == ((0,), "float32", "bilinear")
    assert S.task_config(S.get_args("--task semseg_coco --resample_mode bicubic".split())) == ("P", None, None, (), "int64", "nearest", 1)
    assert S.task_config(S.get_args("--task semseg_hypersim".split()))[-1] == 0
    assert S.MAX_DECODE_THREADS == 16 and "cpu_count" not in open(S.__file__).read()
