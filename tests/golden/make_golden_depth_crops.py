#!/usr/bin/env python3
"""Golden fixture of the Pillow-exact 16-bit depth crops (tests/golden/depth_crops.npz): seeded uint16 sources, crop settings and what Pillow
itself returns for a mode-I;16 image, ``img.crop(box).resize((S, S), resample)`` followed by the flip; and crops with what upstream's own
``DepthTransform.truncated_depth_standardization`` (an upstream checkout, imported through tests/golden/ref_stubs.py, on the CPU) returns
for ``torch.Tensor(crop / (2 ** 16 - 1.0))``.  Needs Pillow and the checkout (Pillow's version is recorded); the tests need only the file.

The script asserts that the restatement (tests/pil_resize16_util.py) gives Pillow's values on every case and that a plain 0 .. 65535 clamp
would not on the saturated-edge cases (nor the 8-bit path's repeated-addition nearest index on the nearest_*_to_* cases), and it MEASURES
how far upstream's fp32 sums take its standardised output from the restatement's exact statistics:  std_bound_units = max over the cases of  max|upstream - restatement| * s / (2^-24 * max|x|),  s = sqrt(var32 + 1e-6):
the error of upstream's mean and deviation in units of half an fp32 ulp of the largest input, before 1 / s amplifies it.

    src_<k>        uint16 (H, W)    source images, none larger than 96 x 80
    cases          int32 (n, 8)     rows of (source, top, left, h, w, flip, S, filter); filter 0 nearest, 1 bilinear, 2 bicubic (FM_PIL_*)
    names          str (n)
    out_<i>        uint16 (S, S)    Pillow's result of case i
    std_in_<i>     uint16 (S, S)    crops for the standardisation;  std_names str
    std_out_<i>    float32 (S, S)   upstream's result
    std_bound_units, pillow_version, torch_version

    python tests/golden/make_golden_depth_crops.py [--check]"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import pil_resize16_util as U  # noqa: E402
from tests import pil_resize_util as U8  # noqa: E402

PATH = os.path.join(HERE, "depth_crops.npz")
PLAIN_CLAMP_DIFFERS = ("edge_up_bicubic", "edge_up_bicubic_flip", "checkerboard_up")


def sources():
    rng = np.random.default_rng(20240611)
    yy, xx = np.mgrid[0:48, 0:48]
    edge = np.zeros((40, 48), np.uint16)
    edge[:, :24] = 65535          # a saturated region next to zeros
    edge[30:] = 0
    band = (30000 + (np.add.outer(np.arange(64), np.arange(60)) // 3) % 50 + rng.integers(0, 3, (64, 60))).astype(np.uint16)
    return [
        rng.integers(0, 65536, (80, 96), dtype=np.uint16),                       # 0: full-range noise
        edge,                                                                    # 1: 65535 | 0
        band,                                                                    # 2: a narrow band of depth levels
        (((yy // 2 + xx // 2) % 2) * 65535).astype(np.uint16),                   # 3: 0 / 65535 checkerboard, 2-pixel squares
        rng.integers(0, 65536, (96, 40), dtype=np.uint16),                       # 4: tall
    ]


def cases(src):
    rng = np.random.default_rng(12)
    out = []

    def add(name, k, box, flip, S, filt):
        out.append((name, (k, *box, flip, S, U.FILTERS.index(filt))))

    for filt in U.FILTERS:          # every filter x both flips, random boxes, at several sizes
        for k, S in ((0, 16), (2, 33), (4, 3)):
            H, W = src[k].shape
            for flip in (0, 1):
                h, w = int(rng.integers(9, H + 1)), int(rng.integers(9, W + 1))
                add(f"{filt}_src{k}_S{S}_flip{flip}", k, (int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1)), h, w), flip, S, filt)
    add("edge_up_bicubic", 1, (10, 20, 6, 8), 0, 33, "bicubic")              # upscale over the 65535 | 0 edge: the per-byte clamp decides
    add("edge_up_bicubic_flip", 1, (26, 18, 8, 11), 1, 16, "bicubic")        # both edges, flipped
    add("edge_up_bilinear", 1, (10, 20, 6, 8), 0, 33, "bilinear")
    add("checkerboard_up", 3, (1, 3, 24, 20), 0, 64, "bicubic")
    add("checkerboard_down", 3, (0, 0, 48, 48), 1, 20, "bicubic")
    for filt in U.FILTERS:
        add(f"down_10x_{filt}", 0, (0, 0, 80, 96), 1, 8, filt)               # 80 x 96 -> 8: windows of 40 and 48 taps
        add(f"up_5x7_{filt}", 0, (10, 20, 5, 7), 1, 16, filt)                # taps clipped at both borders
        add(f"h_eq_S_{filt}", 0, (3, 5, 16, 41), 0, 16, filt)
        add(f"w_eq_S_{filt}", 0, (3, 5, 41, 16), 1, 16, filt)
        add(f"both_eq_S_{filt}", 0, (7, 9, 16, 16), 1, 16, filt)
        add(f"one_wide_{filt}", 4, (5, 17, 60, 1), 0, 16, filt)
        add(f"one_high_{filt}", 0, (33, 4, 1, 70), 1, 16, filt)
        add(f"S2_{filt}", 0, (7, 9, 33, 21), 1, 2, filt)
    add("nearest_8_to_7", 0, (2, 3, 15, 8), 0, 7, "nearest")                 # axes on which the 8-bit scaler's repeated-addition index differs
    add("nearest_15_to_7_flip", 0, (11, 40, 8, 15), 1, 7, "nearest")
    add("whole_image", 0, (0, 0, 80, 96), 0, 64, "bicubic")
    add("band_down", 2, (0, 0, 64, 60), 0, 16, "bicubic")
    return out


def std_cases():
    rng = np.random.default_rng(13)
    out = []
    for S in (2, 3, 16, 33):
        out.append((f"uniform_S{S}", rng.integers(0, 65536, (S, S), dtype=np.uint16)))
        sat = rng.integers(0, 65536, (S, S), dtype=np.uint16)
        sat[:, :(S + 1) // 2] = 65535          # half the crop saturated and rows of zeros (a fifth of the crop, one row is below the
        sat[:(S + 4) // 5] = 0                 # 10 % from S = 10 on): ties straddle both rank boundaries
        out.append((f"saturated_S{S}", sat))
        out.append((f"constant_S{S}", np.full((S, S), 12345, np.uint16)))
        out.append((f"band50_S{S}", (40000 + rng.integers(0, 50, (S, S))).astype(np.uint16)))
    run = np.full((16, 16), 777, np.uint16)          # both rank boundaries inside one value's run of ties
    run.reshape(-1)[:9] = 5
    run.reshape(-1)[-9:] = 60000
    out.append(("one_run_S16", run))
    two = np.full((33, 33), 300, np.uint16)          # the boundaries in two runs that share a high byte
    two[:16] = 290
    out.append(("two_runs_S33", two))
    return out


def upstream_standardize():
    import torch
    from tests.golden import ref_stubs
    ref_stubs.install()
    from fourm.data.modality_transforms import DepthTransform          # the checkout's, not this package's
    assert ref_stubs.REFERENCE_ROOT in sys.modules["fourm.data.modality_transforms"].__file__

    def run(crop):
        x = torch.Tensor(crop / (2 ** 16 - 1.0)).unsqueeze(0)
        return DepthTransform.truncated_depth_standardization(x)[0].numpy()
    return run, torch.__version__


def build():
    import PIL
    src = sources()
    assert all(s.shape[0] <= 96 and s.shape[1] <= 96 and s.dtype == np.uint16 for s in src)
    fx = {f"src_{k}": s for k, s in enumerate(src)}
    cs = cases(src)
    fx["cases"] = np.asarray([c[1] for c in cs], np.int32)
    fx["names"] = np.asarray([c[0] for c in cs])
    fx["pillow_version"] = np.asarray(PIL.__version__)
    for i, (name, (k, top, left, h, w, flip, S, f)) in enumerate(cs):
        ref = U.pillow_crop_resize16(src[k], (top, left, h, w, flip), S, U.FILTERS[f])
        mine = U.crop_resize16(src[k], (top, left, h, w, flip), S, U.FILTERS[f])
        assert np.array_equal(ref, mine), f"{name}: the restatement differs from Pillow {PIL.__version__}"
        if name.startswith("nearest_") and "_to_" in name:
            t8 = (U8.nearest_index(h, S), U8.nearest_index(w, S))
            assert not (np.array_equal(t8[0], U.nearest_index16(h, S)) and np.array_equal(t8[1], U.nearest_index16(w, S))), name
            wrong = src[k][top:top + h, left:left + w][t8[0]][:, t8[1]]
            assert not np.array_equal(wrong[:, ::-1] if flip else wrong, ref), f"{name}: the repeated-addition index gives Pillow's values as well"
        if name in PLAIN_CLAMP_DIFFERS:
            plain = U.crop_resize16(src[k], (top, left, h, w, flip), S, U.FILTERS[f], plain_clamp=True)
            assert not np.array_equal(plain, ref), f"{name}: a plain 16-bit clamp gives Pillow's values, the case does not show the per-byte clamp"
        fx[f"out_{i}"] = ref
    run, tv = upstream_standardize()
    fx["torch_version"] = np.asarray(tv)
    sc = std_cases()
    fx["std_names"] = np.asarray([c[0] for c in sc])
    units = 0.0
    for i, (name, crop) in enumerate(sc):
        ref = run(crop)
        mine, (mean32, var32) = U.standardize(crop)
        s = float(np.sqrt(np.float32(var32 + np.float32(1e-6))))
        u = float(np.max(np.abs(ref.astype(np.float64) - mine.astype(np.float64)))) * s / (2.0 ** -24 * float(U.unit_f32(crop).max()))
        print(f"{name:20s} max|upstream - restatement| {np.max(np.abs(ref - mine)):.3e}   s {s:.3e}   units {u:.3f}")
        units = max(units, u)
        fx[f"std_in_{i}"] = crop
        fx[f"std_out_{i}"] = ref.astype(np.float32)
    fx["std_bound_units"] = np.asarray(units, np.float64)
    print(f"std_bound_units = {units:.4f}")
    return fx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="compare with the committed fixture instead of writing it")
    a = ap.parse_args()
    fx = build()
    if a.check:
        old = np.load(PATH)
        assert sorted(old.files) == sorted(fx), sorted(set(old.files) ^ set(fx))
        loose = ("pillow_version", "torch_version", "std_bound_units")          # upstream's fp32 sums may differ with torch's version and threads
        bad = [k for k in fx if k not in loose and not k.startswith("std_out_") and not np.array_equal(old[k], fx[k])]
        assert not bad, bad
        print(f"{PATH}: {len(fx['cases'])} cases agree (fixture made with Pillow {old['pillow_version']}, this is {fx['pillow_version']}); "
              f"std_bound_units recorded {float(old['std_bound_units']):.4f}, now {float(fx['std_bound_units']):.4f}")
        return
    np.savez_compressed(PATH, **fx)
    print(f"wrote {PATH}: {len(fx['cases'])} + {len(fx['std_names'])} cases, {os.path.getsize(PATH)} bytes, Pillow {fx['pillow_version']}")


if __name__ == "__main__":
    main()
