#!/usr/bin/env python3
"""Golden fixture of the Pillow-exact crops (tests/golden/pil_crops.npz): seeded source images, crop settings and what Pillow itself returns
for ``np.asarray(img.crop(box).resize((S, S), resample))`` followed by the flip.  Needs Pillow (its version is recorded in the file); the GPU
box needs only the file.  The script asserts that the numpy restatement (tests/pil_resize_util.py) gives the same bytes on every case, and
that the checkerboard case drives the bicubic accumulator past both clamps.

    src_<k>      uint8 (H, W, C)   source images, none larger than 96 x 96
    cases        int32 (n, 9)      rows of (source, top, left, h, w, flip, S, filter, invert channel 0 on flip); filter 0 nearest, 1 bilinear,
                                   2 bicubic (FM_PIL_*)
    names        str (n)
    out_<i>      uint8 (S, S, C)   Pillow's result of case i
    pillow_version

    python tests/golden/make_golden_pil_crops.py [--check]"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import pil_resize_util as U  # noqa: E402

PATH = os.path.join(HERE, "pil_crops.npz")


def sources():
    rng = np.random.default_rng(20240607)
    yy, xx = np.mgrid[0:48, 0:48]
    return [
        rng.integers(0, 256, (80, 96, 3), dtype=np.uint8),                                        # 0: RGB noise
        rng.integers(0, 256, (96, 60, 1), dtype=np.uint8),                                        # 1: one channel
        rng.integers(0, 256, (64, 64, 4), dtype=np.uint8),                                        # 2: four plain planes
        np.repeat((((yy // 2 + xx // 2) % 2) * 255).astype(np.uint8)[:, :, None], 3, axis=2),     # 3: 0 / 255 checkerboard, 2-pixel squares
        rng.integers(0, 256, (90, 40, 3), dtype=np.uint8),                                        # 4: tall, for 90 x 17 -> 8
        rng.integers(0, 20, (50, 70, 1), dtype=np.uint8),                                         # 5: a class map
    ]


def cases(src):
    rng = np.random.default_rng(11)
    out = []

    def add(name, k, box, flip, S, filt, invert=0):
        out.append((name, (k, *box, flip, S, U.FILTERS.index(filt), invert)))

    for filt in U.FILTERS:          # every filter x C = 1, 3, 4 x both flips, random boxes
        for k in (1, 0, 2):
            H, W, C = src[k].shape
            for flip in (0, 1):
                h, w = int(rng.integers(9, H + 1)), int(rng.integers(9, W + 1))
                add(f"{filt}_C{C}_flip{flip}", k, (int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1)), h, w), flip, 16, filt)
    for filt in U.FILTERS:
        add(f"up_5x7_{filt}", 0, (10, 20, 5, 7), 1, 16, filt)                # taps clipped at both borders
    add("down_90x17_bicubic", 4, (0, 11, 90, 17), 0, 8, "bicubic")           # wide tables
    add("down_90x17_bilinear", 4, (0, 11, 90, 17), 1, 8, "bilinear")
    add("h_eq_S", 0, (3, 5, 16, 41), 0, 16, "bicubic")
    add("w_eq_S", 0, (3, 5, 41, 16), 1, 16, "bicubic")
    add("h_eq_S_bilinear", 2, (0, 1, 16, 23), 1, 16, "bilinear")
    add("edge_top", 0, (0, 13, 30, 40), 0, 16, "bicubic")
    add("edge_left", 0, (9, 0, 30, 40), 1, 16, "bilinear")
    add("edge_bottom", 0, (50, 13, 30, 40), 0, 16, "bicubic")
    add("edge_right", 0, (9, 56, 30, 40), 1, 16, "bicubic")
    add("whole_image", 0, (0, 0, 80, 96), 0, 24, "bicubic")
    for filt in U.FILTERS:
        add(f"S1_{filt}", 0, (7, 9, 33, 21), 1, 1, filt)
    add("checkerboard_up", 3, (1, 3, 24, 20), 0, 33, "bicubic")              # overshoot hits both clamps
    add("checkerboard_down", 3, (0, 0, 48, 48), 1, 20, "bicubic")
    add("normal_invert_flip", 0, (4, 8, 50, 60), 1, 16, "bicubic", 1)
    add("normal_invert_noflip", 0, (4, 8, 50, 60), 0, 16, "bicubic", 1)
    add("semseg_nearest", 5, (2, 3, 45, 61), 1, 16, "nearest")
    add("semseg_nearest_up", 5, (2, 3, 11, 13), 0, 32, "nearest")
    return out


def build():
    import PIL
    src = sources()
    fx = {f"src_{k}": s for k, s in enumerate(src)}
    cs = cases(src)
    fx["cases"] = np.asarray([c[1] for c in cs], np.int32)
    fx["names"] = np.asarray([c[0] for c in cs])
    fx["pillow_version"] = np.asarray(PIL.__version__)
    for i, (name, (k, top, left, h, w, flip, S, f, inv)) in enumerate(cs):
        inv_ch = (0,) if inv else ()
        ref = U.pillow_crop_resize(src[k], (top, left, h, w, flip), S, U.FILTERS[f], inv_ch)
        stats = {}
        mine = U.crop_resize(src[k], (top, left, h, w, flip), S, U.FILTERS[f], inv_ch, stats)
        assert np.array_equal(ref, mine), f"{name}: the restatement differs from Pillow {PIL.__version__}"
        if name == "checkerboard_up":
            assert stats["lo"] < 0 and stats["hi"] > 255 and ref.min() == 0 and ref.max() == 255, stats
        fx[f"out_{i}"] = ref
    return fx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="compare with the committed fixture instead of writing it")
    a = ap.parse_args()
    fx = build()
    if a.check:
        old = np.load(PATH)
        assert sorted(old.files) == sorted(fx), sorted(set(old.files) ^ set(fx))
        bad = [k for k in fx if k != "pillow_version" and not np.array_equal(old[k], fx[k])]
        assert not bad, bad
        print(f"{PATH}: {len(fx['cases'])} cases agree (fixture made with Pillow {old['pillow_version']}, this is {fx['pillow_version']})")
        return
    np.savez_compressed(PATH, **fx)
    print(f"wrote {PATH}: {len(fx['cases'])} cases, {os.path.getsize(PATH)} bytes, Pillow {fx['pillow_version']}")


if __name__ == "__main__":
    main()
