#!/usr/bin/env python3
"""Throughput of the device-side depth crops (fourm.data.crops.crop_resize_depth) on one GPU.

  crop_resize_depth   64 depth maps of 640 x 480 (uint16) with 10 crops each (upstream's settings: centre crop + 9 random crops of scale
                      0.2 - 1) to 224, bicubic, standardised float32 output: wall time of the whole call (packing on the host, one pinned
                      upload, the two resize launches and the standardisation launch; synchronised), median of --reps calls after a
                      warm-up; the same with standardize=False, and the 8-bit crop_resize on 3-channel images of the same size in the same
                      process for comparison (same-box pair)
  device              the three launches alone, by events around the library calls of one more call
  pillow              the same 640 crops by Pillow (mode I;16 crop + resize + flip) and upstream's formula (torch.sort, slice, mean,
                      var) on 16 host threads, when Pillow is importable; and whether the device's integers equal Pillow's

    python tools/bench_depth_crops.py --out profiles/depth_crops_bench.json"""
import argparse
import json
import os
import random
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ml-4m_amd"), ROOT]


def smooth_depth(rng, H, W):
    """Low-frequency 16-bit depth with a little sensor noise and a saturated far region."""
    small = rng.integers(2000, 60000, (H // 32 + 2, W // 32 + 2)).astype(np.float64)
    ys, xs = np.linspace(0, small.shape[0] - 1.001, H), np.linspace(0, small.shape[1] - 1.001, W)
    y0, x0 = ys.astype(int), xs.astype(int)
    fy, fx = (ys - y0)[:, None], (xs - x0)[None, :]
    a = small[y0][:, x0] * (1 - fy) * (1 - fx) + small[y0 + 1][:, x0] * fy * (1 - fx) + small[y0][:, x0 + 1] * (1 - fy) * fx + small[y0 + 1][:, x0 + 1] * fy * fx
    a = a + rng.normal(0, 20, a.shape)
    a[a > 52000] = 65535
    return np.clip(a, 0, 65535).astype(np.uint16)


def timed(fn, reps):
    import torch
    walls = []
    for it in range(reps + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        if it >= 2:
            walls.append(time.perf_counter() - t0)
    return out, 1e3 * statistics.median(walls)


def device_ms(fn):
    """Milliseconds between events recorded around the library calls of one call of ``fn`` (the launches, not the packing or the upload)."""
    import torch
    from fourm.hip import _lib as L
    names = ("pil_crop_resize16", "depth_standardize", "pil_crop_resize")
    real = {n: getattr(L, n) for n in names}
    spans = {}

    def wrap(n):
        def call(*a):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = real[n](*a)
            e1.record()
            spans[n] = (e0, e1)
            return rc
        return call
    try:
        for n in names:
            setattr(L, n, wrap(n))
        fn()
        torch.cuda.synchronize()
    finally:
        for n in names:
            setattr(L, n, real[n])
    return {n: e0.elapsed_time(e1) for n, (e0, e1) in spans.items()}


def bench(reps):
    import torch
    from fourm.data.crops import crop_resize, crop_resize_depth, make_crop_settings
    rng = np.random.default_rng(0)
    torch.manual_seed(0)
    random.seed(0)
    images = [smooth_depth(rng, 480, 640) for _ in range(64)]
    settings = [make_crop_settings(480, 640, 10, 0.2) for _ in images]
    rgb = [rng.integers(0, 256, (480, 640, 3), dtype=np.uint8) for _ in range(64)]
    half = (0.5, 0.5, 0.5)
    out, ms_std = timed(lambda: crop_resize_depth(images, settings, 224, resample="bicubic"), reps)
    _, ms_plain = timed(lambda: crop_resize_depth(images, settings, 224, resample="bicubic", standardize=False), reps)
    _, ms_rgb = timed(lambda: crop_resize(rgb, settings, 224, resample="bicubic", mean=half, std=half), reps)
    n = out.shape[0]
    res = {"crops": n, "reps": reps, "wall_ms_median": ms_std, "crops_per_s_wall": n / (1e-3 * ms_std), "wall_ms_median_without_standardisation": ms_plain,
           "wall_ms_median_8bit_rgb_crop_resize_same_process": ms_rgb,
           "device_ms": {**device_ms(lambda: crop_resize_depth(images, settings, 224, resample="bicubic")),
                         **device_ms(lambda: crop_resize(rgb, settings, 224, resample="bicubic", mean=half, std=half))}}
    try:
        import PIL
        from PIL import Image
    except ImportError:
        res["pillow"] = "Pillow is not importable here: device figure only"
        return res
    pil = [Image.frombytes("I;16", (640, 480), im.astype("<u2").tobytes()) for im in images]
    torch.set_num_threads(1)          # 16 host threads, each one crop at a time

    def one(job, standardise=True):
        i, (top, left, h, w, flip) = job
        a = np.asarray(pil[i].crop((left, top, left + w, top + h)).resize((224, 224), Image.BICUBIC))
        a = a[:, ::-1].copy() if flip else a
        if not standardise:
            return a
        d = torch.Tensor(a / (2 ** 16 - 1.0)).unsqueeze(0)          # upstream's depth_to_tensor and truncated_depth_standardization
        t = torch.sort(d.reshape(-1), dim=0)[0]
        t = t[int(0.1 * t.shape[0]): int((1 - 0.1) * t.shape[0])]
        return (d - t.mean()) / torch.sqrt(t.var() + 1e-6)
    jobs = [(i, tuple(int(v) for v in s)) for i, st in enumerate(settings) for s in st]
    times = []
    with ThreadPoolExecutor(max_workers=16) as pool:
        for it in range(4):
            t0 = time.perf_counter()
            host = list(pool.map(one, jobs))
            if it >= 1:
                times.append(time.perf_counter() - t0)
        ints = list(pool.map(lambda j: one(j, False), jobs))
    u16 = crop_resize_depth(images, settings, 224, resample="bicubic", out="uint16").cpu().numpy()
    dev = out.cpu()
    res["pillow"] = {"threads": 16, "wall_ms_median": 1e3 * statistics.median(times), "crops_per_s": n / statistics.median(times), "version": PIL.__version__,
                     "device_integers_equal_pillows": bool(all(np.array_equal(a, b) for a, b in zip(u16, ints))),
                     "max_abs_difference_from_the_host_formula": max(float((a - b).abs().max()) for a, b in zip(dev, host))}
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=None)
    p.add_argument("--reps", type=int, default=7)
    a = p.parse_args()
    import torch
    res = {"device": torch.cuda.get_device_name(0), "command": "python tools/bench_depth_crops.py " + " ".join(sys.argv[1:]),
           "crop_resize_depth_64x(480x640)x10_to_224_bicubic_standardised": bench(a.reps)}
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
