#!/usr/bin/env python3
"""Throughput of the LPIPS (AlexNet) validation metric on one GPU, beside the same network in eager torch fp32.

  hip     LearnedPerceptualImagePatchSimilarity.update on a batch of 64 pairs of 224 x 224 fp32 images (two towers of five convolutions and
          two pools, five distance launches, the float64 accumulation): wall time of the call ended by a device synchronise, median of
          --reps calls after a warm-up.
  torch   the test restatement (tests/lpips_metric_util.py: F.conv2d + ReLU + F.max_pool2d, the normalisation and the weighted squared
          difference in torch ops) in fp32 on the same device with the same seeded weights and images, timed the same way.  The two are
          alternated call by call in one process.
  stem    fm_conv2d_stem_f32 alone on the same 64 images (events around 20 launches in a row), with 2 K Cout Ho Wo over the time.
  flop    2 K Cout Ho Wo over the ten convolutions of a pair: the whole-metric rate over the fp32 matrix peak is an end-to-end figure, not
          a kernel's share of peak.

    python tools/time_lpips_metric.py --out profiles/lpips_metric_bench.json"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ml-4m_amd"), ROOT]
PEAK_F32_MATRIX_TFLOPS = 157.3


def flop_per_pair(size):
    """2 K Cout Ho Wo of the five convolutions on one size x size image, twice (both towers)."""
    from tests import lpips_metric_util as MU
    total, h = 0, size
    for li, (_, _, cin, cout, k, st, p) in enumerate(MU.CONVS):
        h = (h + 2 * p - k) // st + 1
        total += 2 * k * k * cin * cout * h * h
        if li < 2:
            h = (h - 3) // 2 + 1
    return 2 * total


def timed_pair(fns, reps, warmup):
    import torch
    walls = {k: [] for k in fns}
    for it in range(warmup + reps):
        for k, fn in fns.items():                                      # alternated: both see the same neighbours on the host
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if it >= warmup:
                walls[k].append(time.perf_counter() - t0)
    return walls


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "lpips_metric_bench.json"))
    p.add_argument("--batch", type=int, default=64)
    p.add_argument("--size", type=int, default=224)
    p.add_argument("--reps", type=int, default=30)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--no-torch", action="store_true", help="time the HIP metric alone")
    a = p.parse_args()
    import torch
    from fourm.vq.metrics import LearnedPerceptualImagePatchSimilarity
    from fourm.vq.percept_losses.lpips_alex import LpipsAlex, conv2d_stem
    from tests import lpips_metric_util as MU
    assert torch.cuda.is_available(), "time_lpips_metric.py measures on an MI355X; there is nothing to time without one"
    dev = "cuda:0"
    sd = MU.seeded_state_dict()
    img0 = torch.rand(a.batch, 3, a.size, a.size, generator=MU.gen(0)).to(dev)
    img1 = (img0 + 0.2 * (torch.rand(img0.shape, generator=MU.gen(1)).to(dev) - 0.5)).clamp(0, 1)
    net = LpipsAlex(sd, chunk=a.batch).to(dev)
    metric = LearnedPerceptualImagePatchSimilarity(net_type='alex', reduction='mean', normalize=True, net=net)
    sd_dev = {k: v.to(dev) for k, v in sd.items()}
    flop = flop_per_pair(a.size)

    def hip():
        metric.update(img0, img1)

    def eager():
        with torch.no_grad():
            return MU.lpips(sd_dev, img0, img1, True, torch.float32).double().sum()

    fns = {"hip": hip} if a.no_torch else {"hip": hip, "torch_fp32": eager}
    walls = timed_pair(fns, a.reps, a.warmup)
    res = {"device": torch.cuda.get_device_name(0),
           "command": f"python tools/time_lpips_metric.py --batch {a.batch} --size {a.size} --reps {a.reps} --warmup {a.warmup}" + (" --no-torch" if a.no_torch else ""),
           "batch": a.batch, "input": f"fp32 pairs {a.size} x {a.size} in [0, 1], normalize=True", "reps": a.reps, "warmup": a.warmup, "gflop_per_pair": flop / 1e9}
    for k, w in walls.items():
        med = statistics.median(w)
        res[k] = {"wall_ms_median": 1e3 * med, "wall_ms_min_max": [1e3 * min(w), 1e3 * max(w)], "pairs_per_s": a.batch / med,
                  "whole_metric_tflops": flop * a.batch / med / 1e12,
                  "whole_metric_share_of_fp32_matrix_peak": flop * a.batch / med / 1e12 / PEAK_F32_MATRIX_TFLOPS}
    if not a.no_torch:
        x, y = net.scores(img0, img1, True).double(), MU.lpips(sd_dev, img0, img1, True, torch.float32).double()
        res["max_abs_difference_over_max"] = float((x - y).abs().max() / y.abs().max())
        res["torch_fp32_over_hip_time"] = res["torch_fp32"]["wall_ms_median"] / res["hip"]["wall_ms_median"]
    # the stem alone
    c = net._prepare(torch.device(dev))
    mul, add = c["affine"][True]
    _, _, cin, cout, k, st, pad = MU.CONVS[0]
    ho = (a.size + 2 * pad - k) // st + 1
    out = torch.empty(a.batch * ho * ho, cout, device=dev)
    n = 20
    for _ in range(3):
        conv2d_stem(img0, c["w"][0], c["bias"][0], k, k, st, pad, mul, add, (0.0, 1.0), True, out)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        conv2d_stem(img0, c["w"][0], c["bias"][0], k, k, st, pad, mul, add, (0.0, 1.0), True, out)
    e1.record()
    torch.cuda.synchronize()
    stem_ms = e0.elapsed_time(e1) / n
    stem_flop = 2.0 * k * k * cin * cout * ho * ho * a.batch
    res["stem"] = {"ms_per_launch": stem_ms, "launches_timed": n, "gflop": stem_flop / 1e9, "tflops": stem_flop / stem_ms / 1e9,
                   "share_of_fp32_matrix_peak": stem_flop / stem_ms / 1e9 / PEAK_F32_MATRIX_TFLOPS,
                   "input_gb_per_s": img0.numel() * 4 / stem_ms / 1e6}
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
