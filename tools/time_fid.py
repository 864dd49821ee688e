#!/usr/bin/env python3
"""Throughput of the FID tower (fourm.utils.inception.FidInceptionV3) on one GPU, beside the same network in eager torch fp32.

  hip     FidInceptionV3.forward on a batch of 64 uint8 images of 256 x 256 (preprocess, 94 convolutions, pools, head): wall time of the
          call ended by a device synchronise, median of --reps calls after a warm-up.
  torch   the test restatement (tests/inception_util.py: F.conv2d + batch norm + ReLU, the TF1 resize) cast to fp32, on the same device
          with the same seeded weights and images, timed the same way.  The two are alternated call by call in one process.
  flop    2 K Cout Ho Wo over the 94 units and the head, from the shapes: the whole-network rate over the fp32 matrix peak is an end-to-end
          figure, not a kernel's share of peak.

    python tools/time_fid.py --out profiles/fid_bench.json"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ml-4m_amd"), ROOT]
PEAK_F32_MATRIX_TFLOPS = 157.3


def flop_per_image():
    """2 K Cout Ho Wo of every convolution the restatement runs on one 299 x 299 image, plus the head."""
    import torch
    import torch.nn.functional as F
    from tests import inception_util as IU
    real, total = F.conv2d, [0]

    def counted(x, w, *args, **kw):
        y = real(x, w, *args, **kw)
        total[0] += 2 * w[0].numel() * y.shape[1] * y.shape[2] * y.shape[3]
        return y
    F.conv2d = counted
    try:
        with torch.no_grad():
            IU.tower(IU.seeded_state_dict(), torch.zeros(1, 3, 299, 299))
    finally:
        F.conv2d = real
    return total[0] + 2 * 2048 * 1008


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
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "fid_bench.json"))
    p.add_argument("--batch", type=int, default=64)
    p.add_argument("--size", type=int, default=256)
    p.add_argument("--reps", type=int, default=30)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--no-torch", action="store_true", help="time the HIP tower alone")
    a = p.parse_args()
    import torch
    from fourm.utils.inception import FidInceptionV3
    from tests import inception_util as IU
    assert torch.cuda.is_available(), "time_fid.py measures on an MI355X; there is nothing to time without one"
    dev = "cuda:0"
    sd = IU.seeded_state_dict()
    imgs = torch.randint(0, 256, (a.batch, 3, a.size, a.size), generator=IU.gen(0), dtype=torch.uint8).to(dev)
    model = FidInceptionV3(chunk=a.batch)
    model.load_state_dict(sd)
    model = model.to(dev).eval().requires_grad_(False)
    sd_dev = {k: v.to(dev) for k, v in sd.items()}
    flop = flop_per_image()

    def hip():
        return model(imgs)["pool"]

    def eager():
        with torch.no_grad():
            return IU.tower(sd_dev, IU.preprocess(imgs, False, torch.float32))["pool"]

    fns = {"hip": hip} if a.no_torch else {"hip": hip, "torch_fp32": eager}
    walls = timed_pair(fns, a.reps, a.warmup)
    res = {"device": torch.cuda.get_device_name(0), "command": f"python tools/time_fid.py --batch {a.batch} --size {a.size} --reps {a.reps} --warmup {a.warmup}" + (" --no-torch" if a.no_torch else ""),
           "batch": a.batch,
           "input": f"uint8 {a.size} x {a.size}", "reps": a.reps, "warmup": a.warmup, "gflop_per_image": flop / 1e9}
    for k, w in walls.items():
        med = statistics.median(w)
        res[k] = {"wall_ms_median": 1e3 * med, "wall_ms_min_max": [1e3 * min(w), 1e3 * max(w)], "images_per_s": a.batch / med,
                  "whole_network_tflops": flop * a.batch / med / 1e12,
                  "whole_network_share_of_fp32_matrix_peak": flop * a.batch / med / 1e12 / PEAK_F32_MATRIX_TFLOPS}
    if not a.no_torch:
        x, y = hip().double(), eager().double()
        res["max_abs_difference_over_max"] = float((x - y).abs().max() / y.abs().max())
        res["torch_fp32_over_hip_time"] = res["torch_fp32"]["wall_ms_median"] / res["hip"]["wall_ms_median"]
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
