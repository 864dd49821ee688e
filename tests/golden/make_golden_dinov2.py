#!/usr/bin/env python3
"""Generate tests/golden/dinov2_micro.npz on the CPU from the restatement tests/dinov2_util.py::dino_forward (the written definition of the
DINOv2 tower is the contract; the `facebookresearch/dinov2` package is not available, parity with it is unpinned).

Stored per micro case: the state-dict key list and shapes; per run and result: the restatement's distance (max |a - ref| / max |ref|) from
its own float64 run when it runs in fp32 (``err32``) and under ``torch.autocast('cpu', bfloat16)`` (``err_ac``) - the sizes of error the
GPU tests allow the tower's two precisions (tests/test_dinov2_gpu.py).  ``layers/<i>`` entries: the same for the residual stream after
block i (get_intermediate_layers).

    python tests/golden/make_golden_dinov2.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import dinov2_util as U  # noqa: E402


def main():
    out = {}
    for case, cfg in U.CASES.items():
        sd = U.seeded_state_dict(case)
        shapes = U.expected_shapes(cfg)
        out[f"{case}/keys"] = np.array([k for k, _ in shapes])
        out[f"{case}/shapes"] = np.array([",".join(map(str, s)) for _, s in shapes])
        for run, B, H, W in U.RUNS[case]:
            x = U.images(case, run)
            r64, r32, rac = U.dino_forward(case, sd, x, torch.float64), U.dino_forward(case, sd, x, torch.float32), U.dino_forward(case, sd, x, autocast=True)
            items = [(name, r64[name], r32[name], rac[name]) for name in U.results_of(case)]
            items += [(f"layers/{i}", r64["layers"][i], r32["layers"][i], rac["layers"][i]) for i in range(cfg["depth"])]
            for name, a64, a32, aac in items:
                assert a32.dtype == torch.float32 and a32.shape == a64.shape == aac.shape
                e32, eac = U.rel_max(a32, a64), U.rel_max(aac.float(), a64)
                pre = f"{case}/{run}/{name}"
                out[pre + "/err32"], out[pre + "/err_ac"] = np.array(e32), np.array(eac)
                print(f"[{pre}] shape {tuple(a64.shape)} autocast dtype {aac.dtype}: fp32 vs float64 {e32:.2e}, autocast vs float64 {eac:.2e}")
    path = os.path.join(HERE, "dinov2_micro.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB)")


if __name__ == "__main__":
    torch.set_num_threads(min(16, os.cpu_count()))
    main()
