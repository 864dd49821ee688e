#!/usr/bin/env python3
"""Generate tests/golden/clip_vit_micro.npz from the UNMODIFIED upstream ``fourm/utils/clip/model.py::VisionTransformer`` on the CPU.

The file is loaded by path (it imports only torch and numpy).  Two micro towers (tests/clip_util.py CASES: patch 8 / width 128 / 2 heads /
2 layers and patch 16 / width 192 / 3 heads / 1 layer) with weights and images from seeds; each runs at its native resolution and at one
that needs an interpolated position table (square and non-square).  Stored per case: the state-dict key list and shapes; per run and
return flag: upstream's fp32 output, upstream's output under ``torch.autocast('cpu', bfloat16)``, and the distances of both
(max |a - ref| / max |ref|) from the float64 restatement tests/clip_util.py::vit_forward.  Runs only where the upstream checkout exists.

    python tests/golden/make_golden_clip.py
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import ref_stubs  # noqa: E402

from tests import clip_util as U  # noqa: E402


def load_upstream():
    path = os.path.join(ref_stubs.REFERENCE_ROOT, "fourm", "utils", "clip", "model.py")
    spec = importlib.util.spec_from_file_location("upstream_clip_model", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ref = load_upstream()
    out = {}
    for case, cfg in U.CASES.items():
        model = ref.VisionTransformer(**cfg)
        sd = U.seeded_state_dict(case)
        model.load_state_dict(sd, strict=True)
        model.eval()
        keys = list(model.state_dict().keys())
        out[f"{case}/keys"] = np.array(keys)
        out[f"{case}/shapes"] = np.array([",".join(map(str, model.state_dict()[k].shape)) for k in keys])
        for run, B, H, W in U.RUNS[case]:
            x = U.images(case, run)
            for flag in U.FLAGS:
                kw = U.flag_kwargs(flag)
                with torch.no_grad():
                    o32 = model(x, **kw)
                    with torch.autocast("cpu", dtype=torch.bfloat16):
                        oac = model(x, **kw)
                    o64 = U.vit_forward(sd, x, flag, torch.float64)
                assert o32.dtype == torch.float32 and o32.shape == o64.shape, (o32.dtype, o32.shape, o64.shape)
                e32, eac = U.rel_max(o32, o64), U.rel_max(oac.float(), o64)
                pre = f"{case}/{run}/{flag}"
                out[pre + "/out32"] = o32.numpy()
                out[pre + "/out_ac"] = oac.float().numpy()
                out[pre + "/err32"] = np.array(e32)
                out[pre + "/err_ac"] = np.array(eac)
                print(f"[{pre}] shape {tuple(o32.shape)} autocast dtype {oac.dtype}: fp32 vs float64 {e32:.2e}, autocast vs float64 {eac:.2e}")
    path = os.path.join(HERE, "clip_vit_micro.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB)")


if __name__ == "__main__":
    torch.set_num_threads(min(16, os.cpu_count()))
    main()
