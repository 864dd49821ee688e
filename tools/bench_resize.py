#!/usr/bin/env python3
"""Throughput of the resize kernels (csrc/resize.hip) on one MI355X at the sizes of upstream's tokenizer recipes:

    (64, 3, 512, 512) -> 224, bilinear with antialias and the CLIP loss's per-channel affine (the perceptual term's transform), and
    (64, 3, 512, 512) -> 384, plain bilinear (prepare_inputs at a drawn training resolution),

forward and adjoint.  Reported per case: the median ms of --iters launches between device events after a warm-up, and GB/s over the
algorithmic bytes (the input read once plus the output written once, 4 bytes per element).  Three input buffers are used in turn (0.6 GB, more
than the 256 MiB Infinity Cache).  torch's own F.interpolate and its autograd backward on the same box stand next to it, for orientation only
(its backward scatters with atomics and computes the weights in fp32).  Everything is reported, nothing asserted; without a GPU it fails.

    python tools/bench_resize.py [--batch 64] [--iters 20] [--out profiles/resize_bench.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ml-4m_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def timed(fn, iters, warmup=3):
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(iters + 1)]
    ev[0].record()
    for i in range(iters):
        fn(i)
        ev[i + 1].record()
    torch.cuda.synchronize()
    ms = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(iters))
    return ms[len(ms) // 2], ms[0], ms[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_resize needs an MI355X: a timing taken elsewhere says nothing")
    from fourm.hip import _lib as L, ops
    from fourm.vq.resize import axis_table
    B, S = a.batch, a.size
    torch.manual_seed(0)
    xs = [torch.randn(B, 3, S, S, device="cuda") for _ in range(3)]
    scale, shift = torch.tensor([1.9, 1.8, 1.7], device="cuda"), torch.tensor([-0.2, 0.1, 0.3], device="cuda")
    res = {"batch": B, "in_size": S, "iters": a.iters, "cases": []}
    for out, aa, affine in ((224, True, True), (384, False, False)):
        mode = L.RESIZE_BILINEAR_AA if aa else L.RESIZE_BILINEAR
        th, tw = axis_table(S, out, mode, "cuda"), axis_table(S, out, mode, "cuda")
        y = torch.empty(B, 3, out, out, device="cuda")
        dys = [torch.randn(B, 3, out, out, device="cuda") for _ in range(3)]
        dx = torch.empty(B, 3, S, S, device="cuda")
        sc, sh = (scale, shift) if affine else (None, None)
        nbytes = 4.0 * (xs[0].numel() + y.numel())
        row = dict(out_size=out, antialias=aa, affine=affine, taps=th["taps"], transposed_taps=th["t_taps"], algorithmic_mb=round(nbytes / 1e6, 1))
        for name, fn in (("hip_fwd", lambda i: ops.resize_bilinear_fwd(xs[i % 3], y, th, tw, sc, sh)),
                         ("hip_bwd", lambda i: ops.resize_bilinear_bwd(dys[i % 3], dx, th, tw, sc)),
                         ("torch_fwd", lambda i: F.interpolate(xs[i % 3], (out, out), mode="bilinear", align_corners=False, antialias=aa))):
            med, lo, hi = timed(fn, a.iters)
            row[name + "_ms"], row[name + "_ms_min_max"], row[name + "_gb_per_s"] = round(med, 4), [round(lo, 4), round(hi, 4)], round(nbytes / med / 1e6, 1)
        # torch's backward alone: the graph is built outside the timed window
        leaves = [x.clone().requires_grad_() for x in xs]
        outs = [F.interpolate(v, (out, out), mode="bilinear", align_corners=False, antialias=aa) for v in leaves]
        med, lo, hi = timed(lambda i: torch.autograd.grad(outs[i % 3], leaves[i % 3], dys[i % 3], retain_graph=True), a.iters)
        row["torch_bwd_ms"], row["torch_bwd_ms_min_max"], row["torch_bwd_gb_per_s"] = round(med, 4), [round(lo, 4), round(hi, 4)], round(nbytes / med / 1e6, 1)
        # the two forwards on the same input (orientation: torch's weights are fp32)
        ops.resize_bilinear_fwd(xs[0], y, th, tw, None, None)
        row["max_abs_diff_vs_torch_fwd"] = float((y - outs[0].detach()).abs().max())
        del leaves, outs
        res["cases"].append(row)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
