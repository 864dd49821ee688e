#!/usr/bin/env python3
"""Time one training step of the LPIPS perceptual loss (frozen VGG16, random weights) on one MI355X: the forward of the target, the forward
of the reconstruction and the backward down to the pixels, at B = 16, 224 x 224 by default.

Measured: bf16 mode (median of --iters steps between device events, after a warm-up of every shape); fp32 mode, once; for context on the same
box the plain-torch restatement tests/lpips_util.py::lpips_ref on the GPU under torch.autocast("cuda", bfloat16) with autograd.  Reported:
ms per step, the achieved rate over the algorithmic work of a step (3 x 15.35 GMAC per image pair: two forwards and the dgrad pass; the
first convolution has no dgrad to the pixels' channels worth counting), and - from a separate profiled step, events around every launch -
the per-kernel breakdown with GB/s of the streaming kernels.  Everything is reported, nothing asserted; without a GPU it fails.

    python tools/bench_lpips.py [--batch 16] [--size 224] [--iters 10] [--out profiles/lpips_step.json]
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

CONVS = [(3, 64, 1), (64, 64, 1), (64, 128, 2), (128, 128, 2), (128, 256, 4), (256, 256, 4), (256, 256, 4), (256, 512, 8), (512, 512, 8), (512, 512, 8),
         (512, 512, 16), (512, 512, 16), (512, 512, 16)]          # (C_in, C_out, down-sampling of the layer's grid)


def forward_macs(H, W):
    return sum(9 * ci * co * (H // s) * (W // s) for ci, co, s in CONVS)


def timed(fn, iters, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(iters + 1)]
    ev[0].record()
    for i in range(iters):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    ms = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(iters))
    return ms[len(ms) // 2], ms[0], ms[-1]


class Prof:
    """Events around every launch of one step (ops.set_profiler)."""

    def __init__(self):
        self.recs = []

    class _Ctx:
        def __init__(self, prof, rec):
            self.p, self.rec = prof, rec

        def __enter__(self):
            self.a, self.b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            self.a.record(torch.cuda.current_stream())
            return self

        def __exit__(self, *exc):
            self.b.record(torch.cuda.current_stream())
            self.p.recs.append(self.rec + (self.a, self.b))
            return False

    def launch(self, name, flops, nbytes, tag=""):
        return self._Ctx(self, (name, flops, nbytes, tag))

    def table(self):
        torch.cuda.synchronize()
        agg = {}
        for name, fl, nb, tag, a, b in self.recs:
            d = agg.setdefault(f"{name} {tag}".strip(), dict(ms=0.0, flops=0.0, bytes=0.0, launches=0))
            d["ms"] += a.elapsed_time(b); d["flops"] += fl; d["bytes"] += nb; d["launches"] += 1
        rows = []
        for k, d in sorted(agg.items(), key=lambda kv: -kv[1]["ms"]):
            row = dict(kernel=k, launches=d["launches"], ms=round(d["ms"], 4))
            if d["flops"]:
                row["tflops"] = round(d["flops"] / d["ms"] / 1e9, 1)
            if d["bytes"]:
                row["gb_per_s"] = round(d["bytes"] / d["ms"] / 1e6, 1)
            rows.append(row)
        return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_lpips needs an MI355X: a timing taken elsewhere says nothing")
    from fourm.hip import ops
    from fourm.vq.percept_losses import LpipsPerceptualLoss
    from tests.lpips_util import lpips_ref
    B, S = a.batch, a.size
    torch.manual_seed(0)
    targets = (torch.rand(B, 3, S, S, device="cuda") * 2 - 1)
    preds = (targets + 0.3 * torch.randn_like(targets)).requires_grad_()
    flops_step = 3 * 2.0 * forward_macs(S, S) * B
    res = {"batch": B, "size": S, "iters": a.iters, "gflop_per_pair": round(flops_step / B / 1e9, 1)}

    def step_of(mod):
        def step():
            preds.grad = None
            mod(preds, targets).mean().backward()
        return step

    bf = LpipsPerceptualLoss(compute_precision="bf16").cuda()
    med, lo, hi = timed(step_of(bf), a.iters)
    res["hip_bf16_ms"], res["hip_bf16_ms_min_max"] = round(med, 3), [round(lo, 3), round(hi, 3)]
    res["hip_bf16_tflops"] = round(flops_step / med / 1e9, 1)
    with torch.no_grad():
        res["hip_bf16_forward_only_ms"] = round(timed(lambda: bf(preds, targets), a.iters)[0], 3)
    prof = Prof()
    ops.set_profiler(prof)
    try:
        step_of(bf)()
    finally:
        ops.set_profiler(None)
    res["hip_bf16_kernels"] = prof.table()
    res["hip_bf16_kernel_ms_sum"] = round(sum(r["ms"] for r in res["hip_bf16_kernels"]), 3)
    g_hip, l_hip = preds.grad.clone(), bf(preds.detach(), targets)

    sd = {k: v.detach() for k, v in bf.state_dict().items()}

    def eager():
        preds.grad = None
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = lpips_ref(sd, preds, targets, torch.float32)
        loss.mean().backward()
        return loss

    res["eager_bf16_autocast_ms"] = round(timed(eager, a.iters)[0], 3)
    l_eager = eager().detach()
    res["loss_rel_diff_vs_eager"] = float((l_hip - l_eager).abs().max() / l_eager.abs().max())
    res["grad_rel_l2_diff_vs_eager"] = float((g_hip - preds.grad).norm() / preds.grad.norm())
    del bf
    torch.cuda.empty_cache()

    f32 = LpipsPerceptualLoss(compute_precision="fp32").cuda()
    step = step_of(f32)
    step()                                                   # (warm-up: buffers, code objects)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    step()
    e1.record()
    torch.cuda.synchronize()
    res["hip_fp32_ms_once"] = round(e0.elapsed_time(e1), 3)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
