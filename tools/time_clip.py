#!/usr/bin/env python3
"""Time CLIP's vision tower (ViT-B/16, 224 x 224, random weights) on one MI355X.

Prints one JSON line: images/s of ``visual(imgs, return_final_tokens_no_cls=True)`` in both compute precisions, the same result from an
eager-torch run on the same device (the plain-torch restatement tests/clip_util.py::vit_forward in fp32 and under bf16 autocast), and the
c_fc launch (M = batch * 197, N = 3072, K = 768, biased) with FM_EPI_QUICK_GELU next to the same shape with FM_EPI_GELU.  Everything is
reported, nothing asserted.

    python tools/time_clip.py [--batch 64] [--iters 10]
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


def timed(fn, iters, warmup=3):
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
    return ms[len(ms) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    from fourm.hip import _lib as L, ops
    from fourm.utils.clip.model import VisionTransformer
    from tests.clip_util import vit_forward
    B = a.batch
    torch.manual_seed(0)
    vit = VisionTransformer(224, 16, 768, 12, 12, 512).cuda().eval().requires_grad_(False)
    x = torch.randn(B, 3, 224, 224, device="cuda")
    res = {"model": "ViT-B/16", "batch": B, "iters": a.iters}
    for prec in ("bf16", "fp32"):
        vit.compute_precision = prec
        ms = timed(lambda: vit(x, return_final_tokens_no_cls=True), a.iters)
        res[f"hip_{prec}_ms"], res[f"hip_{prec}_images_per_s"] = ms, B / ms * 1e3
    vit.compute_precision = "bf16"
    sd = {k: v.detach() for k, v in vit.state_dict().items()}

    def eager(autocast):
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            return vit_forward(sd, x, "return_final_tokens_no_cls", torch.float32)
    for name, ac in (("fp32", False), ("bf16_autocast", True)):
        ms = timed(lambda: eager(ac), a.iters)
        res[f"eager_{name}_ms"], res[f"eager_{name}_images_per_s"] = ms, B / ms * 1e3
    got, want = vit(x, return_final_tokens_no_cls=True), eager(False)
    res["hip_bf16_vs_eager_fp32_rel_max"] = float((got - want).abs().max() / want.abs().max())
    # the c_fc launch alone
    M, N, K = B * 197, 3072, 768
    h = torch.randn(M, K, device="cuda").bfloat16()
    w = (torch.randn(N, K, device="cuda") * K ** -0.5).bfloat16()
    bias = torch.randn(N, device="cuda") * 0.5
    act = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)
    for name, epi in (("quick_gelu", L.EPI_QUICK_GELU), ("gelu", L.EPI_GELU)):
        ms = timed(lambda: ops.gemm_nt(h, w, act, epilogue=epi, bias=bias), 50, warmup=5)
        res[f"c_fc_{name}_us"], res[f"c_fc_{name}_tflops"] = ms * 1e3, 2.0 * M * N * K / ms / 1e9
    print(json.dumps(res))


if __name__ == "__main__":
    main()
