#!/usr/bin/env python3
"""Time the CLIP perceptual loss (ViT-B/16, 224 x 224, taps blocks.2-5-8-11, cosine, random weights) on one MI355X: forward + backward to
the pixels of ``preds``.

Prints one JSON line: ms per call of ``ClipPerceptualLoss`` (bf16 mode) and, for comparison, of the same loss in eager torch under bf16
autocast on the same device (the plain-torch restatement tests/clip_percept_util.py::percept_ref with autograd).  Everything is reported,
nothing asserted.

    python tools/time_clip_percept.py [--batch 64] [--iters 10]
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
    from fourm.utils.clip.model import VisionTransformer
    from fourm.vq.percept_losses import ClipPerceptualLoss
    from tests.clip_percept_util import percept_ref
    B, ids = a.batch, "blocks.2-blocks.5-blocks.8-blocks.11"
    torch.manual_seed(0)
    vit = VisionTransformer(224, 16, 768, 12, 12, 512)
    loss_fn = ClipPerceptualLoss(vit, ids, "cosine").cuda()
    targets = torch.randn(B, 3, 224, 224, device="cuda")
    preds = (targets + 0.3 * torch.randn_like(targets)).requires_grad_()
    res = {"model": "ViT-B/16", "batch": B, "iters": a.iters, "taps": ids, "distance": "cosine"}

    def hip():
        preds.grad = None
        loss_fn(preds, targets).mean().backward()

    res["hip_bf16_ms"] = timed(hip, a.iters)
    with torch.no_grad():
        res["hip_bf16_forward_only_ms"] = timed(lambda: loss_fn(preds, targets), a.iters)
    sd = {k: v.detach() for k, v in vit.state_dict().items()}
    taps = [2, 5, 8, 11]

    def eager():
        preds.grad = None
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = percept_ref(sd, preds, targets, taps, "cosine", torch.float32)
        loss.mean().backward()
        return loss

    res["eager_bf16_autocast_ms"] = timed(eager, a.iters)
    hip()
    g_hip, l_hip = preds.grad.clone(), loss_fn(preds.detach(), targets)
    l_eager = eager().detach()
    res["loss_rel_diff"] = float((l_hip - l_eager).abs().max() / l_eager.abs().max())
    res["grad_rel_diff"] = float((g_hip - preds.grad).abs().max() / preds.grad.abs().max())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
