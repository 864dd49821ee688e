#!/usr/bin/env python3
"""Timing of LoRA fine-tuning on one MI355X: 4M-B mod7, batch 256, 128 + 128 tokens, rank 4, attention targets, frozen base.

  * per-step time (forward + backward + FusedAdamW) of the LoRA fine-tune against the full train step of the same model without adapters
    (the plain-Linear path is the parent commit's, launch for launch), in alternating rounds;
  * per-launch time of fm_lora_apply on the qkv shape (R = batch x 128 rows, K = 768, N = 2304, r = 12, bf16 x / y) against its byte
    count (x read once, y read and written once) at the HBM rate --hbm-tbs.

Device events around warmed-up loops, median and minimum over the rounds; one JSON document on stdout and in --out.
    python tools/time_lora.py [--batch 256] [--rounds 7] [--out profiles/lora_timing.json]"""
import argparse
import contextlib
import io
import json
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ml-4m_amd"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def timed(fn, iters):
    """Milliseconds per call: device events around ``iters`` back-to-back calls."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rank", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--hbm-tbs", type=float, default=8.0, help="HBM rate the byte count is compared with, TB/s")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: timings are taken on an MI355X only")
    import bench
    from fourm.data.synthetic import synthetic_batch
    from fourm.hip import ops
    from fourm.models import lora_utils as LU
    from fourm.utils.optim_factory import FusedAdamW, get_parameter_groups
    dev = torch.device("cuda", 0)
    n_in = n_out = 128

    def make(lora):
        torch.manual_seed(0)
        model = bench.build_model("fm_base_12e_12d_swiglu_nobias", dev, "mod7").train()
        if lora:
            LU.inject_trainable_LoRA(model, rank=a.rank, scale=1.0, target_replace_modules=LU.get_LoRA_module_names("attn"))
            for n, p in model.named_parameters():
                p.requires_grad = "lora_" in n
            model = model.to(dev)
            with torch.no_grad():
                for n, p in model.named_parameters():
                    if "lora_up" in n:
                        p.normal_(std=0.02)
            opt = FusedAdamW([{"params": [p for p in model.parameters() if p.requires_grad], "weight_decay": 0.05}], lr=1e-4, betas=(0.9, 0.95), eps=1e-8)
        else:
            with contextlib.redirect_stdout(io.StringIO()):
                groups = get_parameter_groups(model, weight_decay=0.05, skip_list=model.no_weight_decay())
            opt = FusedAdamW(groups, lr=1e-4, betas=(0.9, 0.95), eps=1e-8)
        batches = [synthetic_batch(model, a.batch, n_in, n_out, device=dev, seed=i) for i in range(2)]
        count = [0]

        def step():
            loss, _ = model(batches[count[0] % 2], n_in, n_out, loss_type="mod")
            loss.backward()
            opt.fused_grad_norm(lazy=True)
            opt.step()
            opt.zero_grad(set_to_none=True)
            count[0] += 1
        return model, step

    random.seed(0)
    full_model, full_step = make(False)
    lora_model, lora_step = make(True)
    R, K, N, r = a.batch * n_in, 768, 2304, 3 * a.rank
    x = torch.randn(R, K, device=dev).bfloat16()
    y = torch.randn(R, N, device=dev).bfloat16()
    down, up = torch.randn(r, K, device=dev) / r, torch.randn(N, r, device=dev) * 0.02
    p = torch.empty(R, r, device=dev)
    work = {"full_step_ms": (full_step, a.iters), "lora_step_ms": (lora_step, a.iters),
            "lora_apply_qkv_ms": (lambda: ops.lora_apply(x, down, up, y, 1.0, p, R, K, N), 20)}
    for fn, _ in work.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in work}
    for _ in range(a.rounds):                        # alternating rounds
        for k, (fn, iters) in work.items():
            samples[k].append(timed(fn, iters))
    res = {"device": torch.cuda.get_device_name(0), "model": "4M-B mod7", "batch": a.batch, "tokens": [n_in, n_out], "rank": a.rank, "targets": "attn",
           "rounds": a.rounds, "trainable_parameters": sum(q.numel() for q in lora_model.parameters() if q.requires_grad),
           "parameters": sum(q.numel() for q in full_model.parameters())}
    for k, v in samples.items():
        res[k] = {"median": statistics.median(v), "min": min(v)}
    res["lora_step_over_full_step"] = res["lora_step_ms"]["median"] / res["full_step_ms"]["median"]
    nbytes = R * K * 2 + 2 * R * N * 2 + R * r * 4
    res["lora_apply_qkv"] = {"R": R, "K": K, "N": N, "r": r, "bytes": nbytes, "ms_at_hbm_rate": nbytes / (a.hbm_tbs * 1e12) * 1e3,
                             "achieved_tbs": nbytes / (res["lora_apply_qkv_ms"]["median"] * 1e-3) / 1e12}
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
