#!/usr/bin/env python3
"""Time DINOv2's vision tower (ViT-B/14, 224 x 224: grid 16 x 16, T = 257; random weights) on one MI355X.

Prints one JSON line and writes it to --out: the median of --iters calls (device events around each call, after a warm-up of every shape) of
``tower(imgs, is_training=True)`` in both compute precisions, bf16 with the batch-invariant GEMM tiling (the default) and with the
shape-dependent routes; the same result from the plain-torch restatement tests/dinov2_util.py::dino_forward in eager torch on the same device,
under bf16 autocast and in fp32; the attention route T = 257 takes and attention's share of the step (events around every profiled launch in
a pass of its own); and the LayerScale fusion (the scaled residual sum inside the next LayerNorm, fm_layernorm_fwd_res_ls) against a run
that settles every sum with fm_layerscale_add alone - the two alternate call by call, and their results are compared bit for bit.
Everything is reported, nothing asserted except that the fused and unfused results are the same bits.

    python tools/time_dinov2.py [--batch 64] [--iters 30] [--out profiles/dinov2_bench.json]
"""
import argparse
import contextlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ml-4m_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


def timed(fns, iters, warmup=3):
    """Median / min / max ms of each callable in ``fns``, the callables alternating call by call (one clock, one neighbourhood)."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    spans = [[] for _ in fns]
    for _ in range(iters):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            spans[k].append((a, b))
    torch.cuda.synchronize()
    out = []
    for sp in spans:
        ms = sorted(a.elapsed_time(b) for a, b in sp)
        out.append((ms[len(ms) // 2], ms[0], ms[-1]))
    return out


class Families:
    """ops.set_profiler target: device events around every profiled launch, summed per family."""

    def __init__(self):
        self.spans = []

    @contextlib.contextmanager
    def launch(self, name, flops, nbytes, tag):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        try:
            yield
        finally:
            b.record()
            self.spans.append((name.split("/")[0], a, b))

    def totals(self):
        torch.cuda.synchronize()
        out = {}
        for fam, a, b in self.spans:
            out[fam] = out.get(fam, 0.0) + a.elapsed_time(b)
        return out


def attention_route(T):
    """The forward route fm_attn_fwd takes for Nq = Nk = T unmasked tokens (csrc/attention.hip: the rule, restated)."""
    if T == 128:
        return "attn_fwd128_kernel (all keys in LDS)"
    if T % 128 == 0 and T <= 512:
        return "attn_fwdt_kernel (online softmax over 128-key tiles)"
    return f"attn_fwd_kernel (general; {(T + 127) // 128} query tiles of 128 rows per head, the last holding {T - (T - 1) // 128 * 128})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_dinov2 measures on an MI355X; no GPU is visible (nothing is measured on the host)")
    from fourm.hip import engine as E
    from fourm.hip import ops
    from fourm.utils.dinov2 import vit_base
    from tests.dinov2_util import dino_forward
    B = a.batch
    torch.manual_seed(0)
    vit = vit_base().cuda().eval().requires_grad_(False)
    with torch.no_grad():
        for blk in vit.blocks:          # (LayerScale away from its init value 1, so that a dropped scale would show in the comparison below)
            blk.ls1.gamma.uniform_(-1.5, 1.5)
            blk.ls2.gamma.uniform_(-1.5, 1.5)
        vit.cls_token.normal_(std=0.5)
    x = torch.randn(B, 3, 224, 224, device="cuda")
    T = 1 + (224 // 14) ** 2
    res = {"model": "DINOv2 ViT-B/14", "batch": B, "image": 224, "tokens_per_image": T, "iters": a.iters, "attention_route": attention_route(T)}

    def hip():
        return vit(x, is_training=True)["x_norm_patchtokens"]

    def put(key, t):
        res[f"{key}_ms"], res[f"{key}_ms_min_max"], res[f"{key}_images_per_s"] = round(t[0], 4), [round(t[1], 4), round(t[2], 4)], round(B / t[0] * 1e3, 1)
    for prec in ("bf16", "fp32"):
        vit.compute_precision = prec
        put(f"hip_{prec}", timed([hip], a.iters)[0])
    vit.compute_precision = "bf16"
    vit.batch_invariant = False
    put("hip_bf16_shape_routed", timed([hip], a.iters)[0])
    vit.batch_invariant = True
    cfg = dict(embed_dim=768, patch_size=14, num_register_tokens=0, num_heads=12, depth=12, ffn_layer="mlp", interpolate_antialias=False,
               interpolate_offset=0.1)
    sd = {k: v.detach() for k, v in vit.state_dict().items()}

    def eager(autocast):
        return dino_forward(cfg, sd, x, torch.float32, autocast=autocast)["x_norm_patchtokens"]
    put("eager_bf16_autocast", timed([lambda: eager(True)], a.iters)[0])
    put("eager_fp32", timed([lambda: eager(False)], a.iters)[0])
    res["eager_autocast_over_hip_bf16"] = round(res["eager_bf16_autocast_ms"] / res["hip_bf16_ms"], 3)
    res["eager_fp32_over_hip_fp32"] = round(res["eager_fp32_ms"] / res["hip_fp32_ms"], 3)
    want = eager(False).float()
    res["hip_bf16_vs_eager_fp32_rel_max"] = float((hip() - want).abs().max() / want.abs().max())
    res["eager_autocast_vs_eager_fp32_rel_max"] = float((eager(True).float() - want).abs().max() / want.abs().max())

    # LayerScale fusion: the sum inside the next LayerNorm against fm_layerscale_add + a plain norm, alternating
    def with_fuse(on):
        def run():
            E.LS_FUSE = on
            try:
                return hip()
            finally:
                E.LS_FUSE = True
        return run
    fused, unfused = with_fuse(True)().clone(), with_fuse(False)().clone()
    if not torch.equal(fused, unfused):
        raise SystemExit("the fused and the unfused LayerScale sums differ")
    tf, tu = timed([with_fuse(True), with_fuse(False)], a.iters)
    put("hip_bf16_ls_fused", tf)
    put("hip_bf16_ls_unfused", tu)
    res["ls_unfused_over_fused"] = round(tu[0] / tf[0], 4)
    # launch families: a pass of its own with events around every profiled launch (their own cost is in the total: read the shares)
    fam = Families()
    ops.set_profiler(fam)
    try:
        hip()
    finally:
        ops.set_profiler(None)
    totals = fam.totals()
    whole = sum(totals.values())
    res["launch_families_ms"] = {k: round(v, 4) for k, v in sorted(totals.items(), key=lambda kv: -kv[1])}
    res["launch_families_share"] = {k: round(v / whole, 3) for k, v in sorted(totals.items(), key=lambda kv: -kv[1])}
    res["attention_share_of_profiled_launches"] = round(totals.get("attn_fwd", 0.0) / whole, 3)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
