#!/usr/bin/env python3
"""Time of CLIP ViT-B/16's text tower (width 512, 8 heads, 12 layers, 77 tokens, vocabulary 49408, random weights) on one MI355X at batch 256:
``fourm.utils.clip.TextTransformer`` in bf16 mode against the plain-torch restatement of ``CLIP.encode_text`` (explicit softmax attention with the
triu mask, F.layer_norm, matmuls) on the same device, under bf16 autocast and in fp32.

One process, one run: a warm-up, then --iters forwards of each between device events; the median per forward is reported with the minimum and
maximum, the two ratios, and - from a separate pass with per-launch events - the share of every launch family of the HIP path and the name of
the one that dominates.  Nothing is asserted and no speed is required; without a GPU it fails.

    python tools/time_clip_text.py [--batch 256] [--iters 10] [--out profiles/clip_text_bench.json]
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
import torch.nn.functional as F  # noqa: E402


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
    return ms[len(ms) // 2], ms[0], ms[-1]


class Families:
    """ops.set_profiler target: device events around every profiled launch, summed per family (the launch name up to the first '/')."""

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


def torch_text_forward(p, ids, heads):
    """CLIP.encode_text, default result, as plain tensor algebra (autocast decides the matmul precision)."""
    D = p["ln_final.weight"].shape[0]
    B, Lc = ids.shape
    t = p["token_embedding.weight"][ids] + p["positional_embedding"]
    blocked = torch.ones(Lc, Lc, dtype=torch.bool, device=ids.device).triu(1)
    i = 0
    while f"transformer.resblocks.{i}.ln_1.weight" in p:
        b = f"transformer.resblocks.{i}."
        h = F.layer_norm(t, (D,), p[b + "ln_1.weight"], p[b + "ln_1.bias"], 1e-5)
        q, k, v = F.linear(h, p[b + "attn.in_proj_weight"], p[b + "attn.in_proj_bias"]).reshape(B, Lc, 3, heads, 64).permute(2, 0, 3, 1, 4)
        s = (q @ k.transpose(-1, -2) * 64 ** -0.5).masked_fill(blocked, float("-inf"))
        a = torch.softmax(s, -1) @ v
        t = t + F.linear(a.permute(0, 2, 1, 3).reshape(B, Lc, D), p[b + "attn.out_proj.weight"], p[b + "attn.out_proj.bias"])
        u = F.linear(F.layer_norm(t, (D,), p[b + "ln_2.weight"], p[b + "ln_2.bias"], 1e-5), p[b + "mlp.c_fc.weight"], p[b + "mlp.c_fc.bias"])
        u = u * torch.sigmoid(1.702 * u)
        t = t + F.linear(u, p[b + "mlp.c_proj.weight"], p[b + "mlp.c_proj.bias"])
        i += 1
    t = F.layer_norm(t, (D,), p["ln_final.weight"], p["ln_final.bias"], 1e-5)
    return t[torch.arange(B, device=ids.device), ids.argmax(dim=-1)] @ p["text_projection"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_clip_text needs an MI355X: a timing taken elsewhere says nothing")
    from fourm.hip import ops
    from fourm.utils.clip import TextTransformer
    cfg = dict(embed_dim=512, context_length=77, vocab_size=49408, width=512, heads=8, layers=12)
    torch.manual_seed(0)
    tower = TextTransformer(**cfg).to("cuda").eval().requires_grad_(False)
    B, Lc, V = a.batch, cfg["context_length"], cfg["vocab_size"]
    ids = torch.randint(1, V - 2, (B, Lc))
    ids[:, 0] = V - 2                                                            # start-of-text, then words, end-of-text at a drawn position
    ids[torch.arange(B), torch.randint(2, Lc, (B,))] = V - 1
    ids = ids.to("cuda")
    params = {k: v.detach() for k, v in tower.state_dict().items()}
    res = dict(config=cfg, batch=B, iters=a.iters, mode="bf16")

    def hip():
        return tower(ids, check_ids=False)

    def torch_autocast():
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            return torch_text_forward(params, ids, cfg["heads"])

    def torch_fp32():
        with torch.no_grad():
            return torch_text_forward(params, ids, cfg["heads"])

    for name, fn in (("hip_bf16", hip), ("torch_autocast_bf16", torch_autocast), ("torch_fp32", torch_fp32)):
        med, lo, hi = timed(fn, a.iters)
        res[name + "_ms"], res[name + "_ms_min_max"] = round(med, 4), [round(lo, 4), round(hi, 4)]
        res[name + "_texts_per_s"] = round(B / med * 1e3, 1)
    res["torch_autocast_over_hip"] = round(res["torch_autocast_bf16_ms"] / res["hip_bf16_ms"], 3)
    res["torch_fp32_over_hip"] = round(res["torch_fp32_ms"] / res["hip_bf16_ms"], 3)
    # orientation: the two bf16 paths against torch's fp32 result (max |a - ref| / max |ref|)
    ref = torch_fp32().double()
    res["hip_bf16_vs_torch_fp32"] = float((hip().double() - ref).abs().max() / ref.abs().max())
    res["torch_autocast_vs_torch_fp32"] = float((torch_autocast().double() - ref).abs().max() / ref.abs().max())
    # launch families of the HIP path: a separate pass with events around every profiled launch (the events serialise nothing, but their own
    # cost is in the total: the shares are what is read off, not the sum)
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
    res["dominant_launch_family"] = max(totals, key=totals.get)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
