#!/usr/bin/env python3
"""Timing of the MLP + Memcodes tokenizers at upstream's three geometries on one MI355X (BottleneckMLP/B_6-Wi_1024 both ways, latent 1024 in
8 heads; DINOv2-B14 global: 768 channels, 8192 codes; ImageBind-H14 global: 1280 channels, 8192 codes; human poses: 207 channels, 1024
codes), one vector per sample, batch 64 and 256: samples / s of ``tokenize`` and of ``decode_tokens``, and the share of the tokenize time
spent in the code search (fm_memcodes_assign: search, merge and value gather).

Device events around warmed-up loops, alternating rounds, median and minimum reported; one JSON document on stdout and in --out.
    python tools/time_memcodes.py [--batches 64 256] [--rounds 7] [--out profiles/memcodes_timing.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ml-4m_amd"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

GEOMETRIES = {"DINOv2-B14-global": (768, 8192), "ImageBind-H14-global": (1280, 8192), "human_poses": (207, 1024)}
MLP = "BottleneckMLP/B_6-Wi_1024"


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
    ap.add_argument("--batches", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: timings are taken on an MI355X only")
    from fourm.vq import VQVAE
    from fourm.vq import engine as E
    res = {"device": torch.cuda.get_device_name(0), "mlp": MLP, "latent_dim": 1024, "heads": 8, "rounds": a.rounds, "cases": []}
    for name, (channels, codes) in GEOMETRIES.items():
        torch.manual_seed(0)
        m = VQVAE(enc_type=MLP, dec_type=MLP, n_channels=channels, latent_dim=1024, num_codebooks=8, codebook_size=codes, quant_type="memcodes",
                  patch_proj=False, sync_codebook=False).cuda().eval()
        for B in a.batches:
            x = torch.randn(B, channels, 1, 1, device="cuda")
            tok = m.tokenize(x)
            z = torch.randn(B, 1024, device="cuda")
            work = {
                "tokenize_ms": (lambda: m.tokenize(x), 20),
                "decode_tokens_ms": (lambda: m.decode_tokens(tok), 20),
                "search_ms": (lambda: E._memcodes_assign(m.quantize, z, B, 1, 1), 50),
            }
            for fn, _ in work.values():                      # warm up every shape of the timed window
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            samples = {k: [] for k in work}
            for _ in range(a.rounds):                        # alternating rounds
                for k, (fn, iters) in work.items():
                    samples[k].append(timed(fn, iters))
            row = {"tokenizer": name, "channels": channels, "codes": codes, "batch": B}
            for k, v in samples.items():
                row[k] = {"median": statistics.median(v), "min": min(v)}
            row["tokenize_samples_per_s"] = B / (row["tokenize_ms"]["median"] * 1e-3)
            row["decode_tokens_samples_per_s"] = B / (row["decode_tokens_ms"]["median"] * 1e-3)
            row["search_share_of_tokenize"] = row["search_ms"]["median"] / row["tokenize_ms"]["median"]
            res["cases"].append(row)
        del m
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
