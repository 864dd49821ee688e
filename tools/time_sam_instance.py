#!/usr/bin/env python3
"""Timing of the SAM-instance tokenizer at upstream's geometry on one MI355X (vit_b_enc / vit_b_dec, 64 x 64 one-channel masks, patch 16,
latent_dim 1024, 1024 codes, out_conv, batch 384 instances): instances / s of ``tokenize`` and of ``decode_tokens``, the time of the search
launch (fm_vq_assign_wide, R = 6144 rows) and of one ConvNeXt launch (fm_convnext_block), and as the yardstick for the search the rate
fm_gemm_f32 (the same exact-fp32 MFMA, full (R, K) output) reaches on the same (6144, 1024, 1024) product.

Device events around warmed-up loops, alternating rounds, median and minimum reported; one JSON document on stdout and in --out.
    python tools/time_sam_instance.py [--batch 384] [--rounds 7] [--out profiles/sam_instance_timing.json]"""
import argparse
import json
import os
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
    ap.add_argument("--batch", type=int, default=384)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: timings are taken on an MI355X only")
    from fourm.hip import _lib as L, ops
    from fourm.vq import VQVAE
    from fourm.vq import engine as E
    from tests.sam_instance_util import synthetic_masks
    torch.manual_seed(0)
    m = VQVAE(enc_type="vit_b_enc", dec_type="vit_b_dec", image_size=64, n_channels=1, patch_size=16, latent_dim=1024, codebook_size=1024, norm_codes=True,
              out_conv=True, post_mlp=True, sync_codebook=False).cuda().eval()
    B = a.batch
    x = synthetic_masks(B, 64, seed=1).cuda()
    tok = m.tokenize(x)
    R, K, D = B * 16, 1024, 1024
    z = torch.randn(R, D, device="cuda")
    eng = E._engine(m.encoder)
    img = torch.randn(B, 1, 64, 64, device="cuda")
    out = torch.empty_like(img)
    blk = m.decoder.out_conv[0]
    cn = [ops._p(t.detach()) for t in (blk.dwconv.weight, blk.dwconv.bias, blk.norm.weight, blk.norm.bias, blk.pwconv1.weight, blk.pwconv1.bias,
                                       blk.pwconv2.weight, blk.pwconv2.bias, blk.gamma)]
    en = torch.nn.functional.normalize(m.quantize._codebook.embed.detach(), dim=-1).contiguous()
    full = torch.empty(R, K, device="cuda")
    work = {
        "tokenize_ms": (lambda: m.tokenize(x), 5),
        "decode_tokens_ms": (lambda: m.decode_tokens(tok), 5),
        "search_launch_ms": (lambda: E._assign(m, eng, z, R, 16, B, 4, 4, True), 50),
        "convnext_launch_ms": (lambda: L.check(L.convnext_block(ops._p(img), ops._p(out), *cn, B, 1, 64, 64, 1e-6, ops._stream())), 200),
        "gemm_f32_full_scores_ms": (lambda: ops._gemm_f32(z, en, full, M=R, N=K, K=D), 50),
    }
    for fn, _ in work.values():                      # warm up every shape of the timed window
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in work}
    for _ in range(a.rounds):                        # alternating rounds
        for k, (fn, iters) in work.items():
            samples[k].append(timed(fn, iters))
    res = {"device": torch.cuda.get_device_name(0), "batch": B, "rows": R, "codes": K, "latent_dim": D, "rounds": a.rounds}
    for k, v in samples.items():
        res[k] = {"median": statistics.median(v), "min": min(v)}
    flop = 2.0 * R * K * D
    res["tokenize_instances_per_s"] = B / (res["tokenize_ms"]["median"] * 1e-3)
    res["decode_tokens_instances_per_s"] = B / (res["decode_tokens_ms"]["median"] * 1e-3)
    res["search_tflops_fp32"] = flop / (res["search_launch_ms"]["median"] * 1e-3) / 1e12      # (search + merge + quant gather launches over the product's FLOPs)
    res["gemm_f32_tflops_fp32"] = flop / (res["gemm_f32_full_scores_ms"]["median"] * 1e-3) / 1e12
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
