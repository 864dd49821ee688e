#!/usr/bin/env python3
"""Compile the gfx950 kernels into ml-4m_amd/fourm/_lib/libfourm_hip.so (in-tree, so the object travels
with the snapshot to the GPU box).  hipcc cross-compiles without a GPU."""
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
OUT = os.path.join(HERE, "fourm", "_lib", "libfourm_hip.so")
SOURCES = ["api.cpp", "gemm.hip", "gemm_nt_flat.hip", "gemm_nt3.hip", "gemm_nt4.hip", "gemm_tn4.hip", "gemm_skinny.hip", "layernorm.hip", "attention.hip", "select_embed.hip", "loss.hip", "elementwise.hip", "vq.hip", "convnext.hip", "fp32_verify.hip", "sample.hip", "masking.hip", "unet.hip", "unet_f32.hip", "unet_f32_bwd.hip", "lora.hip", "vit_embed.hip", "attn_decode.hip", "clip.hip", "lpips.hip", "train_objective.hip", "metrics.hip", "resize.hip", "pil_resize.hip", "pil_resize16.hip", "clip_text.hip", "knn.hip", "inception.hip", "lpips_metric.hip", "layerscale.hip", "dinov2.hip"]


# sample.hip: the sampler's determinism contract needs separately rounded fp32 multiplies and adds (no fused multiply-add)
# train_objective.hip: the EMA update, the diffusion training pair and the mask concat are bit-exact against torch's separately rounded kernels
# metrics.hip: the denormalisation in the loads is torch's separately rounded add and halving; the SSIM moments are rounded product by product
# pil_resize.hip: the HOST coefficient tables must come out as Pillow's doubles do, every multiply and add rounded separately
# lpips_metric.hip: every fused multiply-add of the stem's affine and of the distance is written as one; nothing else may be fused
# pil_resize16.hip: the same tables, and Pillow's 16-bit passes accumulate in double on the DEVICE tap by tap: no fused multiply-add there either
EXTRA_FLAGS = {"sample.hip": ["-ffp-contract=off"], "train_objective.hip": ["-ffp-contract=off"], "metrics.hip": ["-ffp-contract=off"], "pil_resize.hip": ["-ffp-contract=off"], "pil_resize16.hip": ["-ffp-contract=off"], "lpips_metric.hip": ["-ffp-contract=off"]}


def hipcc() -> str:
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("hipcc not found")


def up_to_date(srcs) -> bool:
    if not os.path.exists(OUT):
        return False
    t = os.path.getmtime(OUT)
    deps = srcs + [os.path.join(CSRC, "common.h"), os.path.join(CSRC, "gemm_args.h"), os.path.join(CSRC, "agpr_mfma.h"), os.path.join(CSRC, "pil_axis.h"), os.path.join(ROOT, "include", "fourm_hip.h"), __file__]
    return all(os.path.getmtime(d) <= t for d in deps)


def build(force: bool = False, verbose: bool = True) -> str:
    srcs = [os.path.join(CSRC, s) for s in SOURCES if os.path.exists(os.path.join(CSRC, s))]
    if not force and up_to_date(srcs):
        return OUT
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    objs = []
    objdir = os.path.join(HERE, "build")
    os.makedirs(objdir, exist_ok=True)
    procs = []
    for s in srcs:
        o = os.path.join(objdir, os.path.basename(s) + ".o")
        objs.append(o)
        if not force and os.path.exists(o) and os.path.getmtime(o) >= max(
                os.path.getmtime(s), os.path.getmtime(os.path.join(CSRC, "common.h")), os.path.getmtime(os.path.join(CSRC, "gemm_args.h")), os.path.getmtime(os.path.join(CSRC, "agpr_mfma.h")), os.path.getmtime(os.path.join(CSRC, "pil_axis.h")),
                os.path.getmtime(os.path.join(ROOT, "include", "fourm_hip.h"))):
            continue
        cmd = [hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-munsafe-fp-atomics", "-Wno-unused-value",
               "-x", "hip", "-I", os.path.join(ROOT, "include"), "-I", CSRC, "-c", s, "-o", o] + EXTRA_FLAGS.get(os.path.basename(s), [])
        if verbose:
            print(" ".join(cmd), flush=True)
        procs.append((s, subprocess.Popen(cmd)))
    for s, p in procs:
        if p.wait() != 0:
            raise RuntimeError(f"hipcc failed on {s}")
    cmd = [hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", OUT] + objs
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    return OUT


if __name__ == "__main__":
    print(build(force="--force" in sys.argv))
