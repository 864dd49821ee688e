#!/usr/bin/env python3
"""Throughput of the device-side data stage of dataset pre-tokenization (fourm.data.crops, ml-4m_amd/save_vq_tokens.py) on one GPU.

  crop_resize     64 images of 640 x 480 x 3 with 10 crops each (upstream's settings: centre crop + 9 random crops of scale 0.2 - 1) to 224,
                  bicubic, float32 output: wall time of the whole call (packing on the host, one pinned upload, two launches; synchronised),
                  median of --reps calls after a warm-up (the device time alone is not separated out)
  pillow          the same 640 crops by Pillow (crop + resize + flip, to a uint8 array) on 16 host threads, when Pillow is importable
  script          save_vq_tokens.main on a synthetic folder of --images JPEGs of 640 x 480, 10 crops, a randomly initialised ViT-B tokenizer
                  (224, patch 16, 16 k codes): images per second of its loop (decode on 16 threads, crops and tokens on the device, token files
                  written), second run of two (the first warms the kernels' caches up)

    python tools/bench_pil_crops.py --out profiles/pil_crops_bench.json"""
import argparse
import json
import os
import random
import shutil
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "ml-4m_amd"), ROOT]


def smooth_image(rng, H, W):
    """Low-frequency colour noise (a JPEG of white noise would measure the entropy decoder)."""
    small = rng.integers(0, 256, (H // 16 + 2, W // 16 + 2, 3)).astype(np.float32)
    ys, xs = np.linspace(0, small.shape[0] - 1.001, H), np.linspace(0, small.shape[1] - 1.001, W)
    y0, x0 = ys.astype(int), xs.astype(int)
    fy, fx = (ys - y0)[:, None, None], (xs - x0)[None, :, None]
    a = small[y0][:, x0] * (1 - fy) * (1 - fx) + small[y0 + 1][:, x0] * fy * (1 - fx) + small[y0][:, x0 + 1] * (1 - fy) * fx + small[y0 + 1][:, x0 + 1] * fy * fx
    return np.clip(a + rng.normal(0, 6, a.shape), 0, 255).astype(np.uint8)


def bench_crop_resize(reps):
    import torch
    from fourm.data.crops import crop_resize, make_crop_settings
    rng = np.random.default_rng(0)
    torch.manual_seed(0)
    random.seed(0)
    images = [smooth_image(rng, 480, 640) for _ in range(64)]
    settings = [make_crop_settings(480, 640, 10, 0.2) for _ in images]
    mean = std = (0.5, 0.5, 0.5)
    walls = []
    for it in range(reps + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = crop_resize(images, settings, 224, resample="bicubic", mean=mean, std=std)
        torch.cuda.synchronize()
        if it >= 2:
            walls.append(time.perf_counter() - t0)
    n = out.shape[0]
    res = {"crops": n, "wall_ms_median": 1e3 * statistics.median(walls), "crops_per_s_wall": n / statistics.median(walls), "reps": reps}
    try:
        import PIL
        from PIL import Image
    except ImportError:
        res["pillow"] = "Pillow is not importable here: device figure only"
        return res
    pil = [Image.fromarray(im, mode="RGB") for im in images]

    def one(job):
        i, (top, left, h, w, flip) = job
        a = np.asarray(pil[i].crop((left, top, left + w, top + h)).resize((224, 224), Image.BICUBIC))
        return a[:, ::-1].copy() if flip else a
    jobs = [(i, tuple(int(v) for v in s)) for i, st in enumerate(settings) for s in st]
    times = []
    with ThreadPoolExecutor(max_workers=16) as pool:
        for it in range(4):
            t0 = time.perf_counter()
            got = list(pool.map(one, jobs))
            if it >= 1:
                times.append(time.perf_counter() - t0)
    u8 = crop_resize(images, settings, 224, resample="bicubic", out="uint8").cpu().numpy()
    res["pillow"] = {"threads": 16, "wall_ms_median": 1e3 * statistics.median(times), "crops_per_s": n / statistics.median(times), "version": PIL.__version__,
                     "device_bytes_equal_pillows": bool(all(np.array_equal(a, b) for a, b in zip(u8, got)))}
    return res


def bench_script(n_images):
    import argparse as ap
    import torch
    from PIL import Image
    import save_vq_tokens as S
    from fourm.vq import VQVAE
    tmp = tempfile.mkdtemp(prefix="pil_crops_bench_")
    try:
        rng = np.random.default_rng(1)
        for i in range(n_images):
            d = os.path.join(tmp, "data", "train", "rgb", f"class_{i % 4}")
            os.makedirs(d, exist_ok=True)
            Image.fromarray(smooth_image(rng, 480, 640), mode="RGB").save(os.path.join(d, f"{i:05d}.jpg"), quality=90)
        torch.manual_seed(0)
        m = VQVAE(image_size=224, n_channels=3, enc_type="vit_b_enc", dec_type="vit_s_dec", patch_size=16, codebook_size=16384, latent_dim=32, post_mlp=True)
        args = dict(domain="rgb", input_size=224, encoder_type="vit_b_enc", decoder_type="vit_s_dec", quantizer_type="lucid", patch_size=16, codebook_size=16384,
                    latent_dim=32, num_codebooks=1, norm_codes=True, norm_latents=False, post_mlp=True, quantizer_ema_decay=0.99, lr=1e-4, batch_size=64)
        torch.save({"model": m.state_dict(), "args": ap.Namespace(**args)}, os.path.join(tmp, "tok.pth"))
        argv = ["--data_root", os.path.join(tmp, "data"), "--task", "rgb", "--n_crops", "10", "--min_crop_scale", "0.2", "--tokenizer_ckpt", os.path.join(tmp, "tok.pth"),
                "--folder_suffix", "tok", "--resample_mode", "bicubic"]
        a = S.get_args(argv)
        model = S.load_tokenizer(a)
        runs = []
        for it in range(2):
            shutil.rmtree(os.path.join(tmp, "data", "train", "rgb_tok"), ignore_errors=True)
            t0 = time.perf_counter()
            done, _ = S.main(S.get_args(argv), model=model)
            torch.cuda.synchronize()
            runs.append(time.perf_counter() - t0)
            assert done == n_images
        t0 = time.perf_counter()
        with ThreadPoolExecutor(max_workers=16) as pool:
            list(pool.map(lambda s: S.decode(s[0], "RGB", 0), S.find_samples(os.path.join(tmp, "data", "train", "rgb"))))
        dec = time.perf_counter() - t0
        return {"images": n_images, "n_crops": 10, "seconds_first_run": runs[0], "seconds": runs[1], "images_per_s": n_images / runs[1],
                "crops_per_s": 10 * n_images / runs[1], "decode_only_16_threads_images_per_s": n_images / dec}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=None)
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--images", type=int, default=256)
    a = p.parse_args()
    import torch
    res = {"device": torch.cuda.get_device_name(0), "command": "python tools/bench_pil_crops.py " + " ".join(sys.argv[1:]),
           "crop_resize_64x(480x640x3)x10_to_224_bicubic": bench_crop_resize(a.reps)}
    try:
        res["script_loop"] = bench_script(a.images)
    except ImportError as e:
        res["script_loop"] = f"not measured: {e}"
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
