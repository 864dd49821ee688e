#!/usr/bin/env python3
"""Golden fixture for the MLP + Memcodes tokenizers (human poses, DINOv2 / ImageBind global features) from the UNMODIFIED upstream
``fourm.vq.vqvae.VQVAE`` (container only).  Weights and inputs are regenerated from seeds on the test side (tests/memcodes_util.py); the
fixture keeps upstream's outputs.  Per case (bmlp_small, mlp_small):
  keys / shapes of upstream's state_dict, weight and input checksums;
  per input grid (g1: batch 5, 1 x 1; g3: batch 2, 1 x 3): the fp32 latents fed to the quantizer, tokens, quant, the latents of a .double()
  copy of the model, upstream's own fp32-vs-float64 relative error of the latents, and for every (row, head) the float64 top-2 score margin
  and arg-max of the fp32 latents and of the float64 latents;
  g1 only: decode_tokens(tokens) in fp32 and from the .double() copy, and upstream's own relative error of it.
The generator asserts that upstream's fp32 tokens equal the float64 arg-max wherever the margin exceeds 2 d u |z_h| max_j |k_hj| (u = 2^-24),
and that at most 2 % of the (row, head) pairs fall under that margin.
    python tests/golden/make_golden_memcodes.py [--check]"""
import argparse
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import ref_stubs  # noqa: E402

ref_stubs.install()
from fourm.vq.vqvae import VQVAE as RefVQVAE  # noqa: E402

from tests import memcodes_util as M  # noqa: E402


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def latents(model, x):
    """What the quantizer sees: (B h w, latent_dim)."""
    return M.rows_of(model.quant_proj(model.encoder(model.prepare_input(x))))


def case_fixture(name, c):
    sd, xs = M.state_dict(c), M.inputs(name, c)
    ref = RefVQVAE(**M.kwargs(c))
    msg = ref.load_state_dict(sd, strict=True)
    assert not msg.missing_keys and not msg.unexpected_keys
    ref.eval()
    ref64 = copy.deepcopy(ref).double().eval()
    keys = list(ref.state_dict().keys())
    fx = {"keys": np.array(keys), "shapes": np.array([",".join(map(str, ref.state_dict()[k].shape)) for k in keys]),
          "weight_checksum": np.array(M.checksum(sd.values())), "input_checksum": np.array(M.checksum(xs.values()))}
    k64, _ = M.keys64(sd)
    H, d = c["heads"], c["latent"] // c["heads"]
    under = total = 0
    for tag, B, h, w in M.INPUTS:
        x = xs[tag]
        with torch.no_grad():
            z = latents(ref, x)
            quant, loss, tokens = ref.encode(x)
            z64 = latents(ref64, x.double())
        assert tuple(tokens.shape) == (B, H, h, w) and tuple(quant.shape) == (B, c["latent"], h, w) and float(loss) == 0.0
        best, margin = M.margins64(M.head_scores64(z, k64))
        best_z64, margin_z64 = M.margins64(M.head_scores64(z64, k64))
        clear = margin > 2 * M.score_bound(z, k64)
        assert torch.equal(M.tokens_rows(tokens)[clear], best[clear]), (name, tag)
        under += int((~clear).sum())
        total += clear.numel()
        fx.update({f"{tag}/latents": z.numpy(), f"{tag}/tokens": tokens.numpy().astype(np.int32), f"{tag}/quant": quant.numpy(),
                   f"{tag}/latents64": z64.numpy(), f"{tag}/latents_rel": np.array(rel(z, z64)),
                   f"{tag}/margin64": margin.numpy(), f"{tag}/argmax64": best.numpy().astype(np.int32),
                   f"{tag}/margin64_z64": margin_z64.numpy(), f"{tag}/argmax64_z64": best_z64.numpy().astype(np.int32)})
        if (h, w) == (1, 1):
            with torch.no_grad():
                dec = ref.decode_tokens(tokens)
                dec64 = ref64.decode_tokens(tokens)
                assert torch.equal(ref.tokens_to_embedding(tokens), quant) and rel(ref(x)[0], dec) < 1e-5      # (forward's quant has another memory layout: upstream's BLAS sums differ in the last bits)
            assert tuple(dec.shape) == (B, c["channels"], 1, 1)
            fx.update({f"{tag}/dec_tokens": dec.numpy(), f"{tag}/dec_tokens64": dec64.numpy(), f"{tag}/dec_rel": np.array(rel(dec, dec64))})
            print(f"[{name}] {tag}: latents fp32-vs-float64 {rel(z, z64):.3e}, reconstruction {rel(dec, dec64):.3e}, smallest margin {float(margin.min()):.3e}")
    assert under <= 0.02 * total, f"{name}: {under} of {total} (row, head) pairs under the margin; change the seed or scale"
    return {f"{name}/{k}": v for k, v in fx.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="compare with the committed fixture instead of writing it")
    a = ap.parse_args()
    fx = {}
    for name, c in M.CASES.items():
        fx.update(case_fixture(name, c))
    path = os.path.join(HERE, "memcodes_small.npz")
    if a.check:
        old = np.load(path)
        assert set(old.files) == set(fx), set(old.files) ^ set(fx)
        for k, v in fx.items():
            v = np.asarray(v)
            if k.endswith("_rel"):           # (a ratio of rounding errors: its size is reproduced, not its digits)
                assert 0.25 * float(old[k]) <= float(v) <= 4.0 * float(old[k]), k
            elif v.dtype.kind == "f":        # (upstream's fp32 sums may differ in the last bits between BLAS builds / thread counts)
                np.testing.assert_allclose(v, old[k], rtol=0, atol=1e-5 * max(1.0, float(np.abs(old[k][np.isfinite(old[k])]).max())), err_msg=k)
            else:
                assert np.array_equal(v, old[k]), k
        print("memcodes_small: fixture reproduced")
        return
    np.savez_compressed(path, **fx)
    print("wrote", path, os.path.getsize(path) // 1024, "KB")


if __name__ == "__main__":
    main()
