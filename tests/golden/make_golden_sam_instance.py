#!/usr/bin/env python3
"""Golden fixture for the SAM-instance tokenizer geometry from the UNMODIFIED upstream ``fourm.vq.vqvae.VQVAE`` and
``fourm.vq.models.vit_models.ConvNeXtBlock`` (container only).  Weights, masks and inputs are regenerated from seeds on the test side
(tests/sam_instance_util.py); the fixture keeps upstream's outputs:
  sam_small    VQVAE(vit_s_enc / vit_s_dec, 64 x 64 one-channel masks, patch 16, latent_dim 1024, 1024 codes, norm_codes, out_conv,
               post_mlp), eval, fp32, batch 6: state-dict keys and shapes, the latents fed to the quantizer, tokens, the float64 top-2
               cosine-score margin of every latent row, decode_tokens(tokens)
  convnext_c3  nn.Sequential(ConvNeXtBlock(3), ConvNeXtBlock(3)) on a (2, 3, 40, 56) input, run in float64
    python tests/golden/make_golden_sam_instance.py [--check]"""
import argparse
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
from fourm.vq.models.vit_models import ConvNeXtBlock as RefConvNeXt  # noqa: E402
from fourm.vq.vqvae import VQVAE as RefVQVAE  # noqa: E402

from tests import sam_instance_util as S  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="compare with the committed fixture instead of writing it")
    a = ap.parse_args()
    c = S.SAM_SMALL
    sd, x = S.sam_state_dict(c), S.synthetic_masks(c["batch"], c["image"], seed=c["seed"])
    ref = RefVQVAE(**S.sam_kwargs(c))
    msg = ref.load_state_dict(sd, strict=True)
    assert not msg.missing_keys and not msg.unexpected_keys
    ref.eval()
    with torch.no_grad():
        z = ref.quant_proj(ref.encoder(ref.prepare_input(x))).flatten(2).transpose(1, 2)            # (B, 16, 1024): what the quantizer sees
        quant, _, tokens = ref.encode(x)
        dec = ref.decode_tokens(tokens)
    assert tuple(tokens.shape) == (c["batch"], 4, 4) and tuple(dec.shape) == (c["batch"], 1, c["image"], c["image"])
    z64 = torch.nn.functional.normalize(z.reshape(-1, c["latent"]).double(), dim=-1)
    e64 = torch.nn.functional.normalize(sd["quantize._codebook.embed"].double(), dim=-1)
    top2 = (z64 @ e64.t()).topk(2, dim=-1)
    margin = top2.values[:, 0] - top2.values[:, 1]
    # upstream's fp32 arg-max and the float64 one agree wherever the margin is not a near tie
    u = 2.0 ** -24
    clear = margin > 2 * (c["latent"] + 8) * u
    assert torch.equal(tokens.reshape(-1)[clear], top2.indices[:, 0][clear])
    keys = list(ref.state_dict().keys())
    fx = {"meta/keys": np.array(keys), "meta/shapes": np.array([",".join(map(str, ref.state_dict()[k].shape)) for k in keys]),
          "meta/weight_checksum": np.array(sum(float(v.double().abs().sum()) for v in sd.values())),
          "meta/input_checksum": np.array(float(x.double().abs().sum())),
          "latents": z.numpy().astype(np.float32), "tokens": tokens.numpy().astype(np.int32), "margin64": margin.numpy(),
          "dec_tokens": dec.numpy().astype(np.float32)}
    # the ConvNeXt pair on its own, in double
    cc = S.CONVNEXT_C3
    csd, cx = S.convnext_c3_case(cc)
    seq = torch.nn.Sequential(RefConvNeXt(cc["C"]), RefConvNeXt(cc["C"]))
    msg = seq.load_state_dict(csd, strict=True)
    assert not msg.missing_keys and not msg.unexpected_keys
    seq = seq.double().eval()
    with torch.no_grad():
        y = seq(cx.double())
    fx.update({"convnext_c3/keys": np.array(list(seq.state_dict().keys())), "convnext_c3/out64": y.numpy(),
               "convnext_c3/input_checksum": np.array(float(cx.double().abs().sum()))})
    print(f"[sam_small] {tokens.numel()} tokens, {len(tokens.unique())} distinct; smallest float64 margin {float(margin.min()):.3e}; "
          f"dec range [{float(dec.min()):.3f}, {float(dec.max()):.3f}]; convnext_c3 out range [{float(y.min()):.3f}, {float(y.max()):.3f}]")
    path = os.path.join(HERE, "sam_instance_small.npz")
    if a.check:
        old = np.load(path)
        assert set(old.files) == set(fx), set(old.files) ^ set(fx)
        for k, v in fx.items():
            v = np.asarray(v)
            if v.dtype.kind == "f":        # (upstream's fp32 sums may differ in the last bits between BLAS builds / thread counts)
                np.testing.assert_allclose(v, old[k], rtol=0, atol=1e-5 * max(1.0, float(np.abs(old[k]).max())), err_msg=k)
            else:
                assert np.array_equal(v, old[k]), k
        print("sam_instance_small: fixture reproduced")
        return
    np.savez_compressed(path, **fx)
    print("wrote", path, os.path.getsize(path) // 1024, "KB")


if __name__ == "__main__":
    main()
