"""What the SAM-instance tokenizer tests and their fixture generator (tests/golden/make_golden_sam_instance.py) share: the small
configuration (64 x 64 one-channel masks, patch 16, latent_dim 1024, 1024 codes, out_conv), its seeded state dict in upstream's
layout, seeded ConvNeXt parameters and synthetic binary masks.  Everything is regenerated from seeds on both sides; the fixture keeps
upstream's outputs only."""
import math

import torch

from oracle import vq_oracle as V
from oracle.fourm_oracle import seeded_tensor

SAM_SMALL = dict(enc_type="vit_s_enc", dec_type="vit_s_dec", image=64, patch=16, channels=1, latent=1024, codebook=1024, post_mlp=True, batch=6, seed=7)


def sam_cfg(c=SAM_SMALL):
    return V.vq_cfg(c["enc_type"], image=c["image"], patch=c["patch"], codebook=c["codebook"], post_mlp=c["post_mlp"], channels=c["channels"],
                    latent=c["latent"])


def sam_kwargs(c=SAM_SMALL):
    """Constructor arguments of the case, identical for upstream's VQVAE and this package's."""
    return dict(enc_type=c["enc_type"], dec_type=c["dec_type"], image_size=c["image"], n_channels=c["channels"], patch_size=c["patch"],
                latent_dim=c["latent"], codebook_size=c["codebook"], norm_codes=True, out_conv=True, post_mlp=c["post_mlp"], sync_codebook=False)


def convnext_state(prefix, C, seed=0):
    """One ConvNeXtBlock(C) in upstream's names.  gamma of order 1 (upstream's initial 1e-6 would hide the whole branch at any tolerance);
    LayerNorm affine and every bias non-trivial."""
    p = prefix + "." if prefix else ""
    return {
        p + "dwconv.weight": seeded_tensor(p + "dwconv.weight", (C, 1, 7, 7), 1.0 / 7.0, seed),
        p + "dwconv.bias": seeded_tensor(p + "dwconv.bias", (C,), 0.1, seed),
        p + "norm.weight": 1.0 + seeded_tensor(p + "norm.weight", (C,), 0.2, seed),
        p + "norm.bias": seeded_tensor(p + "norm.bias", (C,), 0.3, seed),
        p + "pwconv1.weight": seeded_tensor(p + "pwconv1.weight", (4 * C, C), 1.0 / math.sqrt(C), seed),
        p + "pwconv1.bias": seeded_tensor(p + "pwconv1.bias", (4 * C,), 0.3, seed),
        p + "pwconv2.weight": seeded_tensor(p + "pwconv2.weight", (C, 4 * C), 1.0 / math.sqrt(4 * C), seed),
        p + "pwconv2.bias": seeded_tensor(p + "pwconv2.bias", (C,), 0.1, seed),
        p + "gamma": 1.0 + seeded_tensor(p + "gamma", (C,), 0.3, seed),
    }


def sam_state_dict(c=SAM_SMALL):
    cfg = sam_cfg(c)
    sd = V.seeded_vqvae_state_dict(cfg, c["dec_type"], seed=c["seed"])
    for i in range(2):
        sd.update(convnext_state(f"decoder.out_conv.{i}", c["channels"], c["seed"]))
    return sd


def synthetic_masks(batch, size, seed=0):
    """(batch, 1, size, size) f32 binary masks in {0, 1}: one filled ellipse or rectangle each, position and extent from the seed."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(size, dtype=torch.float32), torch.arange(size, dtype=torch.float32), indexing="ij")
    out = torch.zeros(batch, 1, size, size)
    for b in range(batch):
        cy, cx = (torch.rand(2, generator=g) * 0.5 + 0.25) * size
        ry, rx = (torch.rand(2, generator=g) * 0.3 + 0.1) * size
        if b % 2 == 0:
            m = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
        else:
            m = ((yy - cy).abs() <= ry) & ((xx - cx).abs() <= rx)
        out[b, 0] = m.float()
    return out


CONVNEXT_C3 = dict(C=3, shape=(2, 3, 40, 56), seed=11)


def convnext_c3_case(c=CONVNEXT_C3):
    """State dict of nn.Sequential(ConvNeXtBlock(3), ConvNeXtBlock(3)) (keys '0.*', '1.*') and its input."""
    sd = {}
    for i in range(2):
        sd.update(convnext_state(str(i), c["C"], c["seed"]))
    x = seeded_tensor("convnext_c3.input", c["shape"], 1.0, c["seed"])
    return sd, x
