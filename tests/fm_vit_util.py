"""FourMViT test helpers shared by the fixture generator (upstream model) and the tests (HIP model): the three micro configurations,
weights, inputs and cotangents from seeds (numpy's generator: the same bits on every machine), and the seeded element sample of a large
gradient tensor that the fixture stores."""
import zlib
from functools import partial

import numpy as np
import torch

DIM, HEADS, DEPTH, IMG, PATCH, BATCH, CLASSES = 128, 2, 2, 32, 8, 3, 5
NP = (IMG // PATCH) ** 2
SAMPLE = 1024                 # elements of a gradient tensor the fixture keeps (tensors up to this size are kept whole)
HEAD_SAMPLE = 256             # the same for the head composition (two batches)
CASES = {
    "swiglu": dict(gated=True, bias=False, qk_norm=False),
    "gelu": dict(gated=False, bias=True, qk_norm=False),
    "qknorm": dict(gated=True, bias=False, qk_norm=True),
}


def model_kwargs(name, LayerNorm):
    """Constructor arguments of case ``name``; ``LayerNorm`` is the bias-switchable LayerNorm class of the package that builds the model."""
    c = CASES[name]
    kw = dict(img_size=IMG, patch_size=PATCH, in_chans=3, dim=DIM, encoder_depth=DEPTH, num_heads=HEADS, mlp_ratio=4.0, qk_norm=c["qk_norm"],
              qkv_bias=c["bias"], proj_bias=c["bias"], mlp_bias=c["bias"], gated_mlp=c["gated"],
              act_layer=torch.nn.SiLU if c["gated"] else torch.nn.GELU)
    kw["norm_layer"] = partial(torch.nn.LayerNorm, eps=1e-6) if c["bias"] else partial(LayerNorm, eps=1e-6, bias=False)
    return kw


def _normal(tag, shape, std=1.0, mean=0.0):
    rng = np.random.default_rng(zlib.crc32(tag.encode()))
    return torch.from_numpy((rng.standard_normal(tuple(shape)) * std + mean).astype(np.float32))


def seeded_state_dict(model, pos_emb=None):
    """Every PARAMETER of ``model`` from a generator seeded by its name; buffers (the sin-cos table, the all-zero bias of a bias-free
    norm) keep their values, except ``pos_emb`` which is replaced when given (upstream's table from the fixture)."""
    params = dict(model.named_parameters())
    sd = {}
    for k, v in model.state_dict().items():
        if k not in params:
            sd[k] = pos_emb.clone() if (pos_emb is not None and k.endswith("pos_emb")) else v.clone()
        elif k.endswith("mod_emb"):
            sd[k] = _normal(k, v.shape, 0.02)
        elif v.dim() >= 2:
            sd[k] = _normal(k, v.shape, 0.06)
        elif "norm" in k and k.endswith("weight"):
            sd[k] = _normal(k, v.shape, 0.1, 1.0)
        else:
            sd[k] = _normal(k, v.shape, 0.05)
    return sd


def images(batch=0):
    return _normal(f"fm_vit.images.{batch}", (BATCH, 3, IMG, IMG))


def cotangent():
    return _normal("fm_vit.cotangent", (BATCH, NP, DIM), 1.0 / 16)


def head_state():
    """Linear(DIM, CLASSES) on the token mean, and the fixed cotangent of its output."""
    return {"weight": _normal("fm_vit.head.weight", (CLASSES, DIM), 0.1), "bias": _normal("fm_vit.head.bias", (CLASSES,), 0.1)}, _normal("fm_vit.head.cot", (BATCH, CLASSES))


def sample_index(key, numel, n=SAMPLE):
    """Sorted flat indices of the elements of tensor ``key`` the fixture keeps: all of a small tensor, else ``n`` drawn without replacement."""
    if numel <= n:
        return np.arange(numel)
    return np.sort(np.random.default_rng(zlib.crc32(("sample." + key).encode())).choice(numel, size=n, replace=False))
