#!/usr/bin/env python3
"""Writes tests/golden/lpips_small.npz from upstream's UNMODIFIED LPIPS.forward (fourm/vq/percept_losses/lpips.py:96-109), built without its
downloading ``__init__``: ``LPIPS.__new__`` + ``nn.Module.__init__``, upstream's own ScalingLayer and NetLinLayer, and a ``net`` made of the
five torch slices (torchvision, requests and tqdm are inert stand-ins: none takes part in the arithmetic).  Weights and inputs are the seeded
ones of tests/lpips_util.py; stored are upstream's state-dict key names and shapes and, per case, the float64 loss and pixel gradient.

Run in the build container, where the upstream tree is available:  python tests/golden/make_golden_lpips.py"""
import importlib.machinery
import os
import sys
import types
from collections import namedtuple

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import ref_stubs  # noqa: E402
from tests import lpips_util as LU  # noqa: E402


def upstream_lpips_module():
    """fourm/vq/percept_losses/lpips.py loaded as a lone file (its package's __init__ pulls in timm)."""
    ref_stubs.install()
    for name in ("requests", "tqdm"):
        if name not in sys.modules:
            m = ref_stubs._Inert(name)
            m.__spec__ = importlib.machinery.ModuleSpec(name, loader=None)
            sys.modules[name] = m
    path = os.path.join(ref_stubs.REFERENCE_ROOT, "fourm", "vq", "percept_losses", "lpips.py")
    mod = types.ModuleType("upstream_lpips")
    mod.__file__ = path
    exec(compile(open(path).read(), path, "exec"), mod.__dict__)
    return mod


class Slices(nn.Module):
    """What upstream's vgg16 wrapper holds, without torchvision: the five slices of vgg16.features with their original indices."""

    def __init__(self):
        super().__init__()
        layout = {1: [0, "r", 2, "r"], 2: ["p", 5, "r", 7, "r"], 3: ["p", 10, "r", 12, "r", 14, "r"], 4: ["p", 17, "r", 19, "r", 21, "r"],
                  5: ["p", 24, "r", 26, "r", 28, "r"]}
        first = {1: 0, 2: 4, 3: 9, 4: 16, 5: 23}
        chan = {idx: (cin, cout) for _, idx, cin, cout in LU.CONVS}
        for s, items in layout.items():
            seq = nn.Sequential()
            for off, it in enumerate(items):
                layer = nn.ReLU(inplace=False) if it == "r" else nn.MaxPool2d(kernel_size=2, stride=2) if it == "p" else nn.Conv2d(*chan[it], kernel_size=3, padding=1)
                seq.add_module(str(first[s] + off), layer)
            setattr(self, f"slice{s}", seq)

    def forward(self, X):
        outs = []
        h = X
        for s in range(1, 6):
            h = getattr(self, f"slice{s}")(h)
            outs.append(h)
        return namedtuple("VggOutputs", ["relu1_2", "relu2_2", "relu3_3", "relu4_3", "relu5_3"])(*outs)


def build_upstream(up):
    m = up.LPIPS.__new__(up.LPIPS)
    nn.Module.__init__(m)
    m.scaling_layer = up.ScalingLayer()
    m.chns = [64, 128, 256, 512, 512]
    m.net = Slices()
    for k, c in enumerate(m.chns):
        setattr(m, f"lin{k}", up.NetLinLayer(c, use_dropout=True))
    return m


def main():
    up = upstream_lpips_module()
    model = build_upstream(up)
    model.load_state_dict(LU.seeded_state_dict(), strict=True)
    model = model.double().eval()
    out = {}
    for k, v in model.state_dict().items():
        out["shape/" + k] = np.asarray(v.shape, dtype=np.int64)
    out["keys"] = np.asarray(list(model.state_dict().keys()))
    for case in LU.CASES:
        preds, targets = LU.inputs(case)
        p = preds.double().requires_grad_()
        loss = model(p, targets.double())
        grad, = torch.autograd.grad(loss.sum(), p)
        out[f"{case}/loss"] = loss.detach().numpy()
        out[f"{case}/grad"] = grad.numpy()
        print(case, tuple(loss.shape), loss.reshape(-1).tolist())
    np.savez_compressed(LU.GOLDEN, **out)
    print("wrote", LU.GOLDEN, os.path.getsize(LU.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
