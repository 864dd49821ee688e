#!/usr/bin/env python3
"""Generate tests/golden/fm_vit_micro.npz from the UNMODIFIED upstream ``fourm/models/fm_vit.py::FourMViT`` on the CPU.

Three micro models (tests/fm_vit_util.py: SwiGLU without biases, GELU with biases and nn.LayerNorm, SwiGLU + QK-norm; dim 128, 2 heads,
depth 2, 32 x 32 images in 8 x 8 patches, batch 3) with weights, input and cotangent from seeds.  Stored per model: the state-dict key
list and shapes, ``no_weight_decay`` / ``get_num_layers``, the output of the fp32 run, of a ``.double()`` copy (as its fp32 difference
from the fp32 one) and of upstream's own ``torch.autocast('cpu', bfloat16)`` run, and for every parameter the gradient of
``sum(out * cotangent)`` (Identity head) from the fp32 and float64 runs - whole for tensors of up to 1024 elements, else on a seeded
sample of 1024 elements - with upstream's own fp32-vs-float64 and autocast-vs-float64 errors on those elements.  For the SwiGLU model
also the composition with a torch head (token mean -> Linear(128, 5)): gradients after one batch and accumulated over two.
The sin-cos position table is stored once.  Runs only where the upstream checkout exists.

    python tests/golden/make_golden_fm_vit.py
"""
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

from fourm.models import fm_utils as ref_utils  # noqa: E402
from fourm.models import fm_vit as ref_vit  # noqa: E402

from tests import fm_vit_util as U  # noqa: E402


class MeanHead(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.fc = torch.nn.Linear(U.DIM, U.CLASSES)

    def forward(self, x):
        return self.fc(x.mean(1))


def grads_of(model, x, cot, autocast=False):
    model.zero_grad()
    if autocast:
        with torch.autocast("cpu", dtype=torch.bfloat16):
            out = model(x)
    else:
        out = model(x)
    (out.to(cot.dtype) * cot).sum().backward()
    return out.detach(), {k: p.grad.detach().clone() for k, p in model.named_parameters()}


def store_grads(out, prefix, g32, g64, gac, n):
    worst = 0.0
    for k in g32:
        idx = U.sample_index(k, g32[k].numel(), n)
        a, b = g32[k].reshape(-1)[idx], g64[k].reshape(-1)[idx]
        out[f"{prefix}/g32/{k}"] = a.numpy()
        out[f"{prefix}/g64_lo/{k}"] = (b - a.double()).float().numpy()          # float64 value = g32 + g64_lo
        out[f"{prefix}/g_err/{k}"] = np.array(float((a.double() - b).abs().max()))
        if gac is not None:
            c = gac[k].reshape(-1)[idx].double()
            out[f"{prefix}/ac_rel/{k}"] = np.array(float((c - b).norm() / b.norm()))
        worst = max(worst, float((a.double() - b).abs().max() / b.abs().max()))
    return worst


def main():
    assert "ml-4m_amd" not in os.path.abspath(ref_vit.__file__), ref_vit.__file__
    out = {}
    x, cot = U.images(0), U.cotangent()
    for name in U.CASES:
        model = ref_vit.FourMViT(**U.model_kwargs(name, ref_utils.LayerNorm))
        sd = U.seeded_state_dict(model)
        model.load_state_dict(sd, strict=True)
        model.train()
        keys = list(model.state_dict().keys())
        out[f"{name}/keys"] = np.array(keys)
        out[f"{name}/shapes"] = np.array([",".join(map(str, model.state_dict()[k].shape)) for k in keys])
        out[f"{name}/param_keys"] = np.array([k for k, _ in model.named_parameters()])
        out[f"{name}/no_weight_decay"] = np.array(sorted(model.no_weight_decay()), dtype=str)
        out[f"{name}/num_layers"] = np.array([model.get_num_layers(), model.get_num_layers_encoder()])
        out[f"{name}/weight_checksum"] = np.array(sum(float(v.double().abs().sum()) for v in sd.values()))
        if "pos_emb" not in out:
            out["pos_emb"] = sd[f"encoder_embeddings.rgb@{U.IMG}.pos_emb"].numpy()
        o32, g32 = grads_of(model, x, cot)
        m64 = copy.deepcopy(model).double()
        o64, g64 = grads_of(m64, x.double(), cot.double())
        oac, gac = grads_of(model, x, cot, autocast=True)
        out[f"{name}/out32"] = o32.numpy()
        out[f"{name}/out64_lo"] = (o64 - o32.double()).float().numpy()
        out[f"{name}/out_err"] = np.array(float((o32.double() - o64).abs().max()))
        out[f"{name}/out_ac"] = oac.float().numpy()
        out[f"{name}/out_ac_rel"] = np.array(float((oac.double() - o64).norm() / o64.norm()))
        worst = store_grads(out, name, g32, g64, gac, U.SAMPLE)
        print(f"[{name}] {len(keys)} keys, out fp32-vs-float64 max abs {float(out[f'{name}/out_err']):.2e}, autocast rel {float(out[f'{name}/out_ac_rel']):.2e}, "
              f"worst gradient fp32-vs-float64 (max abs / max abs) {worst:.2e}")
        if name == "swiglu":          # the composition with a torch head, two batches accumulated
            hs, hcot = U.head_state()
            for dtype, tag in ((torch.float32, "32"), (torch.float64, "64")):
                m = ref_vit.FourMViT(output_head=MeanHead(), **U.model_kwargs(name, ref_utils.LayerNorm))
                m.load_state_dict({**sd, "output_head.fc.weight": hs["weight"], "output_head.fc.bias": hs["bias"]}, strict=True)
                m = m.to(dtype).train()
                res = []
                for b in (0, 1):
                    (m(U.images(b).to(dtype)) * hcot.to(dtype)).sum().backward()
                    res.append({k: p.grad.detach().clone() for k, p in m.named_parameters()})
                out_h = res if tag == "32" else out_h
                if tag == "64":
                    for step, (a, b) in enumerate(zip(out_h, res)):
                        store_grads(out, f"head{step}", a, b, None, U.HEAD_SAMPLE)
    path = os.path.join(HERE, "fm_vit_micro.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB)")


if __name__ == "__main__":
    torch.set_num_threads(min(16, os.cpu_count()))
    main()
