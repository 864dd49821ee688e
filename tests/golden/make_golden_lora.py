#!/usr/bin/env python3
"""Generate tests/golden/lora_micro.npz from the UNMODIFIED upstream FourM and upstream fourm/models/lora_utils.py.

For micro_swiglu and micro_qknorm (tests/golden/cases.py): inject LoRA (rank 4, scale 0.5, attention modules), fill the adapters from
seeds (tests/lora_util.py), run forward + backward in fp32 and again on a ``.double()`` copy.  Stored per case: the state-dict key list
and shapes, loss and logits (fp32 run), the gradient of every ``lora_*`` parameter from both runs (the float64 one as its fp32 difference from the fp32 one) and upstream's own fp32-vs-float64
relative error of each.  Runs only where the upstream checkout exists.

    python tests/golden/make_golden_lora.py
"""
import copy
import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import make_golden as MG  # noqa: E402  (installs the stubs and puts the upstream package on the path)
from fourm.models import lora_utils as ref_lora  # noqa: E402

from tests.golden.cases import build_case  # noqa: E402
from tests.lora_util import LORA_CASES, RANK, SCALE, seed_adapters  # noqa: E402


def cast_mod_dict(md, dtype):
    return {k: {a: (b.to(dtype) if b.is_floating_point() else b.clone()) for a, b in v.items()} for k, v in md.items()}


def run(model, case, dtype):
    model.train()
    model.zero_grad()
    random.seed(case["order_seed"])
    loss, _ = model(cast_mod_dict(case["mod_dict"], dtype), case["N"], case["M"], loss_type=case["loss_type"])
    loss.sum().backward()
    grads = {k: p.grad.detach().clone() for k, p in model.named_parameters() if "lora_" in k}
    random.seed(case["order_seed"])
    with torch.no_grad():
        logits = model(cast_mod_dict(case["mod_dict"], dtype), case["N"], case["M"], return_logits=True)
    return loss.detach().sum(), logits, grads


def main():
    assert "reference" in os.path.abspath(ref_lora.__file__) or "ml-4m_amd" not in os.path.abspath(ref_lora.__file__), ref_lora.__file__
    out = {}
    for name in LORA_CASES:
        case = build_case(name)
        model = MG.upstream_model(case["cfg"], case["share_embedding"], case["norm_bias"], case["learned_pos"])
        model.load_state_dict(case["sd"], strict=True)
        ref_lora.inject_trainable_LoRA(model, rank=RANK, scale=SCALE, target_replace_modules=ref_lora.get_LoRA_module_names("attn"))
        seed_adapters(model)
        keys = list(model.state_dict().keys())
        out[f"{name}/keys"] = np.array(keys)
        out[f"{name}/shapes"] = np.array([",".join(map(str, model.state_dict()[k].shape)) for k in keys])
        loss, logits, grads = run(model, case, torch.float32)
        loss64, logits64, grads64 = run(copy.deepcopy(model).double(), case, torch.float64)
        out[f"{name}/loss"] = np.array(float(loss), dtype=np.float32)
        out[f"{name}/loss64"] = np.array(float(loss64))
        for k, v in logits.items():
            out[f"{name}/logits/{k}"] = v.numpy().astype(np.float32)
        worst = 0.0
        for k, g in grads.items():
            g64 = grads64[k]
            rel = float((g.double() - g64).norm() / g64.norm())
            worst = max(worst, rel)
            out[f"{name}/grad/{k}"] = g.numpy()
            out[f"{name}/grad64_lo/{k}"] = (g64 - g.double()).float().numpy()      # float64 gradient = grad + grad64_lo (half the bytes of a float64 array)
            out[f"{name}/grad_rel/{k}"] = np.array(rel)
        print(f"[{name}] loss {float(loss):.6f} (float64 {float(loss64):.6f}), {len(grads)} adapter gradients, worst fp32-vs-float64 {worst:.2e}")
    path = os.path.join(HERE, "lora_micro.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB)")


if __name__ == "__main__":
    torch.set_num_threads(min(16, os.cpu_count()))
    main()
