"""LoRA test helpers shared by the fixture generator (upstream model) and the tests (HIP model): adapters filled from seeds."""
import zlib

import numpy as np
import torch

RANK, SCALE = 4, 0.5
LORA_CASES = ["micro_swiglu", "micro_qknorm"]


def seed_adapters(model, up_std=0.05):
    """Every ``lora_down`` / ``lora_up`` weight from numpy's generator seeded by the parameter's name (the same bits on every machine and
    on both model implementations): down N(0, 1 / rank^2) like the initialisation, up N(0, up_std^2) - non-zero, or every adapter
    gradient but d(lora_up) would be trivially zero."""
    with torch.no_grad():
        for name, p in model.named_parameters():
            if "lora_" not in name:
                continue
            rng = np.random.default_rng(zlib.crc32(name.encode()))
            std = 1.0 / RANK if "lora_down" in name else up_std
            p.copy_(torch.from_numpy((rng.standard_normal(tuple(p.shape)) * std).astype(np.float32)).to(p.device, p.dtype))


def freeze_base(model):
    for name, p in model.named_parameters():
        p.requires_grad = "lora_" in name


def lora_names(model):
    return [n for n, _ in model.named_parameters() if "lora_" in n]
