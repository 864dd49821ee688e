"""Yardstick of the DiVAE decoder's training step: TEST INFRASTRUCTURE shared by tests/test_divae_train_cpu.py and test_divae_train_gpu.py.

The reference of every parameter gradient is float64 autograd on the CPU through tests/divae_f64_util.unet_forward (pinned to upstream's
fixture, tests/test_divae_fp32_cpu.py); the fp32 side of the rule is the same function in float32 on the CPU.  The rule, for every gradient
tensor:   max |HIP - float64|  <=  8 x max(max |float32 on the CPU - float64|, 2^-24 max |float64|)
(the factor of tests/test_divae_fp32_gpu.py; the floor is half an fp32 ulp of the tensor's largest entry, below which no fp32 result can be
asked to go).  loss = F.mse_loss(out, target) with a seeded randn target, summed over the evaluations of a case."""
import functools
import os

import numpy as np
import torch
import torch.nn.functional as F

from oracle import divae_oracle as DO
from tests import divae_f64_util as F64
from tests.parity_log import record

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "divae_small.npz")
FACTOR = 8.0
SMALL = dict(image_size=32, in_channels=3, out_channels=3, cond_channels=8, patch_size=4, model_channels=64, num_res_blocks=1,
             attention_resolutions=(2,), channel_mult=(1, 2))        # = tests/test_divae.py SMALL: 128 tensors
# three Downs and three Ups, attention on 16 and on 4 tokens in both halves, the skip stack with two blocks per level: 334 tensors
MID = dict(image_size=64, in_channels=3, out_channels=3, cond_channels=8, patch_size=4, model_channels=64, num_res_blocks=2,
           attention_resolutions=(4, 8), channel_mult=(1, 2, 2, 2))
CONFIGS = dict(small=(SMALL, 3), mid=(MID, 5))                      # configuration, seed of the weights


def state_dict(cfg_name):
    kw, seed = CONFIGS[cfg_name]
    return DO.seeded_unet_state_dict(DO.UNetCfg(**kw), seed=seed)


def target_for(x, seed):
    return torch.randn(x.shape, generator=torch.Generator().manual_seed(seed))


@functools.lru_cache(maxsize=None)
def case(name):
    """(configuration name, [(sample, timesteps, conditioning, mask or None, target), ...]): the evaluations whose losses are summed."""
    if name in ("small", "small_masked", "small_two"):
        fx = np.load(GOLD)
        x, cond, ts, mask = (torch.from_numpy(fx[k]) for k in ("x", "cond", "ts", "mask"))      # B = 3, per-sample timesteps
        evals = [(x, ts, cond, mask if name == "small_masked" else None, target_for(x, 11))]
        if name == "small_two":                                   # two live graphs: loss(net(x1)) + loss(net(x2))
            x2 = torch.randn(x.shape, generator=torch.Generator().manual_seed(12))
            evals.append((x2, torch.tensor([3, 500, 998]), cond.flip(0).contiguous(), None, target_for(x, 13)))
        return "small", evals
    if name == "mid":
        g = torch.Generator().manual_seed(21)
        x, cond = torch.randn(2, 3, 64, 64, generator=g), torch.randn(2, 8, 4, 4, generator=g)
        return "mid", [(x, torch.tensor([777, 31]), cond, None, target_for(x, 22))]
    raise KeyError(name)


def cpu_grads(name, dtype):
    cfg_name, evals = case(name)
    cfg = DO.UNetCfg(**CONFIGS[cfg_name][0])
    P = {k: v.clone().requires_grad_(True) for k, v in F64.cast_state(state_dict(cfg_name), dtype).items()}
    loss = sum(F.mse_loss(F64.unet_forward(P, cfg, x, t, c, m, dtype=dtype), tgt.to(dtype)) for x, t, c, m, tgt in evals)
    loss.backward()
    return {k: v.grad.detach() for k, v in P.items()}


@functools.lru_cache(maxsize=None)
def yardstick(name):
    """{parameter: (float64 gradient, bound of the rule, the fp32 CPU error, the floor)}: computed once per case, shared, never modified."""
    g64, g32 = cpu_grads(name, torch.float64), cpu_grads(name, torch.float32)
    out = {}
    for k, ref in g64.items():
        own = float((g32[k].double() - ref).abs().max())
        floor = 2.0 ** -24 * float(ref.abs().max())
        out[k] = (ref, FACTOR * max(own, floor), own, floor)
    return out


def under_the_rule(case_name, got, ref_case=None, only=None):
    """got: {parameter: fp32 gradient}.  Records every ratio, then asserts all of them; returns the largest err / max(own, floor)."""
    ys = yardstick(ref_case or case_name)
    keys = list(ys) if only is None else list(only)
    assert only is not None or set(got) == set(ys), set(got) ^ set(ys)
    worst, bad = 0.0, []
    for k in keys:
        ref, bound, own, floor = ys[k]
        g = got[k]
        assert g.dtype == torch.float32 and tuple(g.shape) == tuple(ref.shape), k
        err = float((g.double().cpu() - ref).abs().max())
        ratio = err / max(own, floor)
        record("divae.fp32.grad", case=case_name, tensor=k, err_vs_float64=err, cpu_fp32_err_vs_float64=own, floor=floor, ratio=ratio)
        worst = max(worst, ratio)
        if not err <= bound:
            bad.append((k, err, own, floor, ratio))
    print(f"{case_name}: {len(keys)} gradient tensors, largest err / max(own, floor) = {worst:.3g} (bound {FACTOR:g})")
    assert not bad, bad[:8]
    return worst
