"""Shared pieces of the LPIPS tests: the seeded weights and inputs of tests/golden/lpips_small.npz (regenerated from the seed, not stored) and
``lpips_ref``, upstream's LPIPS.forward (fourm/vq/percept_losses/lpips.py:96-109, :112-177) restated in plain torch - any float type, under
autograd.  tests/test_lpips_cpu.py pins it to the fixture, which upstream's own unmodified forward wrote (tests/golden/make_golden_lpips.py)."""
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lpips_small.npz")

# (slice, index, C_in, C_out) of the 13 convolutions; a tap follows layers 1, 3, 6, 9, 12 and a 2 x 2 max-pool the first four taps
CONVS = [(1, 0, 3, 64), (1, 2, 64, 64), (2, 5, 64, 128), (2, 7, 128, 128), (3, 10, 128, 256), (3, 12, 256, 256), (3, 14, 256, 256),
         (4, 17, 256, 512), (4, 19, 512, 512), (4, 21, 512, 512), (5, 24, 512, 512), (5, 26, 512, 512), (5, 28, 512, 512)]
TAPS = [1, 3, 6, 9, 12]
CHNS = [64, 128, 256, 512, 512]
CASES = {"b3_32x32": (3, 32, 32), "b2_16x48": (2, 16, 48)}
SEED = 20240


def seeded_state_dict():
    """Upstream's key names and shapes; He-normal convolution weights, 0.1 randn biases, rand / C lin weights (non-negative as the real ones)."""
    g = torch.Generator().manual_seed(SEED)
    sd = {"scaling_layer.shift": torch.tensor([-.030, -.088, -.188])[None, :, None, None],
          "scaling_layer.scale": torch.tensor([.458, .448, .450])[None, :, None, None]}
    for s, idx, cin, cout in CONVS:
        sd[f"net.slice{s}.{idx}.weight"] = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5
        sd[f"net.slice{s}.{idx}.bias"] = 0.1 * torch.randn(cout, generator=g)
    for k, c in enumerate(CHNS):
        sd[f"lin{k}.model.1.weight"] = torch.rand(1, c, 1, 1, generator=g) / c
    return sd


def inputs(case):
    """targets ~ U[-1, 1], preds = targets + 0.3 randn (seeded per case), float32."""
    B, H, W = CASES[case]
    g = torch.Generator().manual_seed(SEED + 1 + sorted(CASES).index(case))
    targets = torch.rand(B, 3, H, W, generator=g) * 2 - 1
    return targets + 0.3 * torch.randn(B, 3, H, W, generator=g), targets


def lpips_features(sd, x, dtype):
    x = (x - sd["scaling_layer.shift"].to(dtype)) / sd["scaling_layer.scale"].to(dtype)
    taps = []
    for li, (s, idx, _, _) in enumerate(CONVS):
        x = F.relu(F.conv2d(x, sd[f"net.slice{s}.{idx}.weight"].to(dtype), sd[f"net.slice{s}.{idx}.bias"].to(dtype), padding=1))
        if li in TAPS:
            taps.append(x)
            if li != TAPS[-1]:
                x = F.max_pool2d(x, kernel_size=2, stride=2)
    return taps


def normalize_tensor(x, eps=1e-10):
    return x / (torch.sqrt(torch.sum(x ** 2, dim=1, keepdim=True)) + eps)


def lpips_ref(sd, preds, targets, dtype):
    """(B, 1, 1, 1): upstream's forward.  Under torch.autocast the convolutions run in bf16 as they would for upstream's module."""
    f0, f1 = lpips_features(sd, preds.to(dtype), dtype), lpips_features(sd, targets.to(dtype), dtype)
    val = None
    for k in range(5):
        diff = (normalize_tensor(f0[k]) - normalize_tensor(f1[k])) ** 2
        res = F.conv2d(diff, sd[f"lin{k}.model.1.weight"].to(dtype)).mean([2, 3], keepdim=True)
        val = res if val is None else val + res
    return val


def ref_run(case, dtype, autocast=False, weights=None):
    """(loss, d (loss . weights).sum() / d preds) of lpips_ref on the CPU."""
    sd = seeded_state_dict()
    preds, targets = inputs(case)
    p = preds.to(dtype).requires_grad_()
    with torch.autocast("cpu", torch.bfloat16, enabled=autocast):
        loss = lpips_ref(sd, p, targets.to(dtype), dtype)
        total = loss.sum() if weights is None else (loss.reshape(-1) * weights.to(loss.dtype)).sum()
    grad, = torch.autograd.grad(total, p)
    return loss.detach(), grad


def rel_max(a, ref):
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return float((a - ref).abs().max() / ref.abs().max())


def rel_l2(a, ref):
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return float((a - ref).norm() / ref.norm())


def load_golden():
    return dict(np.load(GOLDEN))
