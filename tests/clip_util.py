"""Shared pieces of the CLIP vision-tower tests: the two micro towers, a seeded filler for their weights and inputs, and ``vit_forward`` -
a plain-torch restatement of the tower that runs in any float type (float64 is the yardstick of the GPU tests; upstream's own class cannot
run in float64 because its LayerNorm casts to float32, and it is absent where the GPU tests run).

tests/golden/make_golden_clip.py pins the restatement to upstream's class: tests/test_clip_cpu.py checks that it reproduces upstream's fp32
outputs stored in tests/golden/clip_vit_micro.npz."""
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "clip_vit_micro.npz")

# name -> constructor sizes; runs: (tag, batch, height, width).  The first run of each case is the native resolution, the second needs an
# interpolated position table (clip_a: square 64 x 64, 65 rows per image; clip_b: 64 x 48, non-square, 13 rows per image)
CASES = {
    "clip_a": dict(patch_size=8, input_resolution=32, width=128, heads=2, layers=2, output_dim=64),
    "clip_b": dict(patch_size=16, input_resolution=48, width=192, heads=3, layers=1, output_dim=96),
}
RUNS = {
    "clip_a": [("native", 3, 32, 32), ("interp", 2, 64, 64)],
    "clip_b": [("native", 5, 48, 48), ("interp", 2, 64, 48)],
}
FLAGS = ["default", "return_all_tokens", "return_all_final_tokens", "return_final_tokens_no_cls"]
LN_EPS = 1e-5


def flag_kwargs(flag):
    return {} if flag == "default" else {flag: True}


def expected_shapes(case):
    """(key, shape) of the tower's state dict, in module order."""
    c = CASES[case]
    w, p = c["width"], c["patch_size"]
    out = [("class_embedding", (w,)), ("positional_embedding", ((c["input_resolution"] // p) ** 2 + 1, w)), ("proj", (w, c["output_dim"])),
           ("conv1.weight", (w, 3, p, p)), ("ln_pre.weight", (w,)), ("ln_pre.bias", (w,))]
    for i in range(c["layers"]):
        b = f"transformer.resblocks.{i}."
        out += [(b + "attn.in_proj_weight", (3 * w, w)), (b + "attn.in_proj_bias", (3 * w,)), (b + "attn.out_proj.weight", (w, w)),
                (b + "attn.out_proj.bias", (w,)), (b + "ln_1.weight", (w,)), (b + "ln_1.bias", (w,)), (b + "mlp.c_fc.weight", (4 * w, w)),
                (b + "mlp.c_fc.bias", (4 * w,)), (b + "mlp.c_proj.weight", (w, 4 * w)), (b + "mlp.c_proj.bias", (w,)), (b + "ln_2.weight", (w,)),
                (b + "ln_2.bias", (w,))]
    return out + [("ln_post.weight", (w,)), ("ln_post.bias", (w,))]


def seeded_state_dict(case):
    """fp32 weights from a seed (not stored anywhere): matrices at fan-in scale, every bias nonzero (c_fc: std 0.5, so that QuickGELU sees
    both tails), LayerNorm weights 1 +- 0.2 with biases of std 0.1."""
    g = torch.Generator().manual_seed(1000 + sorted(CASES).index(case))
    sd = {}
    for key, shape in expected_shapes(case):
        r = torch.randn(*shape, generator=g)
        if ".ln_" in key or key.startswith("ln_"):
            v = 1.0 + 0.2 * r if key.endswith("weight") else 0.1 * r
        elif key.endswith("c_fc.bias"):
            v = 0.5 * r
        elif key.endswith("bias"):
            v = 0.2 * r
        elif key == "conv1.weight":
            v = r * (shape[1] * shape[2] * shape[3]) ** -0.5
        elif key in ("class_embedding", "positional_embedding"):
            v = 0.5 * r
        elif key == "proj":
            v = r * shape[0] ** -0.5
        else:
            v = r * shape[1] ** -0.5
        sd[key] = v.float().contiguous()
    return sd


def images(case, run):
    tag, B, H, W = next(r for r in RUNS[case] if r[0] == run)
    g = torch.Generator().manual_seed(2000 + 10 * sorted(CASES).index(case) + [r[0] for r in RUNS[case]].index(run))
    return torch.randn(B, 3, H, W, generator=g)


def position_table(pe, gh, gw):
    """Rows of the position table for a (gh, gw) patch grid in pe's float type: the table itself when the token count matches, else the patch
    part resized bicubically with scale factors (g + 0.1) / sqrt(N) (upstream's interpolate_pos_encoding)."""
    n, D = pe.shape[0] - 1, pe.shape[1]
    if gh * gw == n:
        return pe
    side, root = int(math.sqrt(n)), math.sqrt(n)
    grid = F.interpolate(pe[1:].reshape(1, side, side, D).permute(0, 3, 1, 2), scale_factor=((gh + 0.1) / root, (gw + 0.1) / root), mode="bicubic")
    assert tuple(grid.shape[-2:]) == (gh, gw)
    return torch.cat([pe[:1], grid.permute(0, 2, 3, 1).reshape(gh * gw, D)], 0)


def vit_forward(sd, x, flag="default", dtype=torch.float64):
    """The tower as plain tensor algebra in ``dtype``: patch projection, class token, position rows, ln_pre, pre-LN blocks (softmax attention
    with 64-wide heads, QuickGELU MLP), ln_post and the projection; ``flag`` picks one of the four results."""
    p = {k: v.to(dtype) for k, v in sd.items()}
    x = x.to(dtype)
    D, C, P, _ = p["conv1.weight"].shape
    B, _, H, W = x.shape
    gh, gw = H // P, W // P
    G, heads = gh * gw, D // 64

    def ln(t, name):
        return F.layer_norm(t, (D,), p[name + ".weight"], p[name + ".bias"], LN_EPS)

    rows = x.reshape(B, C, gh, P, gw, P).permute(0, 2, 4, 1, 3, 5).reshape(B, G, C * P * P)
    t = rows @ p["conv1.weight"].reshape(D, -1).t()
    t = torch.cat([p["class_embedding"].expand(B, 1, D), t], 1) + position_table(p["positional_embedding"], gh, gw)
    t = ln(t, "ln_pre")
    T = G + 1
    i = 0
    while f"transformer.resblocks.{i}.ln_1.weight" in p:
        b = f"transformer.resblocks.{i}."
        h = ln(t, b + "ln_1")
        q, k, v = (h @ p[b + "attn.in_proj_weight"].t() + p[b + "attn.in_proj_bias"]).reshape(B, T, 3, heads, 64).permute(2, 0, 3, 1, 4)
        a = torch.softmax(q @ k.transpose(-1, -2) * 64 ** -0.5, -1) @ v
        t = t + a.permute(0, 2, 1, 3).reshape(B, T, D) @ p[b + "attn.out_proj.weight"].t() + p[b + "attn.out_proj.bias"]
        u = ln(t, b + "ln_2") @ p[b + "mlp.c_fc.weight"].t() + p[b + "mlp.c_fc.bias"]
        u = u * torch.sigmoid(1.702 * u)
        t = t + u @ p[b + "mlp.c_proj.weight"].t() + p[b + "mlp.c_proj.bias"]
        i += 1
    if flag == "return_all_tokens":
        return ln(t, "ln_post")[:, 1:]
    if flag == "return_all_final_tokens":
        return ln(t, "ln_post") @ p["proj"]
    if flag == "return_final_tokens_no_cls":
        return ln(t, "ln_post")[:, 1:] @ p["proj"]
    assert flag == "default", flag
    return ln(t[:, 0], "ln_post") @ p["proj"]


def rel_max(a, ref):
    """max |a - ref| / max |ref| in float64: the distance the fixture stores and the tests bound."""
    ref = ref.double()
    return float((a.double().cpu() - ref.cpu()).abs().max() / ref.abs().max())


def load_golden():
    return np.load(GOLDEN)
