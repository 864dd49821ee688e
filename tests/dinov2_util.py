"""Shared pieces of the DINOv2 tower tests: two micro towers, a seeded filler for their weights and inputs, and ``dino_forward`` - a
plain-torch restatement of the definition in INTEGRATION.md ("DINOv2 tower") that runs in float64 (the yardstick of the GPU tests), in fp32
and under CPU bf16 autocast.  The `facebookresearch/dinov2` package is not available where these tests run: parity with the package and with
the real checkpoints is unpinned, the written definition is the contract.

tests/golden/make_golden_dinov2.py stores the restatement's own fp32 and autocast distances from float64 in tests/golden/dinov2_micro.npz."""
import os

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "dinov2_micro.npz")

# dino_a: M = 5, plain MLP, no registers, scale-factor interpolation (offset 0.1).  dino_b: M = 3, fused SwiGLU (hidden 512), 4 registers,
# antialiased size interpolation (offset 0).  runs: (tag, batch, height, width)
CASES = {
    "dino_a": dict(img_size=70, patch_size=14, embed_dim=128, depth=2, num_heads=2, ffn_layer="mlp", num_register_tokens=0,
                   interpolate_antialias=False, interpolate_offset=0.1),
    "dino_b": dict(img_size=42, patch_size=14, embed_dim=192, depth=1, num_heads=3, ffn_layer="swiglufused", num_register_tokens=4,
                   interpolate_antialias=True, interpolate_offset=0.0),
}
RUNS = {
    "dino_a": [("native", 2, 70, 70), ("interp", 3, 56, 84)],          # T = 26 (the table unchanged); grid 4 x 6, T = 25
    "dino_b": [("interp", 2, 28, 28), ("native", 2, 42, 42)],          # T = 1 + 4 + 4 = 9; T = 14
}
RESULTS = ["x_norm_clstoken", "x_norm_regtokens", "x_norm_patchtokens", "x_prenorm"]
LN_EPS = 1e-6


def results_of(case):
    return [r for r in RESULTS if r != "x_norm_regtokens" or CASES[case]["num_register_tokens"]]


def swiglu_hidden(D):
    return (int(4 * D * 2 / 3) + 7) // 8 * 8


def expected_shapes(cfg):
    """(key, shape) of the tower's state dict for constructor arguments ``cfg``."""
    D, P, Rn = cfg["embed_dim"], cfg["patch_size"], cfg.get("num_register_tokens", 0)
    M = cfg["img_size"] // P
    out = [("cls_token", (1, 1, D)), ("pos_embed", (1, 1 + M * M, D)), ("mask_token", (1, D))]
    if Rn:
        out.append(("register_tokens", (1, Rn, D)))
    out += [("patch_embed.proj.weight", (D, 3, P, P)), ("patch_embed.proj.bias", (D,))]
    for i in range(cfg["depth"]):
        b = f"blocks.{i}."
        out += [(b + "norm1.weight", (D,)), (b + "norm1.bias", (D,)), (b + "attn.qkv.weight", (3 * D, D)), (b + "attn.qkv.bias", (3 * D,)),
                (b + "attn.proj.weight", (D, D)), (b + "attn.proj.bias", (D,)), (b + "ls1.gamma", (D,)), (b + "norm2.weight", (D,)),
                (b + "norm2.bias", (D,)), (b + "ls2.gamma", (D,))]
        if cfg["ffn_layer"] == "mlp":
            out += [(b + "mlp.fc1.weight", (4 * D, D)), (b + "mlp.fc1.bias", (4 * D,)), (b + "mlp.fc2.weight", (D, 4 * D)), (b + "mlp.fc2.bias", (D,))]
        else:
            h = swiglu_hidden(D)
            out += [(b + "mlp.w12.weight", (2 * h, D)), (b + "mlp.w12.bias", (2 * h,)), (b + "mlp.w3.weight", (D, h)), (b + "mlp.w3.bias", (D,))]
    return out + [("norm.weight", (D,)), ("norm.bias", (D,))]


def seeded_state_dict(case):
    """fp32 weights from a seed (not stored anywhere): matrices at fan-in scale, every bias nonzero, LayerNorm weights 1 +- 0.2 with biases of
    std 0.1, tokens and positions of std 0.5, and the LayerScale gammas uniform in [-1.5, 1.5] - a dropped or misplaced LayerScale cannot pass."""
    g = torch.Generator().manual_seed(3000 + sorted(CASES).index(case))
    sd = {}
    for key, shape in expected_shapes(CASES[case]):
        r = torch.randn(*shape, generator=g)
        if key.endswith("gamma"):
            v = 3.0 * torch.rand(*shape, generator=g) - 1.5
        elif "norm" in key:
            v = 1.0 + 0.2 * r if key.endswith("weight") else 0.1 * r
        elif key.endswith("fc1.bias") or key.endswith("w12.bias"):
            v = 0.5 * r
        elif key.endswith("bias"):
            v = 0.2 * r
        elif key == "patch_embed.proj.weight":
            v = r * (shape[1] * shape[2] * shape[3]) ** -0.5
        elif key in ("cls_token", "pos_embed", "register_tokens", "mask_token"):
            v = 0.5 * r
        else:
            v = r * shape[1] ** -0.5
        sd[key] = v.float().contiguous()
    return sd


def images(case, run):
    tag, B, H, W = next(r for r in RUNS[case] if r[0] == run)
    g = torch.Generator().manual_seed(4000 + 10 * sorted(CASES).index(case) + [r[0] for r in RUNS[case]].index(run))
    return torch.randn(B, 3, H, W, generator=g)


def position_rows(pe, gh, gw, antialias, offset):
    """pos(gh, gw) in pe's float type: (1 + gh * gw, D)."""
    pe = pe[0]
    n, D = pe.shape[0] - 1, pe.shape[1]
    M = int(round(n ** 0.5))
    if gh * gw == n and gh == gw:
        return pe
    grid = pe[1:].reshape(1, M, M, D).permute(0, 3, 1, 2)
    kw = dict(scale_factor=(float(gh + offset) / M, float(gw + offset) / M)) if offset else dict(size=(gh, gw))
    grid = F.interpolate(grid, mode="bicubic", antialias=antialias, **kw)
    assert tuple(grid.shape[-2:]) == (gh, gw)
    return torch.cat([pe[:1], grid.permute(0, 2, 3, 1).reshape(gh * gw, D)], 0)


def bicubic_rule(table, gh, gw, offset):
    """The scale-factor / size form without antialias written out, float64: a bicubic with A = -0.75, clamped borders and source coordinate
    (i + 0.5) * M / (g + offset) - 0.5 per axis.  table (D, M, M) -> (D, gh, gw)."""
    A = -0.75

    def weights(t):
        def near(x):
            return ((A + 2) * x - (A + 3)) * x * x + 1

        def far(x):
            return ((A * x - 5 * A) * x + 8 * A) * x - 4 * A
        return [far(t + 1), near(t), near(1 - t), far(2 - t)]

    def axis(M, g):
        rows = torch.zeros(g, M, dtype=torch.float64)
        for i in range(g):
            src = (i + 0.5) * M / (g + offset) - 0.5
            i0 = int(np.floor(src))
            for k, w in enumerate(weights(src - i0)):
                rows[i, min(max(i0 - 1 + k, 0), M - 1)] += w
        return rows
    t = table.double()
    return torch.einsum("ip,dpq,jq->dij", axis(t.shape[1], gh), t, axis(t.shape[2], gw))


def dino_forward(case_or_cfg, sd, x, dtype=torch.float64, autocast=False):
    """The tower as plain torch.  ``dtype``: the float type of parameters and input (float64 / float32); ``autocast``: fp32 parameters under
    torch.autocast(bfloat16) on x's device - linear, conv and matmul in bf16, LayerNorm and softmax in fp32, gamma (fp32) * branch (bf16) promoted to
    fp32, fp32 residual stream.  Returns the four results plus ``layers``: the residual stream after every block (before the final norm)."""
    cfg = CASES[case_or_cfg] if isinstance(case_or_cfg, str) else case_or_cfg
    dtype = torch.float32 if autocast else dtype
    p = {k: v.to(dtype) for k, v in sd.items()}
    x = x.to(dtype)
    D, P, Rn, heads = cfg["embed_dim"], cfg["patch_size"], cfg["num_register_tokens"], cfg["num_heads"]
    B, _, H, W = x.shape
    gh, gw = H // P, W // P
    with torch.no_grad(), torch.autocast(x.device.type, dtype=torch.bfloat16, enabled=autocast):
        t = F.conv2d(x, p["patch_embed.proj.weight"], p["patch_embed.proj.bias"], stride=P).flatten(2).transpose(1, 2)
        t = torch.cat([p["cls_token"].expand(B, -1, -1), t], 1)
        t = t + position_rows(p["pos_embed"], gh, gw, cfg["interpolate_antialias"], cfg["interpolate_offset"]).unsqueeze(0)
        if Rn:
            t = torch.cat([t[:, :1], p["register_tokens"].expand(B, -1, -1), t[:, 1:]], 1)
        T = t.shape[1]
        layers = []
        for i in range(cfg["depth"]):
            b = f"blocks.{i}."
            h = F.layer_norm(t, (D,), p[b + "norm1.weight"], p[b + "norm1.bias"], LN_EPS)
            q, k, v = F.linear(h, p[b + "attn.qkv.weight"], p[b + "attn.qkv.bias"]).reshape(B, T, 3, heads, D // heads).permute(2, 0, 3, 1, 4)
            a = torch.softmax((q * (D // heads) ** -0.5) @ k.transpose(-2, -1), -1) @ v
            a = F.linear(a.transpose(1, 2).reshape(B, T, D), p[b + "attn.proj.weight"], p[b + "attn.proj.bias"])
            t = t + p[b + "ls1.gamma"] * a
            h = F.layer_norm(t, (D,), p[b + "norm2.weight"], p[b + "norm2.bias"], LN_EPS)
            if cfg["ffn_layer"] == "mlp":
                u = F.linear(F.gelu(F.linear(h, p[b + "mlp.fc1.weight"], p[b + "mlp.fc1.bias"])), p[b + "mlp.fc2.weight"], p[b + "mlp.fc2.bias"])
            else:
                x1, x2 = F.linear(h, p[b + "mlp.w12.weight"], p[b + "mlp.w12.bias"]).chunk(2, -1)
                u = F.linear(F.silu(x1) * x2, p[b + "mlp.w3.weight"], p[b + "mlp.w3.bias"])
            t = t + p[b + "ls2.gamma"] * u
            layers.append(t.float() if autocast else t)
        n = F.layer_norm(t, (D,), p["norm.weight"], p["norm.bias"], LN_EPS)
    return {"x_norm_clstoken": n[:, 0], "x_norm_regtokens": n[:, 1:1 + Rn], "x_norm_patchtokens": n[:, 1 + Rn:], "x_prenorm": t, "layers": layers,
            "norm": lambda s: F.layer_norm(s, (D,), p["norm.weight"], p["norm.bias"], LN_EPS)}


def rel_max(a, ref):
    """max |a - ref| / max |ref| in float64: the distance the fixture stores and the tests bound."""
    ref = ref.double()
    return float((a.double().cpu() - ref.cpu()).abs().max() / ref.abs().max())


def load_golden():
    return np.load(GOLDEN)
