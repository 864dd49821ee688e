"""Shared pieces of the CLIP perceptual-loss tests: ``vit_taps`` - the block loop of tests/clip_util.py::vit_forward returning the residual
streams after named blocks - and ``percept_ref``, lines 89-109 of upstream's fourm/vq/percept_losses/timm_perceptual_loss.py restated on those
streams.  Both run in any float type and under autograd; float64 autograd through them is the yardstick of the GPU tests.
tests/test_clip_percept_cpu.py pins ``vit_taps`` to the pinned restatement ``vit_forward``."""
import torch
import torch.nn.functional as F

from tests.clip_util import LN_EPS, position_table


def vit_taps(sd, x, taps, dtype=torch.float64):
    """{i: residual stream (B, T, D) after block i, class token included} for i in ``taps``; the arithmetic of clip_util.vit_forward line by line."""
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
    out, i = {}, 0
    while f"transformer.resblocks.{i}.ln_1.weight" in p and i <= max(taps):
        b = f"transformer.resblocks.{i}."
        h = ln(t, b + "ln_1")
        q, k, v = (h @ p[b + "attn.in_proj_weight"].t() + p[b + "attn.in_proj_bias"]).reshape(B, T, 3, heads, 64).permute(2, 0, 3, 1, 4)
        a = torch.softmax(q @ k.transpose(-1, -2) * 64 ** -0.5, -1) @ v
        t = t + a.permute(0, 2, 1, 3).reshape(B, T, D) @ p[b + "attn.out_proj.weight"].t() + p[b + "attn.out_proj.bias"]
        u = ln(t, b + "ln_2") @ p[b + "mlp.c_fc.weight"].t() + p[b + "mlp.c_fc.bias"]
        u = u * torch.sigmoid(1.702 * u)
        t = t + u @ p[b + "mlp.c_proj.weight"].t() + p[b + "mlp.c_proj.bias"]
        if i in taps:
            out[i] = t
        i += 1
    assert sorted(out) == sorted(set(taps)), (sorted(out), taps)
    return out


def feature_loss(fp, ft, mode):
    """One tap of upstream's loop (timm_perceptual_loss.py:100-105): (B, T, D) x 2 -> (B,)."""
    if mode in ("l1", "mae"):
        return F.l1_loss(F.normalize(fp, dim=-1), F.normalize(ft, dim=-1), reduction="none").sum(-1).mean(-1)
    assert mode in ("cosine", "cos"), mode
    return 1 - F.cosine_similarity(fp, ft, dim=-1).mean(dim=-1)


def percept_ref(sd, preds, targets, taps, mode, dtype=torch.float64):
    """Upstream's forward without preprocessing on the streams after ``taps``: (B,) in ``dtype``, differentiable with respect to ``preds``."""
    fp, ft = vit_taps(sd, preds, taps, dtype), vit_taps(sd, targets, taps, dtype)
    loss = 0
    for i in taps:
        loss = loss + feature_loss(fp[i], ft[i], mode)
    return loss / preds.shape[0]
