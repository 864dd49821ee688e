"""Float64 yardstick for the diffusion detokenizer: TEST INFRASTRUCTURE.

oracle/divae_oracle.py casts to fp32 at several places (timestep embedding, GroupNorm input, softmax, thresholding, the schedule tables), so it
cannot serve as the reference an fp32 kernel is measured against.  This file restates the same arithmetic - one UNet evaluation
(unet_forward) and the sampling loop (sample_loop) with its scheduler steps and schedule tables - with the working dtype as a parameter:
every tensor, table and constant is created in ``dtype`` and nothing is cast on the way.  ``dtype=torch.float32`` reproduces the oracle and
upstream's fixture (pinned in tests/test_divae_fp32_cpu.py); ``dtype=torch.float64`` is the yardstick of tests/test_divae_fp32_gpu.py.
The plan of the module tree, the configuration classes and the timestep spacing (integers) are the oracle's own."""
import math
from typing import List, Optional

import torch
import torch.nn.functional as F

from oracle import divae_oracle as DO


def cast_state(P, dtype):
    return {k: v.to(dtype) for k, v in P.items()}


def timestep_embedding(t, dim, dtype, max_period=10000.0):
    half = dim // 2
    freqs = torch.exp(-math.log(max_period) * torch.arange(half, dtype=dtype) / half)
    args = t[:, None].to(dtype) * freqs[None]
    emb = torch.cat([torch.cos(args), torch.sin(args)], dim=-1)
    if dim % 2:
        emb = torch.cat([emb, torch.zeros_like(emb[:, :1])], dim=-1)
    return emb


def _gn(P, k, x):
    return F.group_norm(x, 32, P[k + ".weight"], P[k + ".bias"], 1e-5)


def _res(P, k, x, emb, ci, co):
    h = F.conv2d(F.silu(_gn(P, k + ".in_layers.0", x)), P[k + ".in_layers.2.weight"], P[k + ".in_layers.2.bias"], padding=1)
    e = F.linear(F.silu(emb), P[k + ".emb_layers.1.weight"], P[k + ".emb_layers.1.bias"])
    h = h + e[:, :, None, None]
    h = F.conv2d(F.silu(_gn(P, k + ".out_layers.0", h)), P[k + ".out_layers.3.weight"], P[k + ".out_layers.3.bias"], padding=1)
    if ci != co:
        x = F.conv2d(x, P[k + ".skip_connection.weight"], P[k + ".skip_connection.bias"])
    return x + h


def _attn(P, k, x, heads):
    b, c, hh, ww = x.shape
    xf = x.reshape(b, c, -1)
    qkv = F.conv1d(_gn(P, k + ".norm", xf), P[k + ".qkv.weight"], P[k + ".qkv.bias"])
    ch = c // heads
    q, kk, v = qkv.reshape(b * heads, ch * 3, -1).split(ch, dim=1)
    scale = 1 / math.sqrt(math.sqrt(ch))
    w = torch.softmax(torch.einsum("bct,bcs->bts", q * scale, kk * scale), dim=-1)
    a = torch.einsum("bts,bcs->bct", w, v).reshape(b, -1, hh * ww)
    h = F.conv1d(a, P[k + ".proj_out.weight"], P[k + ".proj_out.bias"])
    return (xf + h).reshape(b, c, hh, ww)


def _run(P, cfg, blk, h, emb):
    for item in blk:
        kind, key = item[0], item[1]
        if kind == "conv3":
            h = F.conv2d(h, P[key + ".weight"], P[key + ".bias"], padding=1)
        elif kind == "res":
            h = _res(P, key, h, emb, item[2], item[3])
        elif kind == "attn":
            h = _attn(P, key, h, cfg.num_heads)
        elif kind == "down":
            h = F.conv2d(h, P[key + ".op.weight"], P[key + ".op.bias"], stride=2, padding=1)
        elif kind == "up":
            h = F.conv2d(F.interpolate(h, scale_factor=2, mode="nearest"), P[key + ".conv.weight"], P[key + ".conv.bias"], padding=1)
    return h


def unet_forward(P, cfg, sample, timesteps, cond, cond_mask=None, dtype=torch.float64):
    """PatchedUNetCondCat.forward in ``dtype``; P must be cast_state(P, dtype)."""
    sample, cond = sample.to(dtype), cond.to(dtype)
    B, C, H, W = sample.shape
    p = cfg.patch_size
    nh, nw = H // p, W // p
    x = sample.reshape(B, C, nh, p, nw, p).permute(0, 1, 3, 5, 2, 4).reshape(B, C * p * p, nh, nw)
    if cond_mask is not None:
        cond = torch.where(cond_mask[:, None], torch.zeros((), dtype=dtype), cond)
    x = torch.cat([x, F.interpolate(cond, (nh, nw), mode="nearest")], dim=1)
    t = torch.as_tensor(timesteps)
    t = t.reshape(1) if t.ndim == 0 else t
    emb = timestep_embedding(t, cfg.model_channels, dtype)
    emb = F.linear(F.silu(F.linear(emb, P["time_embed.0.weight"], P["time_embed.0.bias"])), P["time_embed.2.weight"], P["time_embed.2.bias"])
    inp, mid, out, _ = DO.unet_plan(cfg)
    hs, h = [], x
    for blk in inp:
        h = _run(P, cfg, blk, h, emb)
        hs.append(h)
    h = _run(P, cfg, mid, h, emb)
    for blk in out:
        h = _run(P, cfg, blk, torch.cat([h, hs.pop()], dim=1), emb)
    y = F.conv2d(F.silu(_gn(P, "out.0", h)), P["out.2.weight"], P["out.2.bias"], padding=1)
    return y.reshape(B, cfg.out_channels, p, p, nh, nw).permute(0, 1, 4, 2, 5, 3).reshape(B, cfg.out_channels, H, W)


# ---- schedule tables and scheduler steps -------------------------------------------------------------------------------------------------
def alphas_cumprod(c, dtype):
    T = c.num_train_timesteps
    if c.beta_schedule == "linear":
        betas = torch.linspace(c.beta_start, c.beta_end, T, dtype=dtype)
    elif c.beta_schedule == "scaled_linear":
        betas = torch.linspace(c.beta_start ** 0.5, c.beta_end ** 0.5, T, dtype=dtype) ** 2
    elif c.beta_schedule == "squaredcos_cap_v2":
        ab = lambda s: math.cos((s + 0.008) / 1.008 * math.pi / 2) ** 2
        betas = torch.tensor([min(1 - ab((i + 1) / T) / ab(i / T), 0.999) for i in range(T)], dtype=dtype)
    else:
        raise NotImplementedError(c.beta_schedule)
    if c.zero_terminal_snr:
        abs_ = (1 - betas).cumprod(0).sqrt()
        a0, aT = abs_[0].clone(), abs_[-1].clone()
        abs_ = (abs_ - aT) * (a0 / (a0 - aT))
        ab2 = abs_ ** 2
        alphas = torch.cat([ab2[0:1], ab2[1:] / ab2[:-1]])
        betas = 1 - alphas
    return torch.cumprod(1.0 - betas, dim=0)


def threshold_sample(c, x0):
    B = x0.shape[0]
    flat = x0.reshape(B, -1)
    s = torch.quantile(flat.abs(), c.dynamic_thresholding_ratio, dim=1).clamp(min=1, max=c.sample_max_value)[:, None]
    return (torch.clamp(flat, -s, s) / s).reshape(x0.shape)


def _pred_x0_eps(c, a_t, model_output, sample):
    b_t = 1 - a_t
    if c.prediction_type == "epsilon":
        return (sample - b_t ** 0.5 * model_output) / a_t ** 0.5, model_output
    if c.prediction_type == "sample":
        return model_output, (sample - a_t ** 0.5 * model_output) / b_t ** 0.5
    if c.prediction_type == "v_prediction":
        return (a_t ** 0.5) * sample - (b_t ** 0.5) * model_output, (a_t ** 0.5) * model_output + (b_t ** 0.5) * sample
    raise ValueError(c.prediction_type)


def _clean(c, x0):
    if c.thresholding:
        return threshold_sample(c, x0)
    if c.clip_sample:
        return x0.clamp(-c.clip_sample_range, c.clip_sample_range)
    return x0


def ddim_step(c, ac, n_inference, model_output, t, sample, eta=0.0, noise=None):
    prev_t = t - c.num_train_timesteps // n_inference
    a_t = ac[t]
    a_prev = ac[prev_t] if prev_t >= 0 else torch.tensor(1.0, dtype=ac.dtype)
    x0, eps = _pred_x0_eps(c, a_t, model_output, sample)
    x0 = _clean(c, x0)
    variance = ((1 - a_prev) / (1 - a_t)) * (1 - a_t / a_prev)
    std = eta * variance ** 0.5
    prev = a_prev ** 0.5 * x0 + (1 - a_prev - std ** 2) ** 0.5 * eps
    if eta > 0:
        prev = prev + std * noise
    return prev, x0


def ddpm_step(c, ac, n_inference, model_output, t, sample, noise=None):
    prev_t = t - c.num_train_timesteps // n_inference
    a_t = ac[t]
    a_prev = ac[prev_t] if prev_t >= 0 else torch.tensor(1.0, dtype=ac.dtype)
    b_t, b_prev = 1 - a_t, 1 - a_prev
    cur_a = a_t / a_prev
    cur_b = 1 - cur_a
    x0, _ = _pred_x0_eps(c, a_t, model_output, sample)
    x0 = _clean(c, x0)
    prev = (a_prev ** 0.5 * cur_b) / b_t * x0 + cur_a ** 0.5 * b_prev / b_t * sample
    if t > 0:
        var = torch.clamp(b_prev / b_t * cur_b, min=1e-20)
        prev = prev + (var ** 0.5) * noise
    return prev, x0


def sample_loop(P, ucfg, scfg, cond, noise0, n_steps, mode="trailing", step_noise: Optional[List[torch.Tensor]] = None, dtype=torch.float64):
    """PipelineCond.__call__ with guidance scale 0 in ``dtype`` (P = cast_state(P, dtype)); the noise tensors are the caller's fp32 draws,
    widened.  Returns (image, [model outputs])."""
    ac = alphas_cumprod(scfg, dtype)
    ts = DO.inference_timesteps(scfg, n_steps, mode)
    image, outs = noise0.to(dtype), []
    for i, t in enumerate(ts):
        out = unet_forward(P, ucfg, image, int(t), cond, dtype=dtype)
        outs.append(out)
        if scfg.kind == "ddim":
            image, _ = ddim_step(scfg, ac, n_steps, out, int(t), image)
        else:
            image, _ = ddpm_step(scfg, ac, n_steps, out, int(t), image, None if step_noise is None else step_noise[i].to(dtype))
    return image, outs
