"""The tokenizer training objective on the HIP engine: what upstream's tokenizer trainers compute per iteration around ``VQVAE.forward`` /
backward and the perceptual losses (``fourm.vq.percept_losses``), as a library a trainer can sit on.

    compute_reconst_loss     run_training_vqvae.py:961-1003, the seven ``loss_fn`` modes; differentiable in ``model_output`` (fm_reconst_loss)
    mask_out_samples         run_training_vqvae.py:857-878 (fm_mask_out_samples)
    ModelEma                 fourm/utils/timm/model_ema.py:39-81; ``update`` is one launch over a device job list (fm_ema_update)
    diffusion_training_pair  the noised input and the regression target of a DiVAE step, run_training_divae.py:966-986 (fm_diffusion_pair)
    resize_images            F.interpolate at a given size, bilinear (optionally antialiased, optionally with a per-channel affine in the same
                             launch) and nearest; differentiable (fourm.vq.resize: fm_resize_bilinear_fwd / _bwd, fm_resize_nearest)
    prepare_inputs           run_training_vqvae.py:881-958 for the domains that need no feature network: the per-step resize and the masking
    perceptual_loss          run_training_vqvae.py:1146-1148: the perceptual term at any resolution (the CLIP loss's antialiased Resize and its
                             normalisation as one launch per tensor)

``fourm.vq.vq_utils.compute_codebook_usage`` (fm_token_usage) lives in upstream's module of that name.  Everything is fp32; the kernels are
csrc/train_objective.hip and csrc/resize.hip.  Tensors on the CPU raise RuntimeError (there is no CPU path), except where a function says
otherwise.

Not here: the trainer scripts themselves, their data loaders, feature extractors (CLIP / DINOv2 / ImageBind targets computed on the fly) and the
Inception metrics of evaluation."""
from collections import OrderedDict
from copy import deepcopy
from typing import Dict, Optional, Tuple, Union

import torch

from fourm.vq.resize import resize_images

LOSS_FNS = ("mse", "l1", "smooth_l1", "cross_entropy", "binary_cross_entropy", "cosine", "cosine_1d")
FEAT_MODALITIES = ['CLIP-B16', 'CLIP-L14', 'DINOv2-B14', 'DINOv2-B14-global', 'DINOv2-G14', 'DINOv2-G14-global', 'ImageBind-H14', 'ImageBind-H14-global']


def _on_gpu(what, *tensors):
    if not all(t.is_cuda for t in tensors):
        raise RuntimeError(f"{what} runs on the HIP kernels only (tensors on an MI355X; there is no CPU path)")


# ---- reconstruction loss ------------------------------------------------------------------------------------------------------------------
class _ReconstLoss(torch.autograd.Function):
    """One pass writes the loss and d loss / d model_output; the backward scales that gradient by the incoming scalar on the device
    (fm_scale_f32 leaves the buffer alone when the scalar is exactly 1), in place: one backward per forward."""

    @staticmethod
    def forward(ctx, x, target, mode):
        from fourm.hip import ops
        xc = x.detach().contiguous()
        grad = torch.empty_like(xc) if ctx.needs_input_grad[0] else None
        loss = ops.reconst_loss(xc, target, mode, grad)
        ctx.grad, ctx.shape = grad, x.shape
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        from fourm.hip import ops
        grad, ctx.grad = ctx.grad, None
        if grad is None:
            raise RuntimeError("compute_reconst_loss keeps its gradient for one backward (it is scaled in place): retain_graph is not supported")
        ops.scale_f32(grad, g.detach().reshape(1).float().to(grad.device))
        return grad.view(ctx.shape), None, None


def compute_reconst_loss(model_output: torch.Tensor, images: torch.Tensor, loss_fn: str) -> torch.Tensor:
    """Reconstruction loss of the tokenizer trainers, upstream's name and signature: a 0-dim fp32 tensor, differentiable in ``model_output``.

    ``loss_fn``: 'mse', 'l1', 'smooth_l1' (beta 1) - mean over all elements; 'cross_entropy' - ``model_output`` (B, K, H, W) scores against
    int64 class indices (B, H, W), ignore_index -100; 'binary_cross_entropy' - upstream's formulation (a softmax over the 2 C probabilities
    [sigmoid(x), 1 - sigmoid(x)] against [t, 1 - t]); 'cosine' - 1 - mean cosine similarity along H W per (b, c); 'cosine_1d' - along the
    channels per pixel.  Inputs of another floating dtype are converted to fp32 first.  The target gets no gradient (NotImplementedError if it
    requires one); class probabilities as a 'cross_entropy' target are not built."""
    from fourm.hip import _lib as L
    if loss_fn not in LOSS_FNS:
        raise ValueError(f'Unknown loss function {loss_fn}')
    if images.requires_grad:
        raise NotImplementedError("compute_reconst_loss: the target gets no gradient here (detach it)")
    _on_gpu("compute_reconst_loss", model_output, images)
    mode = {"mse": L.LOSS_MSE, "l1": L.LOSS_L1, "smooth_l1": L.LOSS_SMOOTH_L1, "cross_entropy": L.LOSS_CE_INDEX, "binary_cross_entropy": L.LOSS_BCE,
            "cosine": L.LOSS_COSINE, "cosine_1d": L.LOSS_COSINE_1D}[loss_fn]
    if mode == L.LOSS_CE_INDEX:
        if images.is_floating_point():
            raise NotImplementedError("compute_reconst_loss: 'cross_entropy' takes int64 class indices (B, H, W); class probabilities are not built")
        if model_output.dim() < 2 or images.shape != model_output.shape[:1] + model_output.shape[2:]:
            raise ValueError(f"'cross_entropy': scores {tuple(model_output.shape)} need class indices of shape (B, H, W), got {tuple(images.shape)}")
        target = images.to(torch.int64).contiguous()
    else:
        if images.shape != model_output.shape:
            raise ValueError(f"model_output {tuple(model_output.shape)} and images {tuple(images.shape)} differ in shape")
        target = images.float().contiguous()
    x = model_output.float()
    if mode <= L.LOSS_SMOOTH_L1:
        if x.dim() != 4:
            x = x.reshape(1, 1, 1, -1)                              # (element-wise: the mean over everything, whatever the shape)
    elif x.dim() < 3:
        raise ValueError(f"{loss_fn!r} expects (B, C, H, W), got {tuple(model_output.shape)}")
    return _ReconstLoss.apply(x, target, mode)


# ---- invalid-region masking -----------------------------------------------------------------------------------------------------------------
def mask_out_samples(clean_inputs: torch.Tensor, mask_valid: Optional[torch.Tensor] = None, mask_value: Optional[float] = None) -> torch.Tensor:
    """Overwrite the invalid positions (``mask_valid`` (B, 1, H, W) False) of ``clean_inputs`` (B, C, H, W) with ``mask_value`` IN PLACE, as
    upstream's indexing assignment does, and return a new (B, C + 1, H, W) tensor whose last channel is the mask as -1 / 1.  One launch.
    With ``mask_valid`` or ``mask_value`` None the input is returned untouched."""
    if mask_valid is None or mask_value is None:
        return clean_inputs
    from fourm.hip import ops
    _on_gpu("mask_out_samples", clean_inputs)
    if clean_inputs.dtype != torch.float32 or clean_inputs.dim() != 4:
        raise TypeError(f"mask_out_samples: fp32 images (B, C, H, W) expected, got {clean_inputs.dtype} {tuple(clean_inputs.shape)}")
    B, C, H, W = clean_inputs.shape
    valid = mask_valid.to(clean_inputs.device, non_blocking=True)
    if valid.shape != (B, 1, H, W):
        raise ValueError(f"mask_valid {tuple(valid.shape)}: expected {(B, 1, H, W)}")
    valid = valid.to(torch.bool).contiguous().view(torch.uint8)
    work = clean_inputs if clean_inputs.is_contiguous() else clean_inputs.contiguous()
    out = torch.empty(B, C + 1, H, W, dtype=torch.float32, device=clean_inputs.device)
    with torch.no_grad():
        ops.mask_out_samples(work.detach(), valid, mask_value, out)
        if work is not clean_inputs:
            clean_inputs.copy_(work)
    return out


# ---- per-step input preparation -----------------------------------------------------------------------------------------------------------------
def prepare_inputs(x: Dict[str, torch.Tensor], domain: str, feature_extractor: Optional[torch.nn.Module], device: Union[torch.device, str],
                   image_size: Optional[int] = None, mask_value: Optional[float] = None) -> torch.Tensor:
    """Upstream's ``prepare_inputs`` for the domains that need no feature network: take the domain's entry of the batch dict to ``device``,
    resize it to ``image_size`` (an int or (H, W); None: as it is) and mask out the invalid regions.

    Image-like domains: bilinear, align_corners=False (resize_images).  ``semseg*``: nearest on the integer class map (B, H, W), dtype kept.
    ``sam_mask*``: ``x[domain]['instance']`` (B, N, H, W) flattened to (B N, 1, H, W), the instances with ``x[domain]['valid']`` selected; no
    resize.  ``human_poses``: no resize, two trailing axes added.  Then ``mask_out_samples(images, x.get('mask_valid'), mask_value)``.
    A domain of ``FEAT_MODALITIES`` reads ``x['rgb']``; with a ``feature_extractor`` it raises NotImplementedError: feature networks are out
    of scope here (extract the features before, or pass None to get the resized RGB)."""
    if domain in FEAT_MODALITIES:
        if feature_extractor is not None:
            raise NotImplementedError(f"prepare_inputs: domain {domain!r} with a feature_extractor - feature networks (CLIP / DINOv2 / ImageBind targets "
                                      "computed on the fly) are out of scope of this package's trainer pieces")
        images = x['rgb'].to(device, non_blocking=True)
    elif 'sam_mask' in domain:
        images, valid = x[domain]['instance'], x[domain]['valid']
        images = images.flatten(end_dim=1).unsqueeze(1)
        images = images[valid.flatten().to(images.device)].to(device, non_blocking=True)
    else:
        images = x[domain].to(device, non_blocking=True)
    if image_size is not None and 'human_poses' not in domain and 'sam_mask' not in domain:
        if 'semseg' in domain:
            if images.is_floating_point():
                images = resize_images(images.float().unsqueeze(1), image_size, mode='nearest').to(images.dtype).squeeze(1)
            else:
                images = resize_images(images.to(torch.int64), image_size, mode='nearest').to(images.dtype)
        else:
            images = resize_images(images, image_size, mode='bilinear')
    if 'human_poses' in domain:
        images = images.unsqueeze(2).unsqueeze(2)
    return mask_out_samples(images, x.get('mask_valid', None), mask_value=mask_value)


# ---- perceptual term ----------------------------------------------------------------------------------------------------------------------------
def perceptual_loss(loss_fn, model_output: torch.Tensor, images: torch.Tensor) -> torch.Tensor:
    """``loss_fn(transform(model_output), transform(images)).mean()`` with the loss's own ``percept_transform`` - the perceptual term of
    upstream's training and validation loops - at any image resolution.

    ClipPerceptualLoss: at the tower's resolution the transform is its ``percept_transform``.  At any other, upstream's Normalize, Normalize,
    Resize(res, bilinear, antialias) becomes ONE launch per tensor: the antialiased resize with the loss's per-channel affine folded in (the
    weights of a window sum to 1, so R(a x + b) = a R(x) + b: upstream's order up to rounding), and the gradient comes back through the
    adjoint kernel.  LpipsPerceptualLoss: the identity, as upstream.  A wrapped loss (``.module``) is unwrapped for the transform only."""
    from fourm.vq.percept_losses import ClipPerceptualLoss, LpipsPerceptualLoss
    inner = loss_fn.module if hasattr(loss_fn, "module") else loss_fn
    if isinstance(inner, ClipPerceptualLoss):
        _on_gpu("perceptual_loss", model_output, images)
        res = inner.visual.input_resolution
        if model_output.dim() != 4 or model_output.shape != images.shape:
            raise ValueError(f"model_output {tuple(model_output.shape)} and images {tuple(images.shape)}: two (B, 3, H, W) batches of one shape expected")
        if tuple(model_output.shape[-2:]) == (res, res):
            transform = inner.percept_transform
        else:
            def transform(t):
                return resize_images(t.float(), res, mode="bilinear", antialias=True, scale=inner._scale, shift=inner._shift)
        return loss_fn(transform(model_output), transform(images), preprocess_inputs=False).mean()
    if isinstance(inner, LpipsPerceptualLoss):
        return loss_fn(model_output, images).mean()
    raise TypeError(f"perceptual_loss: a ClipPerceptualLoss or LpipsPerceptualLoss expected, got {type(inner).__name__}")


# ---- weight EMA -----------------------------------------------------------------------------------------------------------------------------
def _copy_model(model):
    """deepcopy of the model.  The engines (scratch, cached weight images) stay behind by their own ``__deepcopy__``
    (fourm/vq/engine.py); the HIP stream pools of fourm.vq.tokenize_sub_batches / decode_token_batches are left behind here: the copy
    builds its own of both."""
    memo = {}
    for m in (model.modules() if isinstance(model, torch.nn.Module) else []):
        for a in ("_tok_streams", "_dec_streams"):
            if m.__dict__.get(a) is not None:
                memo[id(m.__dict__[a])] = None
    return deepcopy(model, memo)


class ModelEma:
    """Exponential moving average of everything in the model's state_dict, parameters and buffers (upstream's ``ModelEma``, from timm:
    constructor, ``.ema`` / ``.decay`` / ``.device`` / ``.ema_has_module``, ``update(model)``).

    ``update`` runs every fp32 entry that lives on the model's GPU in ONE launch over a device job list - (ema pointer, model pointer, element
    count, first chunk), built at the first update and rebuilt only when a data pointer changes - with upstream's arithmetic, each operation
    rounded separately: ema * float(decay) + float(1 - decay) * model, bit-identical to upstream's three torch kernels per entry.  Entries of
    another dtype (integer buffers) and an EMA kept on another device (``device='cpu'``) take upstream's torch expression.  The engines' cached
    weight images follow through the weight epoch."""

    def __init__(self, model, decay=0.9999, device='', resume=''):
        self.ema = _copy_model(model)
        self.ema.eval()
        self.decay = decay
        self.device = device          # perform the EMA on another device than the model's if set
        if device:
            self.ema.to(device=device)
        self.ema_has_module = hasattr(self.ema, 'module')
        if resume:
            self._load_checkpoint(resume)
        for p in self.ema.parameters():
            p.requires_grad_(False)
        self._jobs = None             # (stamp, device table, n_jobs, chunks, the tensors the table points into)

    def _load_checkpoint(self, checkpoint_path):
        checkpoint = torch.load(checkpoint_path, map_location='cpu', weights_only=False)
        assert isinstance(checkpoint, dict)
        if 'state_dict_ema' in checkpoint:
            new_state_dict = OrderedDict()
            for k, v in checkpoint['state_dict_ema'].items():
                # the EMA model may be wrapped (DataParallel) and need the module prefix
                new_state_dict['module.' + k if self.ema_has_module and not k.startswith('module') else k] = v
            self.ema.load_state_dict(new_state_dict)
            print("Loaded state_dict_ema")
        else:
            print("Failed to find state_dict_ema, starting from loaded model weights")

    def update(self, model):
        needs_module = hasattr(model, 'module') and not self.ema_has_module
        with torch.no_grad():
            msd = model.state_dict()
            pairs = []
            for k, ema_v in self.ema.state_dict().items():
                model_v = msd['module.' + k if needs_module else k].detach()
                if (ema_v.is_cuda and model_v.device == ema_v.device and ema_v.dtype == model_v.dtype == torch.float32 and ema_v.shape == model_v.shape
                        and ema_v.is_contiguous() and model_v.is_contiguous() and ema_v.numel() > 0):
                    pairs.append((ema_v, model_v))
                    continue
                if self.device:
                    model_v = model_v.to(device=self.device)
                ema_v.copy_(ema_v * self.decay + (1. - self.decay) * model_v)
            if pairs:
                self._launch(pairs)

    def _launch(self, pairs):
        from fourm.hip import engine as hip_engine
        from fourm.hip import ops
        device = pairs[0][0].device
        stamp = (device, tuple((e.data_ptr(), m.data_ptr(), e.numel()) for e, m in pairs))
        if self._jobs is None or self._jobs[0] != stamp:
            table, chunks = ops.ema_jobs_table(pairs, device)
            self._jobs = (stamp, table, len(pairs), chunks, pairs)
        _, table, n_jobs, chunks, _ = self._jobs
        with torch.cuda.device(device):
            ops.ema_update(table, n_jobs, chunks, self.decay)
        hip_engine.bump_weight_epoch()          # (the kernel writes behind torch's version counters)


# ---- DiVAE training pair ----------------------------------------------------------------------------------------------------------------------
def _schedule_tables(scheduler, device):
    """sqrt(alpha_bar_t) and sqrt(1 - alpha_bar_t) for every training timestep on ``device``, by the scheduler's own expression."""
    ac = scheduler.alphas_cumprod
    cache = scheduler.__dict__.setdefault("_training_tables", {})
    hit = cache.get(device)
    stamp = (id(ac), ac._version, ac.numel())
    if hit is None or hit[0] != stamp:
        T = ac.numel()
        sa, ss = scheduler.get_alpha_sigma_sqrts(torch.arange(T, device=device), device, torch.float32, (T,))
        hit = cache[device] = (stamp, sa.contiguous(), ss.contiguous())
    return hit[1], hit[2]


def diffusion_training_pair(scheduler, clean: torch.Tensor, noise: torch.Tensor, timesteps: torch.Tensor, prediction_type: str) -> Tuple[torch.Tensor, torch.Tensor]:
    """(noisy, target) of one diffusion training step: ``noisy = scheduler.add_noise(clean, noise, timesteps)`` and the regression target of
    ``prediction_type`` - 'sample': ``clean`` itself; 'epsilon' and 'v_prediction-epsilon_loss' (whose model output the trainer converts with
    ``get_noise``): ``noise`` itself; 'v_prediction': ``scheduler.get_velocity(clean, noise, timesteps)``.  One launch reads ``clean`` and
    ``noise`` once, the per-sample coefficients are gathered on the device from the scheduler's tables: no host synchronisation.  Bit-identical
    to the scheduler's own methods."""
    from fourm.hip import ops
    if prediction_type not in ("sample", "epsilon", "v_prediction", "v_prediction-epsilon_loss"):
        raise ValueError(f"prediction_type given as {prediction_type} must be one of `epsilon`, `sample`, `v_prediction` or `v_prediction-epsilon_loss`")
    _on_gpu("diffusion_training_pair", clean, noise)
    if clean.dtype != torch.float32 or noise.dtype != torch.float32:
        raise TypeError(f"diffusion_training_pair: fp32 images and noise expected, got {clean.dtype} / {noise.dtype}")
    if clean.shape != noise.shape or timesteps.numel() != clean.shape[0]:
        raise ValueError(f"clean {tuple(clean.shape)}, noise {tuple(noise.shape)}, timesteps {tuple(timesteps.shape)}: one timestep per sample expected")
    with torch.no_grad():
        sa, ss = _schedule_tables(scheduler, clean.device)
        t = timesteps.detach().to(device=clean.device, dtype=torch.int64, non_blocking=True).reshape(-1).contiguous()
        c, z = clean.detach().contiguous(), noise.detach().contiguous()
        noisy = torch.empty_like(c)
        velocity = torch.empty_like(c) if prediction_type == "v_prediction" else None
        with torch.cuda.device(clean.device):
            ops.diffusion_pair(c, z, t, sa, ss, noisy, velocity)
    target = clean if prediction_type == "sample" else velocity if prediction_type == "v_prediction" else noise
    return noisy, target
