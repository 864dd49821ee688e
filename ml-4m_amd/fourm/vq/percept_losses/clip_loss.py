"""CLIP perceptual loss of the RGB tokenizer recipe on the HIP engine (upstream fourm/vq/percept_losses/timm_perceptual_loss.py:63-111 with
``percept_loss_type: vit_base_patch16_clip_224.openai``, ``percept_loss_blocks: blocks.2-blocks.5-blocks.8-blocks.11`` and
``percept_loss_distance: cosine``): the residual stream of a FROZEN CLIP vision tower after some blocks, for the reconstruction and for the
image, compared token by token.  The gradient flows through the tower back to the reconstructed pixels; the tower gets none.

    targets -> VisionTransformer.features (no state kept)  -> tap rows (copies)
    preds   -> VisionTransformer.features (state kept)     -> tap rows
    per tap: fm_feat_distance  -> loss (B,) +=, d(loss[b]) / d(tap rows of preds)
    backward: VisionTransformer.features_backward - fm_tap_add scales sample b's rows by the incoming d / d(loss[b]) and adds them to the
    stream gradient in front of the block below the tap; the blocks' backward with every dW skipped; fm_clip_embed_ln_bwd; the patch
    projection transposed; fm_vq_unpatchify.

Not here: fetching or converting timm checkpoints (build the tower from an OpenAI CLIP state dict: ``fourm.utils.clip.model.build_visual``),
DINOv2 or other feature networks, a trainable tower (LPIPS: lpips_loss.py).  Images of another size than the tower's are refused here;
``fourm.vq.training.perceptual_loss`` resizes them in front of this module (fm_resize_bilinear_fwd / _bwd with this module's affine folded in)."""
import torch
from torch import nn

from fourm.utils.clip.model import VisionTransformer, _engine, affine_fp32

OPENAI_CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
OPENAI_CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


class _PerceptStep(torch.autograd.Function):
    """Bridges the hand-written backward into autograd: ``preds`` is the only differentiable input."""

    @staticmethod
    def forward(ctx, preds, module, targets, fold):
        loss, saved = module._run(preds, targets, fold, save=True)
        ctx.module, ctx.saved, ctx.dtype = module, saved, preds.dtype
        return loss

    @staticmethod
    def backward(ctx, g_loss):
        saved, ctx.saved = ctx.saved, None
        d = ctx.module.visual.features_backward(saved["tower"], saved["d_taps"], g_loss.float().contiguous())
        return d.to(ctx.dtype), None, None, None


class ClipPerceptualLoss(nn.Module):
    """forward(preds, targets, preprocess_inputs=False) -> (B,) fp32: per tap ``1 - cosine_similarity(fp, ft, -1).mean(-1)`` ('cosine' | 'cos')
    or ``l1_loss(normalize(fp), normalize(ft), 'none').sum(-1).mean(-1)`` ('l1' | 'mae'), summed over the taps and divided by the batch
    size (upstream's own division; the trainer takes ``.mean()`` afterwards).

    visual: a ``fourm.utils.clip.model.VisionTransformer`` (``build_visual(state_dict)``, ``VisionTransformer.from_upstream(module)``); it is
    frozen and put in eval mode here.  Its ``compute_precision`` selects bf16 (default) or fp32 arithmetic.
    feature_ids: hyphen-separated string or list of ``blocks.<i>``: the residual stream after block i, every token, class token included
    (what torchvision's feature extractor returns for timm's ``blocks.i``).
    ``targets`` never receives a gradient; ``preds`` does when it requires one and gradients are enabled.  The state of that pass lives in
    the tower's engine: one forward may be awaiting its backward at a time."""

    def __init__(self, visual, feature_ids="blocks.2-blocks.5-blocks.8-blocks.11", feature_loss="cosine", mean=OPENAI_CLIP_MEAN, std=OPENAI_CLIP_STD):
        super().__init__()
        if not isinstance(visual, VisionTransformer):
            raise TypeError("visual: a fourm.utils.clip.model.VisionTransformer (build_visual(state_dict) or VisionTransformer.from_upstream(module))")
        ids = feature_ids.split("-") if isinstance(feature_ids, str) else list(feature_ids)
        layers = len(visual.blocks)
        taps = []
        for name in ids:
            head, _, idx = str(name).partition(".")
            if head != "blocks" or not idx.isdigit() or int(idx) >= layers:
                raise ValueError(f"feature id {name!r}: 'blocks.<i>' with i in range({layers}) expected (the residual stream after block i)")
            if int(idx) not in taps:
                taps.append(int(idx))
        if not taps:
            raise ValueError("feature_ids names no feature")
        if feature_loss not in ("cosine", "cos", "l1", "mae"):
            raise ValueError(f"Unknown feature loss: {feature_loss}")
        if len(mean) != 3 or len(std) != 3:
            raise ValueError("mean and std: one value per RGB channel")
        self.feature_ids, self.feature_loss, self.taps = [f"blocks.{i}" for i in taps], feature_loss, taps
        self.visual = visual.requires_grad_(False).eval()
        # [-1, 1] -> [0, 1] -> (v - mean) / std as ONE affine per channel: v = (x + 1) / 2
        self.register_buffer("_scale", torch.tensor([0.5 / s for s in std], dtype=torch.float32), persistent=False)
        self.register_buffer("_shift", torch.tensor([(0.5 - m) / s for m, s in zip(mean, std)], dtype=torch.float32), persistent=False)

    def train(self, mode: bool = True):
        """The tower stays in eval mode whatever the trainer sets on the modules around it."""
        super().train(mode)
        self.visual.eval()
        return self

    def _check_size(self, x):
        res = self.visual.input_resolution
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"expected images (B, 3, H, W), got {tuple(x.shape)}")
        if tuple(x.shape[-2:]) != (res, res):
            raise NotImplementedError(f"images of {x.shape[-2]}x{x.shape[-1]}: the tower takes {res}x{res} and no antialiased resize (or its "
                                      "adjoint) is built - resize before the loss")

    def percept_transform(self, x):
        """Upstream's transform for inputs in [-1, 1]: Normalize((-1, -1, -1), (2, 2, 2)), Normalize(mean, std) and the Resize, which is the
        identity at the tower's input size (any other size is refused).  One differentiable affine per channel, rounded once to fp32."""
        self._check_size(x)
        return affine_fp32(x, self._scale.to(x.device), self._shift.to(x.device))

    def forward(self, preds: torch.Tensor, targets: torch.Tensor, preprocess_inputs=False) -> torch.Tensor:
        self._check_size(preds)
        if preds.shape != targets.shape:
            raise ValueError(f"preds {tuple(preds.shape)} and targets {tuple(targets.shape)} differ in shape")
        if preds.requires_grad and torch.is_grad_enabled():
            return _PerceptStep.apply(preds, self, targets.detach(), bool(preprocess_inputs))
        return self._run(preds.detach(), targets.detach(), bool(preprocess_inputs), save=False)[0]

    def _run(self, preds, targets, fold, save):
        from fourm.hip import _lib as L
        from fourm.hip import ops
        vis = self.visual
        scale, shift = (self._scale, self._shift) if fold else (None, None)
        if fold and self._scale.device != preds.device:
            raise RuntimeError(f"input on {preds.device}, loss module on {self._scale.device}")
        with torch.no_grad():
            ft, _ = vis.features(targets, self.taps, False, scale, shift)
            fp, tower = vis.features(preds, self.taps, save, scale, shift)
            ws = _engine(vis).ws
            B = preds.shape[0]
            T = ft[self.taps[0]].shape[0] // B
            mode = L.FEAT_COSINE if self.feature_loss in ("cosine", "cos") else L.FEAT_L1
            loss = torch.zeros(B, dtype=torch.float32, device=preds.device)
            d_taps = {}
            for i in self.taps:
                d = ws.get(f"percept.dtap{i}" if save else "percept.dtap", (B * T, vis.width), torch.float32)
                ops.feat_distance(fp[i], ft[i], B, T, mode, loss, d)
                d_taps[i] = d
        return loss, (dict(tower=tower, d_taps=d_taps) if save else None)
