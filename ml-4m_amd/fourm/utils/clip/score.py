"""CLIP score on the HIP engine: the number upstream's ``run_generation.py`` judges text-to-image generation by (:34, :678-700, :836-848, where
it comes from ``torchmetrics.multimodal.CLIPScore``), over this package's two towers.

    score(pair) = 100 * cos(image_features, text_features)        metric = max(mean of the scores of all pairs since reset, 0)

(the clamp is applied to the mean, not per pair).  That definition ("CLIP text tower and CLIP score") is the contract:
torchmetrics is not a dependency, and parity with it is not pinned.  ``ClipScore`` follows the ``update`` / ``compute`` / ``reset`` / ``.to``
pattern of ``fourm.vq.metrics``: the sum (float64) and the count (int64) live on the device, ``update`` does not synchronise with the host
beyond the text tower's id check, ``compute`` is where a number is asked for.  Not here: string prompts (tokenise with
``fourm.utils.clip.tokenize``) and image preprocessing (bicubic resize, centre crop): images arrive in CLIP's normalised space at the
tower's resolution."""
import torch

__all__ = ["ClipScore"]


def _is_text(x):
    return isinstance(x, str) or (isinstance(x, (list, tuple)) and any(isinstance(t, str) for t in x))


class ClipScore:
    def __init__(self, visual, text):
        """``visual``: a ``VisionTransformer`` (images -> (B, embed_dim)); ``text``: a ``TextTransformer`` (ids -> (B, embed_dim)); both on the
        GPU and frozen.  Either may be None when only ``update_features`` is used."""
        self.visual, self.text = visual, text
        self.sum = self.count = None

    def reset(self):
        if self.sum is not None:
            self.sum.zero_()
            self.count.zero_()

    def to(self, device):
        """Moves the accumulated state (the towers are the caller's)."""
        if self.sum is not None:
            self.sum, self.count = self.sum.to(device), self.count.to(device)
        return self

    def update(self, images: torch.Tensor, ids: torch.Tensor) -> torch.Tensor:
        """images (B, 3, res, res) fp32, already in CLIP's normalised space at the vision tower's resolution; ids (B, context_length) token ids.
        Returns the per-pair scores (B,) fp32."""
        if _is_text(ids) or _is_text(images):
            raise TypeError("ClipScore takes token ids, not strings: tokenise the prompts with fourm.utils.clip.tokenize first")
        if self.visual is None or self.text is None:
            raise RuntimeError("ClipScore.update needs both towers (update_features takes features)")
        with torch.no_grad():
            return self.update_features(self.visual(images), self.text(ids))

    def update_features(self, image_features: torch.Tensor, text_features: torch.Tensor) -> torch.Tensor:
        """image_features, text_features (B, E) fp32, pair b in row b of both.  Returns the per-pair scores (B,) fp32."""
        from fourm.hip import ops
        if _is_text(image_features) or _is_text(text_features):
            raise TypeError("ClipScore takes features or token ids, not strings: tokenise the prompts with fourm.utils.clip.tokenize first")
        if not (torch.is_tensor(image_features) and torch.is_tensor(text_features)) or image_features.dim() != 2 \
                or tuple(image_features.shape) != tuple(text_features.shape) or image_features.numel() == 0:
            raise ValueError("ClipScore: two (B, E) feature tensors of one shape expected")
        if image_features.dtype != torch.float32 or text_features.dtype != torch.float32:
            raise TypeError(f"ClipScore: fp32 features expected, got {image_features.dtype} / {text_features.dtype}")
        if not (image_features.is_cuda and text_features.is_cuda):
            raise RuntimeError("ClipScore runs on the HIP kernels only (tensors on an MI355X; there is no CPU path)")
        dev = image_features.device
        if self.sum is None:
            self.sum, self.count = torch.zeros(1, dtype=torch.float64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev)
        elif self.sum.device != dev:
            self.to(dev)
        with torch.no_grad(), torch.cuda.device(dev):
            img, txt = image_features.detach(), text_features.detach()
            img = img if img.stride(1) == 1 else img.contiguous()
            txt = txt if txt.stride(1) == 1 else txt.contiguous()
            score = torch.empty(img.shape[0], dtype=torch.float32, device=dev)
            ops.clip_pair_score(img, txt, score, self.sum, self.count)
        return score

    def compute(self) -> float:
        """max(sum / n, 0) over all pairs since ``reset`` as a Python float (nan when nothing was seen): the one host synchronisation."""
        if self.sum is None:
            return float("nan")
        mean = float((self.sum[0] / self.count[0].double()).item())
        return mean if mean != mean else max(mean, 0.0)
