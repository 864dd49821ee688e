"""Perceptual losses of tokenizer training.  ``ClipPerceptualLoss`` (clip_loss.py) and ``LpipsPerceptualLoss`` (lpips_loss.py) are this
package's: a frozen CLIP vision tower and the frozen VGG16 of LPIPS on the HIP engine, forward and backward.  Everything else upstream's
package of the same name offers (``timm_perceptual_loss``, and upstream's own eager ``lpips`` module) resolves through an upstream checkout
(fourm/_upstream.py)."""
from fourm import _upstream as _up

_up.extend_path(__name__, __path__)          # first: fourm.vq.percept_losses.lpips falls through to upstream's file
from .clip_loss import OPENAI_CLIP_MEAN, OPENAI_CLIP_STD, ClipPerceptualLoss
from .lpips_alex import LpipsAlex          # the AlexNet tower of the LPIPS validation METRIC (fourm.vq.metrics), forward only
from .lpips_loss import LpipsPerceptualLoss

__all__ = ["ClipPerceptualLoss", "OPENAI_CLIP_MEAN", "OPENAI_CLIP_STD", "LpipsAlex", "LpipsPerceptualLoss"]
