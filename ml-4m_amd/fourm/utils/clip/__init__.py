"""``fourm.utils.clip``: the vision tower (``model.VisionTransformer``, ``model.build_visual``), the text tower (``text.TextTransformer``,
``text.build_text``), the logits (``text.clip_logits``) and the CLIP score (``score.ClipScore``) run on the HIP engine; ``load``, ``tokenize``,
``available_models``, ``CLIP`` and ``ModifiedResNet`` are upstream's and resolve through an upstream checkout (fourm/_upstream.py)."""
from ... import _upstream
_upstream.extend_path(__name__, __path__)          # first: upstream's clip.py / simple_tokenizer.py are found next to this package's model.py
from .model import QuickGELU, VisionTransformer, build_visual
from .text import TextTransformer, build_text, clip_logits
from .score import ClipScore

__getattr__ = _upstream.fallthrough(__name__, is_package=True)
