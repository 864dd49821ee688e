"""Low-rank adaptation (LoRA, https://arxiv.org/abs/2106.09685) of a FourM model on the HIP engine.

The public names, signatures, defaults, initialisation and state-dict keys are those of upstream's ``fourm/models/lora_utils.py``
(``<name>.linear.weight``, ``<name>.lora_down.weight``, ``<name>.lora_up.weight``), so an upstream LoRA checkpoint loads with
``strict=True``.  The low-rank path itself runs in ``fm_lora_apply`` / ``fm_lora_grad`` (csrc/lora.hip), called by
``fourm.hip.engine`` right behind the base GEMM of a wrapped Linear; a wrapper forwards ``weight`` / ``bias`` to the Linear it
wraps, so the engine's reads of ``blk.attn.qkv.weight`` keep working.

Supported on the engine: the attention Linears (upstream's default ``ATTENTION_MODULES``).  The MLP ids are refused here: fc1 / fc3
run as one launch whose SwiGLU epilogue consumes the pre-activation, so there is no buffer a low-rank term could be added to.
"""
from typing import Iterator, Optional, Set, Tuple

import torch
import torch.nn as nn

SELF_ATTENTION_MODULES = {"Attention", "NormAttention"}
CROSS_ATTENTION_MODULES = {"CrossAttention", "NormCrossAttention"}
ATTENTION_MODULES = SELF_ATTENTION_MODULES | CROSS_ATTENTION_MODULES
MLP_MODULES = {"Mlp", "GatedMlp", "SwiGLUFFNFused"}
TRANSFORMER_MODULES = ATTENTION_MODULES | MLP_MODULES

MAX_LORA_WIDTH = 64          # rank * num_packed_linear the kernels hold on chip (fm_lora_apply / fm_lora_grad)
_MLP_REASON = ("LoRA on the MLP Linears is not implemented on the HIP engine: fc1 / fc3 run as one launch whose SwiGLU (GELU) epilogue "
               "consumes the pre-activation, so a low-rank term has no buffer to be added to; adapt the attention Linears ('attn')")
_IDS = {
    "selfattn": SELF_ATTENTION_MODULES, "selfattention": SELF_ATTENTION_MODULES, "self_attn": SELF_ATTENTION_MODULES,
    "self_attention": SELF_ATTENTION_MODULES,
    "crossattn": CROSS_ATTENTION_MODULES, "crossattention": CROSS_ATTENTION_MODULES, "cross_attn": CROSS_ATTENTION_MODULES,
    "cross_attention": CROSS_ATTENTION_MODULES,
    "attn": ATTENTION_MODULES, "attention": ATTENTION_MODULES,
}


def get_LoRA_module_names(id: str) -> Set[str]:
    """Class names of the modules whose Linears are adapted for ``id`` ('selfattn', 'crossattn', 'attn', ...)."""
    key = id.lower()
    if key in ("mlp", "all", "transformer"):
        raise NotImplementedError(f"LoRA module id {id!r}: {_MLP_REASON}")
    if key not in _IDS:
        raise ValueError(f"Unknown LoRA module id {id}.")
    return _IDS[key]


def packed_linears(name: str) -> int:
    """How many Linears a fused projection packs, from its attribute name: qkv -> 3, kv / qk / qv -> 2, anything else 1."""
    letters = sorted(name)
    if letters == sorted("qkv"):
        return 3
    if letters in (sorted("kv"), sorted("qk"), sorted("qv")):
        return 2
    return 1


class LoRAWrapper(nn.Module):
    """``y = linear(x) + scale * lora_up(lora_down(x))`` around an ``nn.Linear``.

    Args:
        linear: the Linear to adapt
        rank: rank of the update ``lora_up.weight @ lora_down.weight``
        scale: factor on the low-rank branch
        num_packed_linear: > 1 for a fused projection (kv: 2, qkv: 3): the bottleneck is that many times ``rank`` wide while the
            initialisation stays the one of a single Linear of rank ``rank``
    """

    def __init__(self, linear: nn.Module, rank: int = 4, scale: float = 1.0, num_packed_linear: int = 1):
        super().__init__()
        self.rank, self.scale = rank, scale
        self.in_features, self.out_features = linear.in_features, linear.out_features
        width = num_packed_linear * rank
        if width < 1 or width > min(self.in_features, self.out_features):
            raise ValueError(f"LoRA rank {num_packed_linear} * {rank} must be between 1 and {min(self.in_features, self.out_features)}")
        self.linear = linear
        kw = dict(device=linear.weight.device, dtype=linear.weight.dtype)
        self.lora_down = nn.Linear(self.in_features, width, bias=False, **kw)
        self.lora_up = nn.Linear(width, self.out_features, bias=False, **kw)
        nn.init.normal_(self.lora_down.weight, std=1 / rank)
        nn.init.zeros_(self.lora_up.weight)

    # the engine reads ``<module>.weight`` / ``.bias`` of every Linear it runs: those are the base Linear's
    @property
    def weight(self):
        return self.linear.weight

    @property
    def bias(self):
        return self.linear.bias

    def fuse_LoRA_into_linear(self) -> nn.Linear:
        """A plain Linear with ``W + scale * up @ down`` (and the base bias)."""
        w = self.linear.weight
        fused = nn.Linear(self.in_features, self.out_features, bias=self.linear.bias is not None, device=w.device, dtype=w.dtype)
        with torch.no_grad():
            fused.weight.copy_(w + self.scale * (self.lora_up.weight @ self.lora_down.weight))
            if self.linear.bias is not None:
                fused.bias.copy_(self.linear.bias)
        return fused

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """Stand-alone call (inference): three launches of the bf16 GEMM; inside FourM the engine runs the fused low-rank kernel instead."""
        from fourm.hip import functional as F
        return F.linear(x, self.linear.weight, self.linear.bias) + F.linear(F.linear(x, self.lora_down.weight, None), self.lora_up.weight, None) * self.scale


def _targets(model: nn.Module, ancestor_class: Optional[Set[str]], kind) -> Iterator[Tuple[nn.Module, str, nn.Module]]:
    """(parent, attribute name, module) of every ``kind`` module below a module whose class name is in ``ancestor_class`` (anywhere
    with None); what sits inside a LoRAWrapper is left alone."""
    seen = set()
    for anc in model.modules():
        if ancestor_class is not None and type(anc).__name__ not in ancestor_class:
            continue
        for parent in anc.modules():
            if isinstance(parent, LoRAWrapper):
                continue
            for name, child in parent.named_children():
                if isinstance(child, kind) and (id(parent), name) not in seen:
                    seen.add((id(parent), name))
                    yield parent, name, child


def _weights_changed(model: nn.Module) -> None:
    """The module tree changed under the engine: its flat parameter store and the bf16 weight shadows are rebuilt at the next call."""
    if hasattr(model, "_engine"):
        model._engine = None
    try:
        from fourm.hip.engine import bump_weight_epoch
    except ImportError:          # no kernel library: the model is a parameter container only
        return
    bump_weight_epoch()


def inject_trainable_LoRA(model: nn.Module, rank: int = 4, scale: float = 1.0, target_replace_modules: Set[str] = ATTENTION_MODULES) -> None:
    """Wrap, in place, every Linear of the ``target_replace_modules`` classes in a LoRAWrapper (qkv: 3 packed ranks, kv: 2)."""
    if set(target_replace_modules) & MLP_MODULES:
        raise NotImplementedError(_MLP_REASON)
    found = list(_targets(model, target_replace_modules, nn.Linear))
    for _, name, _ in found:       # refuse before the first module is replaced
        if rank * packed_linears(name) > MAX_LORA_WIDTH:
            raise ValueError(f"LoRA rank {rank} x {packed_linears(name)} packed Linears in '{name}' exceeds {MAX_LORA_WIDTH}, the widest "
                             "bottleneck the low-rank kernels hold on chip")
    for parent, name, child in found:
        parent._modules[name] = LoRAWrapper(child, rank=rank, scale=scale, num_packed_linear=packed_linears(name))
    _weights_changed(model)


def fuse_LoRA_into_linear(model: nn.Module, target_replace_modules: Set[str] = ATTENTION_MODULES) -> None:
    """Replace, in place, every LoRAWrapper of the ``target_replace_modules`` classes by one Linear holding ``W + scale * up @ down``."""
    for parent, name, child in list(_targets(model, target_replace_modules, LoRAWrapper)):
        parent._modules[name] = child.fuse_LoRA_into_linear()
    _weights_changed(model)


def unfreeze_all_LoRA_layers(model: nn.Module) -> None:
    """requires_grad = True on every adapter parameter."""
    for name, param in model.named_parameters():
        if "lora" in name:
            param.requires_grad = True
