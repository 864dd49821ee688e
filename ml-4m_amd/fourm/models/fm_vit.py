"""A pre-trained 4M encoder as a plain RGB ViT on MI355X: transfer learning to classification, segmentation, depth.

API-compatible with upstream ``fourm/models/fm_vit.py`` (``FourMViT``, ``FMViT``, the 13 ``fm_vit_*`` factories): the same constructor
arguments and defaults, attribute tree and state-dict keys (``encoder_embeddings.rgb@{img_size}.*``, ``encoder.{i}.*``,
``encoder_norm.*``, ``output_head.*``), so an upstream FourMViT checkpoint loads with ``strict=True`` and a FourM checkpoint with
``strict=False``.  All patches are visible, there is no masking and no decoder; ``output_head`` is any ``nn.Module``.

The encoder runs on ``fourm.hip.vit_engine.ViTEngine`` inside ONE ``torch.autograd.Function``: its forward is the HIP forward, its
backward takes the gradient the head's autograd graph delivers and launches the hand-written backward, which leaves fp32 gradients in
``param.grad`` (views of the engine's flat gradient store, accumulating over calls) exactly where ``FourM``'s backward puts them.
"""
import copy
import math
from functools import partial
from typing import Optional, Union

import torch
from torch import nn

from fourm.data.modality_info import MODALITY_INFO
from fourm.utils.registry import register_model
from .encoder_embeddings import ImageEncoderEmbedding
from .fm_utils import Block, LayerNorm, act_name

try:  # the hub mixin only adds from_pretrained / push_to_hub
    from huggingface_hub import PyTorchModelHubMixin
except Exception:  # pragma: no cover
    class PyTorchModelHubMixin:  # type: ignore
        pass

__all__ = []


class _Encode(torch.autograd.Function):
    """pixels -> encoder output on the engine.  ``anchor`` (a trainable trunk parameter) makes the output part of the autograd graph;
    the parameter gradients do not travel through autograd - the engine writes them into its flat store."""

    @staticmethod
    def forward(ctx, x, anchor, engine):
        out = engine.vit_forward(x, save=True)
        ctx.engine, ctx.saved = engine, engine._ctx
        return out

    @staticmethod
    def backward(ctx, grad_out):
        eng = ctx.engine
        eng.attach_grads(zero=eng.grads_were_cleared())
        eng.vit_backward(ctx.saved, grad_out)
        ctx.saved = None
        return None, None, None


class FourMViT(nn.Module):
    """See upstream ``FourMViT`` for the meaning of the arguments; they are identical."""

    def __init__(self,
                 img_size=224,
                 patch_size=16,
                 in_chans=3,
                 dim=768,
                 encoder_depth=12,
                 num_heads=12,
                 mlp_ratio=4.0,
                 qkv_bias: bool = True,
                 proj_bias: bool = True,
                 mlp_bias: bool = True,
                 drop_path_rate: float = 0.0,
                 drop_rate: float = 0.0,
                 attn_drop_rate: float = 0.0,
                 act_layer: torch.Tensor = nn.GELU,
                 norm_layer: Union[partial, nn.Module] = partial(LayerNorm, eps=1e-6),
                 gated_mlp: bool = False,
                 qk_norm: bool = False,
                 encoder_norm=True,
                 output_head: Optional[nn.Module] = None):
        super().__init__()
        # refused before anything is built or launched
        if drop_rate > 0 or attn_drop_rate > 0:
            raise NotImplementedError(f"drop_rate={drop_rate}, attn_drop_rate={attn_drop_rate}: dropout inside attention / the MLP has no HIP "
                                      "path (use drop_path_rate for regularisation)")
        if dim % num_heads or dim // num_heads != 64:
            raise NotImplementedError(f"dim {dim} / num_heads {num_heads}: the HIP attention kernels are built for head_dim 64")
        if encoder_depth < 1:
            raise ValueError("encoder_depth must be at least 1")
        act = act_name(act_layer())          # raises for anything but SiLU / exact GELU
        if (gated_mlp and act != "silu") or (not gated_mlp and act != "gelu"):
            raise NotImplementedError(f"{'gated ' if gated_mlp else ''}MLP with {act_layer.__name__}: the HIP epilogues implement the "
                                      "SiLU-gated MLP (SwiGLU) and the plain MLP with exact GELU only")
        self.img_size = img_size
        self.dim = dim
        self.init_std = 0.02
        # "bf16": the hot path (upstream's autocast arithmetic); "fp32": verification kernels without any rounding (set before the
        # first forward, or afterwards followed by ``model._engine = None``)
        self.compute_precision = "bf16"
        rgb_embedding = ImageEncoderEmbedding(num_channels=in_chans, patch_size=patch_size, dim_tokens=dim, sincos_pos_emb=True,
                                              image_size=img_size)
        self.num_patches = rgb_embedding.num_patches
        self.encoder_embeddings = nn.ModuleDict({f"rgb@{img_size}": rgb_embedding})
        dpr = [r.item() for r in torch.linspace(0, drop_path_rate, encoder_depth)]
        self.encoder = nn.ModuleList([
            Block(dim=dim, num_heads=num_heads, mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, proj_bias=proj_bias, mlp_bias=mlp_bias,
                  drop_path=dpr[i], drop=drop_rate, attn_drop=attn_drop_rate, act_layer=act_layer, norm_layer=norm_layer,
                  gated_mlp=gated_mlp, qk_norm=qk_norm)
            for i in range(encoder_depth)])
        self.encoder_norm = norm_layer(dim) if encoder_norm else nn.Identity()
        self.init_weights()
        # attached after init_weights(): a head may bring its own initialisation scale
        if output_head is not None:
            self.output_head = output_head
            if hasattr(self.output_head, "init"):
                self.output_head.init(dim)
        else:
            self.output_head = nn.Identity()
        self._engine = None
        try:        # stand-alone ``blk(x)`` calls find the engine through this registry (fourm/hip/functional.py)
            from fourm.hip.functional import register_blocks
            register_blocks(self)
        except (ImportError, OSError):      # no (loadable) kernel library: the model is a parameter container only (state_dict tools)
            pass

    def init_weights(self):
        """MAE-style initialisation: Xavier-uniform Linears with the fused qkv / kv matrices treated as separate square blocks,
        unit LayerNorms, N(0, 0.02) embeddings."""
        for name, mod in self.named_modules():
            if "tokenizer" in name:
                continue
            if isinstance(mod, nn.Linear):
                fused = 3 if "qkv" in name else 2 if "kv" in name else 1
                if fused > 1:
                    bound = math.sqrt(6. / float(mod.weight.shape[0] // fused + mod.weight.shape[1]))
                    nn.init.uniform_(mod.weight, -bound, bound)
                else:
                    nn.init.xavier_uniform_(mod.weight)
                if mod.bias is not None:
                    nn.init.constant_(mod.bias, 0)
            elif isinstance(mod, (nn.LayerNorm, LayerNorm)):
                nn.init.constant_(mod.weight, 1.0)
                if mod.bias is not None:
                    nn.init.constant_(mod.bias, 0)
            elif isinstance(mod, nn.Embedding):
                nn.init.normal_(mod.weight, std=self.init_std)

    def get_num_layers_encoder(self):
        return len(self.encoder)

    def get_num_layers(self):
        return self.get_num_layers_encoder()

    @torch.jit.ignore
    def no_weight_decay(self):
        skip = set()
        for mod, emb in self.encoder_embeddings.items():
            if hasattr(emb, "no_weight_decay"):
                skip |= {f"encoder_embeddings.{mod}.{n}" for n in emb.no_weight_decay()}
        return skip

    # ------------------------------------------------------------------------------------------
    # engine plumbing
    # ------------------------------------------------------------------------------------------
    def engine_parameters(self):
        """(name, parameter) of what the engine owns: embedding, blocks, encoder_norm - not the output head, which is torch's."""
        for prefix in ("encoder_embeddings", "encoder", "encoder_norm"):
            for n, p in getattr(self, prefix).named_parameters():
                yield f"{prefix}.{n}", p

    @property
    def engine(self):
        from fourm.hip.vit_engine import ViTEngine
        if self._engine is None:
            if not self.encoder[0].norm1.weight.is_cuda:
                raise RuntimeError("FourMViT computes on an MI355X through libfourm_hip.so; move the model to the GPU first "
                                   "(there is no CPU implementation of the hot path)")
            self._engine = ViTEngine(self)
            from fourm.hip.functional import register_blocks
            register_blocks(self)
        return self._engine

    def _apply(self, fn, *a, **k):
        out = super()._apply(fn, *a, **k)
        self._engine = None          # parameters moved / changed dtype: rebuild stores and shadows lazily
        return out

    def __getstate__(self):
        d = self.__dict__.copy()
        d["_engine"] = None
        return d

    def _check_input(self, x):
        emb = self.encoder_embeddings[f"rgb@{self.img_size}"]
        if x.dim() != 4:
            raise ValueError(f"FourMViT expects a (B, C, H, W) image batch, got a tensor of shape {tuple(x.shape)}")
        if tuple(x.shape[2:]) != tuple(emb.image_size):
            raise ValueError(f"input of {x.shape[2]} x {x.shape[3]} pixels: this model is built for {emb.image_size[0]} x {emb.image_size[1]} "
                             "(its position embedding is a fixed table; resize the images or build the model with another img_size)")
        if x.shape[1] != emb.num_channels:
            raise ValueError(f"input has {x.shape[1]} channels, the patch projection expects {emb.num_channels}")
        if isinstance(emb.pos_emb, nn.Parameter) and emb.pos_emb.requires_grad:
            raise NotImplementedError("a learned (trainable) pos_emb has no gradient path in FourMViT: every FourMViT carries the sin-cos buffer")

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """x (B, C, H, W) -> output_head(encoder_norm(blocks(patches(x) + emb))); the encoder output is fp32 (B, num_patches, dim)."""
        self._check_input(x)
        eng = self.engine
        train = torch.is_grad_enabled() and self.training
        anchor = next((p for _, p in self.engine_parameters() if p.requires_grad), None) if train else None
        if anchor is None:          # no_grad / eval / linear probing on a frozen encoder: nothing is saved, no engine backward
            feats = eng.vit_forward(x, save=False)
        else:
            feats = _Encode.apply(x, anchor, eng)
        return self.output_head(feats)

    def _set_trainable(self, modules, flag):
        for m in modules:
            for p in m.parameters():
                p.requires_grad = flag

    def freeze_encoder(self, freeze_embeddings=True):
        self._set_trainable([self.encoder, self.encoder_norm] + ([self.encoder_embeddings] if freeze_embeddings else []), False)

    def unfreeze_encoder(self, unfreeze_embeddings=True):
        self._set_trainable([self.encoder, self.encoder_norm] + ([self.encoder_embeddings] if unfreeze_embeddings else []), True)


class FMViT(FourMViT, PyTorchModelHubMixin):
    """``FMViT(config, output_head)``: a FourMViT from the config dict stored with released 4M checkpoints (keys ``image_size``,
    ``patch_size``, ``norm_bias``, ``act_layer`` plus FourMViT keyword arguments; the FourM-only keys are dropped)."""

    def __init__(self, config: dict, output_head: Optional[nn.Module] = None):
        cfg = copy.deepcopy(config)
        cfg["norm_layer"] = partial(LayerNorm, eps=1e-6, bias=cfg["norm_bias"])
        cfg["act_layer"] = getattr(torch.nn, cfg["act_layer"])
        img_size = cfg["image_size"]
        info = MODALITY_INFO[f"rgb@{img_size}"]
        cfg["img_size"] = img_size
        cfg["patch_size"] = info.get("patch_size", cfg["patch_size"])
        cfg["in_chans"] = info.get("num_channels", 3)
        for key in ("image_size", "norm_bias", "domains_in", "domains_out", "decoder_depth", "share_modality_embeddings"):
            cfg.pop(key, None)
        super().__init__(output_head=output_head, **cfg)


# --------------------------------------------------------------------------------------------------
# named configurations: (dim, depth, heads)
# --------------------------------------------------------------------------------------------------
_SIZES = {"tiny_6e": (384, 6, 6), "small_8e": (512, 8, 8), "base_12e": (768, 12, 12), "large_24e": (1024, 24, 16), "xlarge_24e": (2048, 24, 32)}


def _factory(name, size, **fixed):
    dim, depth, heads = _SIZES[size]

    def build(**kwargs):
        return FourMViT(encoder_depth=depth, dim=dim, num_heads=heads, mlp_ratio=4, **fixed, **kwargs)
    build.__name__ = build.__qualname__ = name
    build.__module__ = __name__
    globals()[name] = register_model(build, listed=False)      # (list_models('fm_*') stays the 13 pre-training architectures)
    __all__.append(name)


_GELU = dict(qkv_bias=True, norm_layer=partial(nn.LayerNorm, eps=1e-6))
_SWIGLU = dict(qkv_bias=False, proj_bias=False, mlp_bias=False, norm_layer=partial(LayerNorm, eps=1e-6, bias=False),
               act_layer=nn.SiLU, gated_mlp=True)
for _size in _SIZES:
    _factory(f"fm_vit_{_size}_gelu", _size, **_GELU)
for _size in _SIZES:
    _factory(f"fm_vit_{_size}_swiglu_nobias", _size, **_SWIGLU)
for _size in ("base_12e", "large_24e", "xlarge_24e"):
    _factory(f"fm_vit_{_size}_swiglu_qknorm_nobias", _size, qk_norm=True, **_SWIGLU)
