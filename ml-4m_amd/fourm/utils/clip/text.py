"""CLIP's text tower on the HIP engine, and the logits of ``CLIP.forward``: the text half of what upstream's ``run_generation.py`` scores
text-to-image generation with (fourm/utils/clip/score.py has the score itself).

``TextTransformer`` holds the text half of upstream's ``CLIP`` under upstream's parameter names (an OpenAI state dict with its ``visual.*``
keys and ``logit_scale`` removed loads with ``strict=True``) and has its initialisation (model.py:363-390); ``forward`` / ``encode_text`` give
the three results of ``CLIP.encode_text`` (model.py:407-424).  The torch modules only HOLD the parameters.  The forward is a launch sequence on
one MI355X, inference only:

    fm_clip_text_embed (token rows + position rows -> fp32 residual stream; the end-of-text row of every sample; ids range-checked) -> the
    blocks on the tokenizer's engine (fourm/vq/engine.py) with the QuickGELU epilogue and the causal mask -> ln_final through a row map that
    picks the end-of-text rows -> one GEMM against the image of text_projection^T.

The causal mask is FM_MASK_DECODER with causal = 1 and no modality arrays (blocked[q][k] = k > q, upstream's triu(1) of -inf): the route of
fm_attn_fwd / fm_attn_f32_fwd that the trunk's causal decoder already takes - no kernel changed, no (B, Lc, Lc) mask tensor is built.

``compute_precision`` "bf16" (default) is upstream's autocast arithmetic, "fp32" the same launches on the fp32 kernels, as on
``VisionTransformer``.  Every result is fp32.  String tokenisation (``fourm.utils.clip.tokenize``), ``CLIP`` itself and ``clip.load`` stay
upstream's; no backward of the text tower exists."""
import math

import torch
from torch import nn

from .model import HEAD_DIM, _BlockView, _Stack

_NOT_TEXT = ("input_resolution", "context_length", "vocab_size", "logit_scale")


def _engine(tt):
    """The block executor of this tower: one per (device, precision), as for the vision tower (its own scratch and weight images)."""
    eng = tt.__dict__.get("_hip_engine")
    dev = tt.positional_embedding.device
    if eng is None or eng.device != dev or eng.precision != tt.compute_precision:
        if dev.type != "cuda":
            raise RuntimeError("CLIP's text tower computes on an MI355X through libfourm_hip.so; move it to the GPU first (there is no CPU path)")
        from fourm.vq.engine import _VitEngine
        eng = tt.__dict__["_hip_engine"] = _VitEngine(tt)
        eng.act = "quick_gelu"
    eng.prepare()
    return eng


class TextTransformer(nn.Module):
    def __init__(self, embed_dim: int, context_length: int, vocab_size: int, width: int, heads: int, layers: int):
        super().__init__()
        if heads <= 0 or width % heads or width // heads != HEAD_DIM:
            raise NotImplementedError(f"width {width} with {heads} heads: the HIP attention kernels are built for head_dim {HEAD_DIM}")
        self.embed_dim, self.context_length, self.vocab_size, self.width, self.heads = embed_dim, context_length, vocab_size, width, heads
        self.transformer = _Stack(width, layers, heads)
        self.token_embedding = nn.Embedding(vocab_size, width)
        self.positional_embedding = nn.Parameter(torch.empty(context_length, width))
        self.ln_final = nn.LayerNorm(width)
        self.text_projection = nn.Parameter(torch.empty(width, embed_dim))
        self.__dict__["_views"] = [_BlockView(b) for b in self.transformer.resblocks]
        self.initialize_parameters()

    def initialize_parameters(self):
        """The text part of upstream's CLIP.initialize_parameters (model.py:363-390)."""
        nn.init.normal_(self.token_embedding.weight, std=0.02)
        nn.init.normal_(self.positional_embedding, std=0.01)
        proj_std = (self.transformer.width ** -0.5) * ((2 * self.transformer.layers) ** -0.5)
        attn_std = self.transformer.width ** -0.5
        fc_std = (2 * self.transformer.width) ** -0.5
        for block in self.transformer.resblocks:
            nn.init.normal_(block.attn.in_proj_weight, std=attn_std)
            nn.init.normal_(block.attn.out_proj.weight, std=proj_std)
            nn.init.normal_(block.mlp.c_fc.weight, std=fc_std)
            nn.init.normal_(block.mlp.c_proj.weight, std=proj_std)
        nn.init.normal_(self.text_projection, std=self.transformer.width ** -0.5)

    # ---- the executor's view of this module ---------------------------------------------------------------------------------------
    @property
    def blocks(self):
        return self.__dict__["_views"]

    @property
    def dim_tokens(self):
        return self.width

    @property
    def compute_precision(self) -> str:
        """"bf16" (default): autocast arithmetic on the hot-path kernels; "fp32": the same launches on the fp32 kernels.  Read at every forward."""
        return self.__dict__.get("_compute_precision", "bf16")

    @compute_precision.setter
    def compute_precision(self, value: str):
        if value not in ("bf16", "fp32"):
            raise ValueError(f"compute_precision {value!r}: 'bf16' or 'fp32'")
        self.__dict__["_compute_precision"] = value

    # ---- construction from existing weights ---------------------------------------------------------------------------------------
    @classmethod
    def from_upstream(cls, module: nn.Module) -> "TextTransformer":
        """Adopt the text half of a loaded ``CLIP`` (``clip.load(...)[0]``, or any module with its state dict): the weights as fp32 copies on
        the module's device, eval mode, frozen."""
        sd = module.state_dict()
        return build_text(sd).to(sd["text_projection"].device)

    # ---- forward ------------------------------------------------------------------------------------------------------------------
    def forward(self, text: torch.Tensor, return_all_tokens=False, return_patch_tokens=False, check_ids=True):
        """text (B, context_length) int64 or int32 token ids.  Results (all fp32), in upstream's order of precedence: return_patch_tokens:
        ln_final of every token (B, Lc, width); return_all_tokens: every token projected (B, Lc, embed_dim); else the projected end-of-text
        row (the first maximum of each sample's ids) (B, embed_dim).  An id outside [0, vocab_size) raises ValueError after the launches
        (one synchronisation per call; check_ids=False skips it: such a row then enters the blocks as zeros)."""
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            raise NotImplementedError("CLIP's text tower runs at inference only on the HIP engine (no backward): call under torch.no_grad() "
                                      "or freeze it with requires_grad_(False)")
        if isinstance(text, str) or (isinstance(text, (list, tuple)) and any(isinstance(t, str) for t in text)):
            raise TypeError("the text tower takes token ids, not strings: tokenise with fourm.utils.clip.tokenize first")
        if not torch.is_tensor(text) or text.dtype not in (torch.int64, torch.int32) or text.dim() != 2 or text.shape[1] != self.context_length:
            got = f"{tuple(text.shape)} {text.dtype}" if torch.is_tensor(text) else type(text).__name__
            raise ValueError(f"expected token ids (B, {self.context_length}) int64 or int32, got {got}")
        if text.shape[0] == 0:
            raise ValueError("empty batch of token ids")
        eng = _engine(self)
        if text.device != eng.device:
            raise RuntimeError(f"input on {text.device}, model on {eng.device}")
        with torch.no_grad(), torch.cuda.device(eng.device):
            return self._forward(eng, text, return_all_tokens, return_patch_tokens, check_ids)

    encode_text = forward

    def _forward(self, eng, text, all_tokens, patch_tokens, check_ids):
        from fourm.hip import _lib as L
        from fourm.hip import ops
        from fourm.hip.engine import ru
        from fourm.vq.engine import _blocks_fwd
        f32, bf, i32 = torch.float32, torch.bfloat16, torch.int32
        ws, D = eng.ws, self.width
        ids = text.detach().long().contiguous()
        B, Lc = ids.shape
        R = B * Lc
        # every buffer of this tower lives under the prefix "cliptext" (and in this tower's own engine)
        stream = ws.get("cliptext.x0", (ru(R, 128), D), f32)
        eot_row, eot_map, bad = ws.get("cliptext.eot", (B,), i32), ws.get("cliptext.eot_map", (R,), i32), ws.get("cliptext.bad", (1,), i32)
        ops.clip_text_embed(ids, self.token_embedding.weight.detach(), self.positional_embedding.detach(), stream, eot_row, bad, eot_map)
        causal = dict(mask_kind=L.MASK_DECODER, causal=True)          # the k > q rule alone: cs / modq / modk absent
        stream = _blocks_fwd(eng, self, stream, B, Lc, None, "cliptext", mask=causal)
        eng._settle()
        fin = self.ln_final
        if patch_tokens:
            out = torch.empty(R, D, dtype=f32, device=ids.device)
            ops.layernorm_fwd(stream, fin.weight, fin.bias, out, eps=fin.eps, R=R)
            out = out.view(B, Lc, D)
        else:
            mode, M = ("all", R) if all_tokens else ("eot", B)
            n = ws.get("cliptext.post." + mode, (ru(M, 128), D), eng.adt)
            ops.layernorm_fwd(stream, fin.weight, fin.bias, n, row_map=None if all_tokens else eot_map, eps=fin.eps, R=R)
            O = self.embed_dim
            if eng.fp32:
                out = torch.empty(M, O, dtype=f32, device=ids.device)
                ops.gemm_nt(n, eng.wt(self.text_projection), out, epilogue=L.EPI_F32, M=M, N=O, K=D)
            else:
                # bf16 result as under autocast (x @ text_projection); up to 32 end-of-text rows are a launch of the few-row kernel
                o16 = ws.get("cliptext.out." + mode, (ru(M, 128), ru(O, 8)), bf)
                ops.gemm_nt(n, eng.wt(self.text_projection), o16, M=M, N=O, K=ru(D, 64))
                out = o16[:M, :O].float()
            out = out.view(B, Lc, O) if all_tokens else out
        if check_ids:
            n_bad = int(bad.item())
            if n_bad:
                raise ValueError(f"{n_bad} token ids lie outside [0, {self.vocab_size})")
        return out


def build_text(state_dict: dict) -> TextTransformer:
    """The text tower of a CLIP checkpoint: a full state dict (the ``visual.*`` keys, ``logit_scale`` and the three size entries are dropped) or
    a text-only one.  Sizes are read off the tensors as upstream's ``build_model`` reads them (model.py:485-490); half-precision checkpoints
    load as fp32 masters."""
    sd = {k: v for k, v in state_dict.items() if not k.startswith("visual.") and k not in _NOT_TEXT}
    for k in ("text_projection", "positional_embedding", "token_embedding.weight", "ln_final.weight"):
        if k not in sd:
            raise NotImplementedError(f"not a CLIP text tower: {k!r} is missing from the state dict")
    embed_dim = sd["text_projection"].shape[1]
    context_length = sd["positional_embedding"].shape[0]
    vocab_size = sd["token_embedding.weight"].shape[0]
    width = sd["ln_final.weight"].shape[0]
    layers = len(set(k.split(".")[2] for k in sd if k.startswith("transformer.resblocks")))
    tt = TextTransformer(embed_dim, context_length, vocab_size, width, width // HEAD_DIM, layers)
    tt.load_state_dict({k: v.detach().float() for k, v in sd.items()}, strict=True)
    return tt.eval().requires_grad_(False)


def clip_logits(image_features: torch.Tensor, text_features: torch.Tensor, logit_scale):
    """(logits_per_image (N, M), logits_per_text (M, N)) of upstream's ``CLIP.forward`` (model.py:426-440) from image features (N, E), text
    features (M, E) and ``logit_scale`` (the parameter, a tensor or a number; its exp multiplies the logits): two fm_l2_normalize_rows
    launches, exp(logit_scale) folded into the first, then fm_gemm_f32.  The second result is the transposed view of the first."""
    from fourm.hip import _lib as L
    from fourm.hip import ops
    if not (torch.is_tensor(image_features) and torch.is_tensor(text_features)) or image_features.dim() != 2 or text_features.dim() != 2 \
            or image_features.shape[1] != text_features.shape[1] or 0 in image_features.shape or 0 in text_features.shape:
        raise ValueError("clip_logits: image features (N, E) and text features (M, E) expected")
    if not (image_features.is_cuda and text_features.is_cuda):
        raise RuntimeError("clip_logits runs on the HIP kernels only (tensors on an MI355X; there is no CPU path)")
    dev = image_features.device
    with torch.no_grad(), torch.cuda.device(dev):
        img, txt = image_features.detach().float().contiguous(), text_features.detach().float().contiguous()
        if torch.is_tensor(logit_scale):
            factor, factor_dev = 1.0, logit_scale.detach().float().exp().reshape(1).to(dev)
        else:
            factor, factor_dev = math.exp(float(logit_scale)), None
        a = ops.l2_normalize_rows(img, torch.empty_like(img), factor, factor_dev)
        b = ops.l2_normalize_rows(txt, torch.empty_like(txt))
        (N, E), M = img.shape, txt.shape[0]
        out = torch.empty(N, M, dtype=torch.float32, device=dev)
        ops.gemm_nt(a, b, out, epilogue=L.EPI_F32, M=N, N=M, K=E)
    return out, out.t()
