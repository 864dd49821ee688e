"""CLIP's vision tower on the HIP engine: the feature network in front of the ``tok_clip`` tokenizer.

``VisionTransformer`` has upstream's constructor, parameter names (an OpenAI ViT checkpoint loads with ``strict=True``), initialisation and
the four results of ``forward`` (upstream fourm/utils/clip/model.py:227-305); the torch modules below only HOLD the parameters.  The
forward is a launch sequence on one MI355X, inference only:

    fm_vq_patchify (rows in conv-weight order c, py, px) -> patch GEMM (conv1, bias-free) -> fm_clip_embed_ln (class token, position
    table, ln_pre in one pass -> fp32 residual stream) -> the blocks on the tokenizer's engine (fourm/vq/engine.py: LayerNorm, qkv GEMM +
    bias, unmasked fused attention, c_fc with the QuickGELU epilogue FM_EPI_QUICK_GELU, residual epilogues) -> ln_post through a row map
    that drops or picks the class rows -> one GEMM against the image of proj^T.

``compute_precision`` "bf16" (default) is upstream's autocast arithmetic: bf16 GEMM operands, fp32 accumulation, fp32 residual stream,
LayerNorm statistics and softmax.  "fp32" runs the same sequence on the fp32 kernels (csrc/fp32_verify.hip): upstream's run without
autocast.  Every result is fp32.  ``CLIP``, ``ModifiedResNet``, ``build_model`` and ``clip.load`` stay upstream's (fourm/_upstream.py; the
text tower is fourm/utils/clip/text.py); ``VisionTransformer.from_upstream(model.visual)`` adopts a loaded tower.

``features`` / ``features_backward`` are the differentiable path of a FROZEN tower: the residual streams after chosen blocks and the gradient of
anything computed from them with respect to the input image (the perceptual loss of tokenizer training, fourm/vq/percept_losses).  ``forward``
itself stays inference only, and a tower with trainable parameters is refused by both."""
import math
from collections import OrderedDict

import torch
import torch.nn.functional as F
from torch import nn

HEAD_DIM = 64          # the HIP attention kernels are built for this width; CLIP's B/32, B/16 and L/14 towers all have it


def affine_fp32(x, scale, shift):
    """scale[c] * x + shift[c] on (B, C, H, W) with ONE rounding to fp32 per element, differentiable: the value the patch-gather kernel's fused
    multiply-add gives (fm_vq_patchify_ex), so an affine applied here and one folded into the kernel agree.  The product of two fp32 numbers is
    exact in float64; the sum is rounded to float64 and then to fp32."""
    return (x.double() * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)).float()


class QuickGELU(nn.Module):
    """x * sigmoid(1.702 x) - the activation of CLIP's MLP.  On the device it is the epilogue of the c_fc GEMM; this module marks the place."""

    def forward(self, x):
        return x * torch.sigmoid(1.702 * x)


class _Block(nn.Module):
    """Parameter holder of one pre-LN block under upstream's names: attn.in_proj_*, attn.out_proj.*, ln_1, mlp.c_fc, mlp.c_proj, ln_2."""

    def __init__(self, width, heads):
        super().__init__()
        self.attn = nn.MultiheadAttention(width, heads)
        self.ln_1 = nn.LayerNorm(width)
        self.mlp = nn.Sequential(OrderedDict(c_fc=nn.Linear(width, 4 * width), gelu=QuickGELU(), c_proj=nn.Linear(4 * width, width)))
        self.ln_2 = nn.LayerNorm(width)


class _Stack(nn.Module):
    def __init__(self, width, layers, heads):
        super().__init__()
        self.width, self.layers = width, layers
        self.resblocks = nn.Sequential(*[_Block(width, heads) for _ in range(layers)])


# ---- what the block executor reads (attn.qkv / attn.proj / mlp.fc1 / mlp.fc2 / norm1 / norm2), presented over the names above -----
class _LinearView:
    def __init__(self, owner, weight_name, bias_name):
        self._owner, self._w, self._b = owner, weight_name, bias_name

    @property
    def weight(self):
        return getattr(self._owner, self._w)

    @property
    def bias(self):
        return getattr(self._owner, self._b)

    @property
    def out_features(self):
        return self.weight.shape[0]

    @property
    def in_features(self):
        return self.weight.shape[1]


class _AttnView:
    def __init__(self, mha):
        self.num_heads = mha.num_heads
        self.qkv = _LinearView(mha, "in_proj_weight", "in_proj_bias")
        self.proj = mha.out_proj


class _MlpView:
    def __init__(self, mlp):
        self.fc1, self.fc2 = mlp.c_fc, mlp.c_proj
        self.hidden_features = mlp.c_fc.out_features


class _BlockView:
    def __init__(self, blk):
        self.norm1, self.norm2 = blk.ln_1, blk.ln_2
        self.attn, self.mlp = _AttnView(blk.attn), _MlpView(blk.mlp)


def _engine(vit):
    """The block executor of this tower: one per (device, precision), rebuilt when either changes (scratch and weight images of the other go)."""
    eng = vit.__dict__.get("_hip_engine")
    dev = vit.class_embedding.device
    if eng is None or eng.device != dev or eng.precision != vit.compute_precision:
        if dev.type != "cuda":
            raise RuntimeError("CLIP's vision tower computes on an MI355X through libfourm_hip.so; move it to the GPU first (there is no CPU path)")
        from fourm.vq.engine import _VitEngine
        eng = vit.__dict__["_hip_engine"] = _VitEngine(vit)
        eng.act = "quick_gelu"          # c_fc runs with FM_EPI_QUICK_GELU (FourMEngine._mlp_fwd)
    eng.prepare()
    return eng


class VisionTransformer(nn.Module):
    def __init__(self, input_resolution: int, patch_size: int, width: int, layers: int, heads: int, output_dim: int):
        super().__init__()
        if heads <= 0 or width % heads or width // heads != HEAD_DIM:
            raise NotImplementedError(f"width {width} with {heads} heads: the HIP attention kernels are built for head_dim {HEAD_DIM}")
        self.input_resolution, self.patch_size, self.output_dim, self.width, self.heads = input_resolution, patch_size, output_dim, width, heads
        self.conv1 = nn.Conv2d(3, width, kernel_size=patch_size, stride=patch_size, bias=False)
        scale = width ** -0.5
        self.class_embedding = nn.Parameter(scale * torch.randn(width))
        self.positional_embedding = nn.Parameter(scale * torch.randn((input_resolution // patch_size) ** 2 + 1, width))
        self.ln_pre = nn.LayerNorm(width)
        self.transformer = _Stack(width, layers, heads)
        self.ln_post = nn.LayerNorm(width)
        self.proj = nn.Parameter(scale * torch.randn(width, output_dim))
        self.__dict__["_views"] = [_BlockView(b) for b in self.transformer.resblocks]
        self.__dict__["_tables"] = {}

    # ---- the executor's view of this module ---------------------------------------------------------------------------------------
    @property
    def blocks(self):
        return self.__dict__["_views"]

    @property
    def dim_tokens(self):
        return self.width

    @property
    def compute_precision(self) -> str:
        """"bf16" (default): autocast arithmetic on the hot-path kernels; "fp32": the same launches on the fp32 kernels.  Assign after
        construction; read at every forward."""
        return self.__dict__.get("_compute_precision", "bf16")

    @compute_precision.setter
    def compute_precision(self, value: str):
        if value not in ("bf16", "fp32"):
            raise ValueError(f"compute_precision {value!r}: 'bf16' or 'fp32'")
        self.__dict__["_compute_precision"] = value

    # ---- construction from existing weights ---------------------------------------------------------------------------------------
    @classmethod
    def from_upstream(cls, module: nn.Module) -> "VisionTransformer":
        """Adopt a loaded tower (``clip.load(...)[0].visual``, or any module with its attributes and state dict): same sizes, the weights as
        fp32 copies on the module's device, eval mode."""
        sd = module.state_dict()
        layers = len([k for k in sd if k.endswith(".attn.in_proj_weight")])
        vit = cls(module.input_resolution, module.patch_size, sd["conv1.weight"].shape[0], layers, module.heads, sd["proj"].shape[1])
        vit.load_state_dict({k: v.detach().float() for k, v in sd.items()}, strict=True)
        return vit.to(sd["proj"].device).eval().requires_grad_(False)

    # ---- forward ------------------------------------------------------------------------------------------------------------------
    def forward(self, x: torch.Tensor, return_all_tokens=False, return_all_final_tokens=False, return_final_tokens_no_cls=False, **kwargs):
        """x (B, 3, H, W), H and W multiples of the patch size.  Results (all fp32), in upstream's order of precedence:
        return_all_tokens: ln_post of the patch tokens (B, G, width); return_all_final_tokens: every token projected (B, G + 1, output_dim);
        return_final_tokens_no_cls: the patch tokens projected (B, G, output_dim) - the input of the tok_clip tokenizer; else the projected
        class token (B, output_dim)."""
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            raise NotImplementedError("CLIP's vision tower runs at inference only on the HIP engine (no backward): call under torch.no_grad() "
                                      "or freeze it with requires_grad_(False)")
        if x.dim() != 4 or x.shape[1] != self.conv1.in_channels:
            raise ValueError(f"expected images (B, {self.conv1.in_channels}, H, W), got {tuple(x.shape)}")
        P = self.patch_size
        if x.shape[2] % P or x.shape[3] % P:
            raise ValueError(f"image size {x.shape[2]}x{x.shape[3]} must be divisible by the patch size {P}")
        eng = _engine(self)
        if x.device != eng.device:
            raise RuntimeError(f"input on {x.device}, model on {eng.device}")
        with torch.no_grad():
            return self._forward(eng, x, return_all_tokens, return_all_final_tokens, return_final_tokens_no_cls)

    def _forward(self, eng, x, all_tokens, all_final, no_cls):
        from fourm.hip import _lib as L
        from fourm.hip import ops
        from fourm.hip.engine import ru
        from fourm.vq.engine import _blocks_fwd
        f32, bf = torch.float32, torch.bfloat16
        ws, D = eng.ws, self.width
        stream, _, _, (B, G) = self._embed(eng, x, "clip")
        T, Rg = G + 1, B * G
        R = B * T
        stream = _blocks_fwd(eng, self, stream, B, T, None, "clip")
        eng._settle()
        # ln_post on the rows that are returned (the row map drops or picks the class rows), then the projection
        post = self.ln_post
        if all_tokens:
            out = torch.empty(Rg, D, dtype=f32, device=x.device)
            ops.layernorm_fwd(stream, post.weight, post.bias, out, row_map=self._row_map("patches", B, T, x.device), eps=post.eps, R=R)
            return out.view(B, G, D)
        mode, M = ("all", R) if all_final else ("patches", Rg) if no_cls else ("cls", B)
        n = ws.get("clip.post." + mode, (ru(M, 128), D), eng.adt)
        ops.layernorm_fwd(stream, post.weight, post.bias, n, row_map=None if all_final else self._row_map(mode, B, T, x.device), eps=post.eps, R=R)
        O = self.output_dim
        if eng.fp32:
            out = torch.empty(M, O, dtype=f32, device=x.device)
            ops.gemm_nt(n, eng.wt(self.proj), out, epilogue=L.EPI_F32, M=M, N=O, K=D)
        else:
            # bf16 result as under autocast (x @ proj); a class-token batch of up to 32 rows is a launch of the few-row kernel
            o16 = ws.get("clip.out." + mode, (ru(M, 128), ru(O, 8)), bf)
            ops.gemm_nt(n, eng.wt(self.proj), o16, M=M, N=O, K=ru(D, 64))
            out = o16[:M, :O].float()
        return out if mode == "cls" else out.view(B, M // B, O)

    def _embed(self, eng, x, prefix, scale=None, shift=None):
        """Images -> the fp32 residual stream in front of block 0 (buffers named under ``prefix``): conv1 as a GEMM on patch rows
        'b c (gh p) (gw q) -> (b gh gw) (c p q)' (the column order of the flattened convolution weight), then class token + position table +
        ln_pre.  ``scale`` / ``shift`` (fp32 (3,) device tensors): the per-channel affine scale * x + shift applied while the rows are gathered.
        Returns (stream, patch-projection rows, position table, (B, G))."""
        from fourm.hip import _lib as L
        from fourm.hip import ops
        from fourm.hip.engine import ru
        f32, bf = torch.float32, torch.bfloat16
        ws, D, P = eng.ws, self.width, self.patch_size
        B, C, H, W = x.shape
        gh, gw = H // P, W // P
        G = gh * gw
        Rg, R = B * G, B * (G + 1)
        Rp, Rgp, feat = ru(R, 128), ru(Rg, 128), C * P * P
        x = x.float().contiguous()
        if eng.fp32:
            if scale is not None:
                x = affine_fp32(x, scale, shift)
            rows = ws.get(prefix + ".patches32", (Rgp, feat), f32)
            rows[:Rg].view(B, gh, gw, C, P, P).copy_(x.view(B, C, gh, P, gw, P).permute(0, 2, 4, 1, 3, 5))        # (plumbing)
            patches = ws.get(prefix + ".proj32", (Rgp, D), f32)
            ops.gemm_nt(rows, eng.w(self.conv1.weight), patches, epilogue=L.EPI_F32, M=Rg, N=D, K=feat)
        else:
            rows = ws.get(prefix + ".patches", (Rgp, ru(feat, 64)), bf)
            if scale is None:
                L.check(L.vq_patchify(ops._p(x), ops._p(rows), rows.stride(0), B, C, H, W, P, ops._stream()))
            else:
                L.check(L.vq_patchify_ex(ops._p(x), None, None, ops._p(scale), ops._p(shift), ops._p(rows), rows.stride(0), B, C, H, W, P, ops._stream()))
            patches = ws.get(prefix + ".proj", (Rgp, D), bf)
            ops.gemm_nt(rows, eng.w(self.conv1.weight), patches, M=Rg, N=D, K=ru(feat, 64))
        # class token + position table + ln_pre -> the fp32 residual stream
        pos = self._pos_table(gh, gw, x.device)
        stream = ws.get(prefix + ".x0", (Rp, D), f32)
        L.check(L.clip_embed_ln(ops._p(patches), patches.stride(0), 1 if eng.fp32 else 0, ops._p(self.class_embedding), ops._p(pos), ops._p(self.ln_pre.weight),
                                ops._p(self.ln_pre.bias), ops._p(stream), stream.stride(0), B, G, D, self.ln_pre.eps, ops._stream()))
        return stream, patches, pos, (B, G)

    # ---- the differentiable path of a FROZEN tower: residual streams after some blocks, and the gradient back to the pixels ------------
    def features(self, x: torch.Tensor, taps, save: bool, scale=None, shift=None):
        """Residual streams after the blocks in ``taps`` (indices; every token, class token included) for images x (B, 3, H, W): the launch
        sequence of ``forward`` up to the highest tap, without ln_post or the projection.  Returns ({tap: (B * T, width) fp32 rows}, saved).
        save=False: the rows are copies and ``saved`` is None.  save=True: the rows are the engine's own buffers and ``saved`` is what
        ``features_backward`` needs - it lives in the engine's named workspace, so the tower keeps ONE saved pass: the most recent one.
        ``scale`` / ``shift``: a per-channel affine folded into the patch gather (``features_backward`` then applies ``scale`` on the way out)."""
        if any(p.requires_grad for p in self.parameters()):
            raise NotImplementedError("the tower's differentiable path is that of a frozen tower (gradient to the input image only): "
                                      "freeze it with requires_grad_(False)")
        taps = sorted(set(int(t) for t in taps))
        if not taps or taps[0] < 0 or taps[-1] >= len(self.blocks):
            raise ValueError(f"taps {taps}: block indices in range({len(self.blocks)}) expected")
        if x.dim() != 4 or x.shape[1] != self.conv1.in_channels:
            raise ValueError(f"expected images (B, {self.conv1.in_channels}, H, W), got {tuple(x.shape)}")
        P = self.patch_size
        if x.shape[2] % P or x.shape[3] % P:
            raise ValueError(f"image size {x.shape[2]}x{x.shape[3]} must be divisible by the patch size {P}")
        eng = _engine(self)
        if x.device != eng.device:
            raise RuntimeError(f"input on {x.device}, model on {eng.device}")
        from fourm.hip import _lib as L
        none = dict(mask_kind=L.MASK_NONE)
        with torch.no_grad():
            if save:
                self.__dict__["_feat_saved"] = None                  # (the buffers of an earlier saving pass are about to be rewritten)
            stream, patches, pos, (B, G) = self._embed(eng, x, "clipf" if save else "clip", scale, shift)
            T = G + 1
            R, top, out, layers = B * T, taps[-1], {}, []
            for i in range(top + 1):
                sv = {} if save else None
                nxt = eng.encoder_block_fwd(self.blocks[i], stream, B, T, none, sv, f"clipf{i}" if save else f"clip{i % 2}", defer_out=i < top)
                layers.append(sv)
                if i - 1 in taps:                                    # block i's norm1 has written the stream after block i - 1
                    out[i - 1] = stream[:R] if save else stream[:R].clone()
                stream = nxt
            eng._settle()
            out[top] = stream[:R] if save else stream[:R].clone()
            saved = None
            if save:
                saved = self.__dict__["_feat_saved"] = dict(eng=eng, layers=layers, patches=patches, pos=pos, dims=(B, G, x.shape[2], x.shape[3]),
                                                            top=top, scale=scale)
        return out, saved

    def features_backward(self, saved, d_taps, row_scale=None):
        """Gradient with respect to the images of the ``features(..., save=True)`` pass that returned ``saved``.  d_taps {tap: (>= B * T, width)
        fp32 gradient rows}, ``row_scale`` (B,) fp32 or None: sample b's rows of every tap gradient are multiplied by row_scale[b] as they
        enter.  Walks the blocks from the highest tap down (before block i's backward, tap i's gradient is added to the fp32 stream gradient
        and its bf16 copy refreshed), then the embedding + ln_pre backward, the patch projection and the un-patching.  No parameter
        gradient is produced."""
        if saved is None or saved is not self.__dict__.get("_feat_saved") or saved["eng"] is not self.__dict__.get("_hip_engine"):
            raise RuntimeError("CLIP tower backward: the engine keeps the state of the most recent training forward only "
                               "(run forward and backward of one batch before the next forward)")
        self.__dict__["_feat_saved"] = None
        from fourm.hip import _lib as L
        from fourm.hip import ops
        from fourm.hip.engine import ru
        eng = saved["eng"]
        f32 = torch.float32
        ws, D, P = eng.ws, self.width, self.patch_size
        B, G, H, W = saved["dims"]
        T, Rg, C = G + 1, B * G, self.conv1.in_channels
        R, feat = B * T, C * P * P
        Rp, Rgp = ru(R, 128), ru(Rg, 128)
        none = dict(mask_kind=L.MASK_NONE)
        with torch.no_grad():
            g = ws.get("bwd.clipf.g", (Rp, D), f32)
            g_bf = ws.get("bwd.clipf.g_bf", (Rp, D), eng.adt)
            g.zero_()
            for i in reversed(range(saved["top"] + 1)):
                if i in d_taps:
                    ops.tap_add(g, d_taps[i], None if eng.fp32 else g_bf, row_scale, T, R)
                    if eng.fp32:
                        g_bf.copy_(g)
                eng.encoder_block_bwd(self.blocks[i], saved["layers"][i], g, g_bf, B, T, none)
            patches = saved["patches"]
            dpat = ws.get("bwd.clipf.dpat", (Rgp, D), eng.adt)
            L.check(L.clip_embed_ln_bwd(ops._p(g), g.stride(0), ops._p(patches), patches.stride(0), 1 if eng.fp32 else 0, ops._p(saved["pos"]),
                                        ops._p(self.ln_pre.weight), ops._p(dpat), dpat.stride(0), B, G, D, self.ln_pre.eps, ops._stream()))
            drows = ws.get("bwd.clipf.drows", (Rgp, feat), f32)
            ops.gemm_nt(dpat, eng.wt(self.conv1.weight), drows, epilogue=L.EPI_F32, M=Rg, N=feat, K=D)        # d(rows) = d(patches) conv1.weight
            img = torch.empty(B, C, H, W, dtype=f32, device=g.device)
            L.check(L.vq_unpatchify(ops._p(drows), drows.stride(0), ops._p(img), B, C, H, W, P, ops._stream()))
            if saved["scale"] is not None:
                img *= saved["scale"].view(1, C, 1, 1)
        return img

    def _row_map(self, mode, B, T, device):
        """Destination row of every stream row for ln_post (-1: not normalised into the output)."""
        key = ("rows", mode, B, T, str(device))
        m = self._tables.get(key)
        if m is None:
            t = torch.arange(B * T, dtype=torch.int64).view(B, T)
            b, j = t // T, t % T
            m = torch.where(j == 0, b, torch.full_like(t, -1)) if mode == "cls" else torch.where(j == 0, torch.full_like(t, -1), b * (T - 1) + j - 1)
            m = self._tables[key] = m.reshape(-1).to(torch.int32).to(device)
        return m

    def _pos_table(self, gh, gw, device):
        """(gh * gw + 1, width) fp32 position rows for a (gh, gw) patch grid, built once per grid and parameter version.  The native table
        whenever the token count matches it; otherwise the patch part resized as upstream's interpolate_pos_encoding does it (model.py:285-305:
        bicubic, scale factors (g + 0.1) / sqrt(N)) - evaluated on the host in fp32, the arithmetic of upstream's own CPU run."""
        pe = self.positional_embedding
        key = ("pos", gh, gw, pe._version, pe.data_ptr(), str(device))
        t = self._tables.get(key)
        if t is None:
            src = pe.detach().float()
            n = src.shape[0] - 1
            if gh * gw == n:
                t = src.contiguous()
            else:
                side, root = int(math.sqrt(n)), math.sqrt(n)
                grid = src[1:].cpu().reshape(1, side, side, self.width).permute(0, 3, 1, 2)
                grid = F.interpolate(grid, scale_factor=((gh + 0.1) / root, (gw + 0.1) / root), mode="bicubic")
                if tuple(grid.shape[-2:]) != (gh, gw):
                    raise RuntimeError(f"position table resized to {tuple(grid.shape[-2:])}, expected {(gh, gw)}")
                t = torch.cat([src[:1].cpu(), grid.permute(0, 2, 3, 1).reshape(gh * gw, self.width)], dim=0).contiguous()
            for k in [k for k in self._tables if k[0] == "pos" and k[3:5] != key[3:5]]:      # tables of an older parameter version go
                del self._tables[k]
            t = self._tables[key] = t.to(device)
            if device.type == "cuda":
                torch.cuda.current_stream(device).synchronize()
        return t

    def interpolate_pos_encoding(self, x, w, h):
        """Upstream's helper, kept for callers: the (1, tokens, width) table for an image of height ``w`` and width ``h`` (its names)."""
        return self._pos_table(w // self.patch_size, h // self.patch_size, self.positional_embedding.device).unsqueeze(0)


def build_visual(state_dict: dict) -> VisionTransformer:
    """The vision tower of a CLIP ViT checkpoint: a full state dict (keys under ``visual.``) or a visual-only one.  Sizes are read off the
    tensors as upstream's ``build_model`` reads them (model.py:467-475); half-precision checkpoints load as fp32 masters."""
    if any(k.startswith("visual.") for k in state_dict):
        state_dict = {k[len("visual."):]: v for k, v in state_dict.items() if k.startswith("visual.")}
    if "proj" not in state_dict or "conv1.weight" not in state_dict:
        raise NotImplementedError("not a CLIP ViT checkpoint (ModifiedResNet towers stay upstream's)")
    width = state_dict["conv1.weight"].shape[0]
    layers = len([k for k in state_dict if k.endswith(".attn.in_proj_weight")])
    patch = state_dict["conv1.weight"].shape[-1]
    grid = round((state_dict["positional_embedding"].shape[0] - 1) ** 0.5)
    vit = VisionTransformer(patch * grid, patch, width, layers, width // HEAD_DIM, state_dict["proj"].shape[1])
    vit.load_state_dict({k: v.detach().float() for k, v in state_dict.items()}, strict=True)
    return vit.eval().requires_grad_(False)


# names only upstream's same-named module defines (CLIP, ModifiedResNet, build_model, ...; see fourm/_upstream.py)
from fourm import _upstream as _up
_up.merge(__name__, globals())
