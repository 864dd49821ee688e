"""DINOv2's vision tower on the HIP engine: the feature network in front of the ``tok_dinov2`` and ``tok_dinov2_global`` tokenizers.

Upstream takes this network from ``torch.hub`` (save_vq_tokens.py:193-195, run_training_vqvae.py:444-451), so its source is not part of the
upstream checkout.  The definition written out in INTEGRATION.md ("DINOv2 tower") is the contract this module implements; parity with the
`facebookresearch/dinov2` package and with the real checkpoints is unpinned.

``DinoVisionTransformer`` has the package's constructor arguments, parameter names (a hub state dict with ``block_chunks=0`` key names loads with
``strict=True``) and results; the torch modules below only HOLD the parameters.  The forward is a launch sequence on one MI355X, inference only:

    fm_vq_patchify (rows in conv-weight order c, py, px; K = 3 * 14 * 14 = 588, padded to 640 in the bf16 path) -> patch GEMM (the conv bias
    on its bias=) -> fm_cls_pos_embed (class token, registers, position table of the grid -> fp32 residual stream) -> the blocks on the
    tokenizer's engine (fourm/vq/engine.py: LayerNorm, qkv GEMM + bias, unmasked fused attention, fc1 with the GELU epilogue or w12 with the
    SwiGLU epilogue; both residual sums carry LayerScale: the branch GEMM writes delta, and x + gamma * delta runs inside the LayerNorm that
    follows, fm_layernorm_fwd_res_ls, or in fm_layerscale_add after the last block) -> one fm_layernorm_fwd over all rows; the three
    ``x_norm_*`` results are views of it.

``compute_precision`` "bf16" (default) is autocast arithmetic: bf16 GEMM operands, fp32 accumulation, fp32 residual stream, LayerNorm
statistics, LayerScale and softmax.  "fp32" runs the same sequence on the fp32 kernels (csrc/fp32_verify.hip).  Every result is fp32."""
from functools import partial

import torch
import torch.nn.functional as F
from torch import nn

HEAD_DIM = 64          # the HIP attention kernels are built for this width; every hub configuration has it
LN_EPS = 1e-6


# ---- parameter holders under the package's names ---------------------------------------------------------------------------------------
class _PatchEmbed(nn.Module):
    def __init__(self, patch_size, in_chans, embed_dim):
        super().__init__()
        self.proj = nn.Conv2d(in_chans, embed_dim, kernel_size=patch_size, stride=patch_size)


class _Attention(nn.Module):
    def __init__(self, dim, num_heads):
        super().__init__()
        self.num_heads = num_heads
        self.qkv = nn.Linear(dim, 3 * dim)
        self.proj = nn.Linear(dim, dim)


class _LayerScale(nn.Module):
    def __init__(self, dim, init_values):
        super().__init__()
        self.gamma = nn.Parameter(init_values * torch.ones(dim))


class _Mlp(nn.Module):
    def __init__(self, dim, hidden):
        super().__init__()
        self.fc1 = nn.Linear(dim, hidden)
        self.fc2 = nn.Linear(hidden, dim)


class _SwiGLUFFNFused(nn.Module):
    """w3(silu(x1) * x2) with x1, x2 = w12(x).chunk(2, -1); the hidden width is (int(hidden * 2 / 3) + 7) // 8 * 8."""

    def __init__(self, dim, hidden):
        super().__init__()
        h = (int(hidden * 2 / 3) + 7) // 8 * 8
        self.w12 = nn.Linear(dim, 2 * h)
        self.w3 = nn.Linear(h, dim)


class _Block(nn.Module):
    def __init__(self, dim, num_heads, mlp_ratio, ffn_layer, init_values):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim, eps=LN_EPS)
        self.attn = _Attention(dim, num_heads)
        self.ls1 = _LayerScale(dim, init_values)
        self.norm2 = nn.LayerNorm(dim, eps=LN_EPS)
        self.mlp = _Mlp(dim, int(dim * mlp_ratio)) if ffn_layer == "mlp" else _SwiGLUFFNFused(dim, int(dim * mlp_ratio))
        self.ls2 = _LayerScale(dim, init_values)


# ---- what the block executor reads (attn.qkv / attn.proj / mlp.fc1 / mlp.fc2 [/ mlp.fc3] / norm1 / norm2 / ls1 / ls2) ------------------
class _HalfLinear:
    """One half of the fused w12 Linear as the executor's fc1 (half 0: the SiLU side) or fc3 (half 1).  ``weight`` / ``bias`` are row slices
    of the parameters: views that share their storage and version counter, so the engine's weight images (keyed on the tensor object,
    stamped with its version and address) follow ``load_state_dict``.  The views are rebuilt when the parameter's storage moves."""

    def __init__(self, lin, half):
        self._lin, self._half, self._at, self._w, self._b = lin, half, None, None, None

    def _views(self):
        w = self._lin.weight
        at = (w.data_ptr(), w.device)
        if self._at != at:
            h = w.shape[0] // 2
            lo, hi = self._half * h, (self._half + 1) * h
            self._w, self._b, self._at = w.detach()[lo:hi], self._lin.bias.detach()[lo:hi], at
        return self._w, self._b

    @property
    def weight(self):
        return self._views()[0]

    @property
    def bias(self):
        return self._views()[1]


class _SwiGLUView:
    def __init__(self, mlp):
        self.fc1, self.fc3, self.fc2 = _HalfLinear(mlp.w12, 0), _HalfLinear(mlp.w12, 1), mlp.w3
        self.hidden_features = mlp.w3.in_features


class _MlpView:
    def __init__(self, mlp):
        self.fc1, self.fc2 = mlp.fc1, mlp.fc2
        self.hidden_features = mlp.fc1.out_features


class _BlockView:
    def __init__(self, blk):
        self._blk = blk
        self.norm1, self.norm2, self.attn = blk.norm1, blk.norm2, blk.attn
        self.mlp = _MlpView(blk.mlp) if isinstance(blk.mlp, _Mlp) else _SwiGLUView(blk.mlp)

    @property
    def ls1(self):          # LayerScale gammas, f32 (D): FourMEngine.encoder_block_fwd hands them to the residual sums
        return self._blk.ls1.gamma

    @property
    def ls2(self):
        return self._blk.ls2.gamma


class _ExecView:
    """The tower as the block executor sees it (fourm.vq.engine._VitEngine): ``blocks`` are the views above."""

    def __init__(self, vit):
        self._vit = vit
        self.blocks = [_BlockView(b) for b in vit.blocks]
        self.dim_tokens = vit.embed_dim

    @property
    def compute_precision(self):
        return self._vit.compute_precision


def _engine(vit):
    """The block executor of this tower: one per (device, precision), rebuilt when either changes (scratch and weight images of the other go)."""
    eng = vit.__dict__.get("_hip_engine")
    dev = vit.cls_token.device
    if eng is None or eng.device != dev or eng.precision != vit.compute_precision:
        if dev.type != "cuda":
            raise RuntimeError("DINOv2's vision tower computes on an MI355X through libfourm_hip.so; move it to the GPU first (there is no CPU path)")
        from fourm.vq.engine import _VitEngine
        eng = vit.__dict__["_hip_engine"] = _VitEngine(vit.__dict__["_exec"])
        if vit.ffn_layer != "mlp":
            eng.gated, eng.act = True, "silu"          # w12's halves run as fc1 / fc3 of FM_EPI_SWIGLU (FourMEngine._mlp_fwd)
    eng.prepare()
    return eng


def position_table(pos_embed, gh, gw, antialias=False, offset=0.1):
    """(1 + gh * gw, D) float64 position rows for a (gh, gw) patch grid from the (1, 1 + M * M, D) table: the table itself when gh == gw == M;
    otherwise the class row unchanged and the patch rows F.interpolate of the (1, D, M, M) table, bicubic, in float64 on the host - called
    with scale_factor=((gh + offset) / M, (gw + offset) / M) when the offset is non-zero, with size=(gh, gw) when it is zero."""
    src = pos_embed.detach().double().cpu()[0]
    n, D = src.shape[0] - 1, src.shape[1]
    M = int(round(n ** 0.5))
    if M * M != n:
        raise ValueError(f"position table with {n} patch rows is not square")
    if gh * gw == n and gh == gw:
        return src.contiguous()
    grid = src[1:].reshape(1, M, M, D).permute(0, 3, 1, 2)
    if offset:
        kw = dict(scale_factor=(float(gh + offset) / M, float(gw + offset) / M))
    else:
        kw = dict(size=(gh, gw))
    grid = F.interpolate(grid, mode="bicubic", antialias=bool(antialias), **kw)
    if tuple(grid.shape[-2:]) != (gh, gw):
        raise RuntimeError(f"position table resized to {tuple(grid.shape[-2:])}, expected {(gh, gw)}")
    return torch.cat([src[:1], grid.permute(0, 2, 3, 1).reshape(gh * gw, D)], dim=0).contiguous()


class DinoVisionTransformer(nn.Module):
    def __init__(self, img_size=518, patch_size=14, in_chans=3, embed_dim=768, depth=12, num_heads=12, mlp_ratio=4.0, ffn_layer="mlp",
                 init_values=1.0, num_register_tokens=0, interpolate_antialias=False, interpolate_offset=0.1):
        super().__init__()
        if num_heads <= 0 or embed_dim % num_heads or embed_dim // num_heads != HEAD_DIM:
            raise NotImplementedError(f"width {embed_dim} with {num_heads} heads: the HIP attention kernels are built for head_dim {HEAD_DIM}")
        if ffn_layer not in ("mlp", "swiglufused"):
            raise NotImplementedError(f"ffn_layer {ffn_layer!r}: 'mlp' or 'swiglufused'")
        if init_values is None:
            raise NotImplementedError("DINOv2 blocks carry LayerScale: init_values is a number")
        if depth < 1 or num_register_tokens < 0:
            raise ValueError("depth >= 1 and num_register_tokens >= 0 expected")
        self.embed_dim = self.num_features = embed_dim
        self.patch_size, self.img_size, self.n_blocks, self.num_heads, self.ffn_layer = patch_size, img_size, depth, num_heads, ffn_layer
        self.num_register_tokens, self.interpolate_antialias, self.interpolate_offset = num_register_tokens, interpolate_antialias, interpolate_offset
        self.patch_embed = _PatchEmbed(patch_size, in_chans, embed_dim)
        M = img_size // patch_size
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.pos_embed = nn.Parameter(torch.zeros(1, 1 + M * M, embed_dim))
        if num_register_tokens:
            self.register_tokens = nn.Parameter(torch.zeros(1, num_register_tokens, embed_dim))
        self.blocks = nn.ModuleList([_Block(embed_dim, num_heads, mlp_ratio, ffn_layer, init_values) for _ in range(depth)])
        self.norm = nn.LayerNorm(embed_dim, eps=LN_EPS)
        self.head = nn.Identity()
        self.mask_token = nn.Parameter(torch.zeros(1, embed_dim))          # held for the state dict; masked (iBOT) inputs are refused
        hidden = self.blocks[0].mlp.w3.in_features if ffn_layer != "mlp" else self.blocks[0].mlp.fc1.out_features
        if hidden % 64:
            raise NotImplementedError(f"hidden width {hidden}: the MLP epilogues with a bias run on whole 64-column groups")
        nn.init.trunc_normal_(self.pos_embed, std=0.02)
        nn.init.normal_(self.cls_token, std=1e-6)
        if num_register_tokens:
            nn.init.normal_(self.register_tokens, std=1e-6)
        self.__dict__["_exec"] = _ExecView(self)
        self.__dict__["_tables"] = {}

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

    @property
    def batch_invariant(self) -> bool:
        """True (default): every bf16 GEMM of the tower runs on ONE kernel and tile configuration (fourm.hip.ops.fixed_tiling), so an image's
        features are the same bits in any batch - the tokens a pre-tokenization run writes do not depend on how the images were batched.  False:
        the GEMMs pick their kernel from the shape (few-row, split-K and large-tile routes): faster on large batches (tools/time_dinov2.py
        measures both), a row's low bits then depend on the batch it came in.  Every other kernel of the path is row- or sample-local."""
        return self.__dict__.get("_batch_invariant", True)

    @batch_invariant.setter
    def batch_invariant(self, value: bool):
        self.__dict__["_batch_invariant"] = bool(value)

    @classmethod
    def from_upstream(cls, module: nn.Module) -> "DinoVisionTransformer":
        """Adopt a loaded tower (the hub module, or any module with its state dict and interpolation attributes): same sizes, the weights as
        fp32 copies on the module's device, eval mode."""
        sd = module.state_dict()
        vit = build_dinov2(sd, interpolate_antialias=getattr(module, "interpolate_antialias", False),
                           interpolate_offset=getattr(module, "interpolate_offset", 0.1))
        return vit.to(sd["cls_token"].device)

    # ---- forward ------------------------------------------------------------------------------------------------------------------
    def _check(self, x, masks):
        if masks is not None:
            raise NotImplementedError("masks: masked (iBOT) inputs are out of scope of the HIP tower (mask_token is held, never used)")
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            raise NotImplementedError("DINOv2's vision tower runs at inference only on the HIP engine (no backward): call under torch.no_grad() "
                                      "or freeze it with requires_grad_(False)")
        C, P = self.patch_embed.proj.in_channels, self.patch_size
        if x.dim() != 4 or x.shape[1] != C:
            raise ValueError(f"expected images (B, {C}, H, W), got {tuple(x.shape)}")
        if x.shape[2] % P or x.shape[3] % P or x.shape[2] < P or x.shape[3] < P:
            raise ValueError(f"image size {x.shape[2]}x{x.shape[3]} must be divisible by the patch size {P}")
        eng = _engine(self)
        if x.device != eng.device:
            raise RuntimeError(f"input on {x.device}, model on {eng.device}")
        return eng

    def forward_features(self, x, masks=None):
        eng = self._check(x, masks)
        from fourm.hip import ops
        with torch.no_grad(), ops.fixed_tiling(self.batch_invariant):
            (stream,), (B, T) = self._run(eng, x, [self.n_blocks - 1])
            normed = self._final_norm(stream, B * T).view(B, T, self.embed_dim)
        Rn = self.num_register_tokens
        return {"x_norm_clstoken": normed[:, 0], "x_norm_regtokens": normed[:, 1:1 + Rn], "x_norm_patchtokens": normed[:, 1 + Rn:],
                "x_prenorm": stream.view(B, T, self.embed_dim), "masks": None}

    def forward(self, x, masks=None, is_training=False):
        ret = self.forward_features(x, masks)
        return ret if is_training else self.head(ret["x_norm_clstoken"])

    def get_intermediate_layers(self, x, n=1, reshape=False, return_class_token=False, norm=True):
        """The residual streams after the last ``n`` blocks (or after the blocks listed in ``n``), as the package returns them: patch tokens
        (B, G, D) - (B, D, gh, gw) with ``reshape`` - optionally paired with the class tokens; ``norm`` applies the final LayerNorm."""
        eng = self._check(x, None)
        take = list(range(self.n_blocks - n, self.n_blocks)) if isinstance(n, int) else sorted(int(i) for i in n)
        if not take or take[0] < 0 or take[-1] >= self.n_blocks or len(set(take)) != len(take):
            raise ValueError(f"get_intermediate_layers: blocks {take} of {self.n_blocks}")
        from fourm.hip import ops
        with torch.no_grad(), ops.fixed_tiling(self.batch_invariant):
            streams, (B, T) = self._run(eng, x, take)
            outs = [(self._final_norm(s, B * T) if norm else s).view(B, T, self.embed_dim) for s in streams]
        cls = [o[:, 0] for o in outs]
        outs = [o[:, 1 + self.num_register_tokens:] for o in outs]
        if reshape:
            gh, gw = x.shape[2] // self.patch_size, x.shape[3] // self.patch_size
            outs = [o.reshape(B, gh, gw, -1).permute(0, 3, 1, 2).contiguous() for o in outs]
        return tuple(zip(outs, cls)) if return_class_token else tuple(outs)

    def _final_norm(self, rows, R):
        from fourm.hip import ops
        out = torch.empty(R, self.embed_dim, dtype=torch.float32, device=rows.device)
        ops.layernorm_fwd(rows, self.norm.weight, self.norm.bias, out, eps=self.norm.eps, R=R)
        return out

    def _run(self, eng, x, taps):
        """Images -> copies of the fp32 residual stream (B * T, D) after the blocks in ``taps`` (ascending), and (B, T)."""
        from fourm.hip import _lib as L
        from fourm.hip import ops
        from fourm.hip.engine import ru
        f32, bf = torch.float32, torch.bfloat16
        ws, D, P = eng.ws, self.embed_dim, self.patch_size
        B, C, H, W = x.shape
        gh, gw = H // P, W // P
        G, Rn = gh * gw, self.num_register_tokens
        T = 1 + Rn + G
        Rg, R, feat = B * G, B * T, C * P * P
        Rp, Rgp = ru(R, 128), ru(Rg, 128)
        x = x.float().contiguous()
        proj = self.patch_embed.proj
        if eng.fp32:
            rows = ws.get("dino.patches32", (Rgp, feat), f32)
            rows[:Rg].view(B, gh, gw, C, P, P).copy_(x.view(B, C, gh, P, gw, P).permute(0, 2, 4, 1, 3, 5))        # (plumbing)
            patches = ws.get("dino.proj32", (Rgp, D), f32)
            ops.gemm_nt(rows, eng.w(proj.weight), patches, epilogue=L.EPI_F32, bias=proj.bias, M=Rg, N=D, K=feat)
        else:
            rows = ws.get("dino.patches", (Rgp, ru(feat, 64)), bf)          # (the pad columns are never written: they stay zero)
            L.check(L.vq_patchify(ops._p(x), ops._p(rows), rows.stride(0), B, C, H, W, P, ops._stream()))
            patches = ws.get("dino.proj", (Rgp, D), bf)
            ops.gemm_nt(rows, eng.w(proj.weight), patches, bias=proj.bias, M=Rg, N=D, K=ru(feat, 64))
        pos = self._pos_table(gh, gw, x.device)
        stream = ws.get("dino.x0", (Rp, D), f32)
        ops.cls_pos_embed(patches, self.cls_token, self.register_tokens[0] if Rn else None, pos, stream, B, G, D)
        none = dict(mask_kind=L.MASK_NONE)
        top, out, views = taps[-1], {}, self.__dict__["_exec"].blocks
        for i in range(top + 1):
            # (the last residual sum of every block but the top one is left to the next block's norm1: fm_layernorm_fwd_res_ls)
            nxt = eng.encoder_block_fwd(views[i], stream, B, T, none, None, f"dino{i % 2}", defer_out=i < top)
            if i - 1 in taps:                                        # block i's norm1 has written the stream after block i - 1
                out[i - 1] = stream[:R].clone()
            stream = nxt
        eng._settle()
        out[top] = stream[:R].clone()
        return [out[t] for t in taps], (B, T)

    def _pos_table(self, gh, gw, device):
        """(1 + gh * gw, D) fp32 position rows of a patch grid on the device: float64 on the host (position_table), rounded to fp32 once,
        cached per grid and parameter version.  Tables of an OLDER parameter version are dropped; the other grids' tables of this version stay
        (a table is never freed under a launch that may still read it, cf. fourm/vq/engine.py::_pos_rows)."""
        pe = self.pos_embed
        key = ("pos", gh, gw, pe._version, pe.data_ptr(), str(device))
        t = self._tables.get(key)
        if t is None:
            t = position_table(pe, gh, gw, self.interpolate_antialias, self.interpolate_offset).float().contiguous()
            for k in [k for k in self._tables if k[0] == "pos" and k[3:5] != key[3:5]]:
                del self._tables[k]
            t = self._tables[key] = t.to(device)
            if device.type == "cuda":
                torch.cuda.current_stream(device).synchronize()
        return t

    def interpolate_pos_encoding(self, x, w, h):
        """The package's helper, kept for callers: the (1, 1 + G, D) table for an image of height ``w`` and width ``h`` (its names)."""
        return self._pos_table(w // self.patch_size, h // self.patch_size, self.pos_embed.device).unsqueeze(0)


def _hub(embed_dim, depth, num_heads, ffn_layer, patch_size=14, img_size=518, **kwargs):
    return DinoVisionTransformer(img_size=img_size, patch_size=patch_size, embed_dim=embed_dim, depth=depth, num_heads=num_heads, mlp_ratio=4,
                                 ffn_layer=ffn_layer, **kwargs)


REG4 = dict(num_register_tokens=4, interpolate_antialias=True, interpolate_offset=0.0)
vit_small = partial(_hub, 384, 12, 6, "mlp")
vit_base = partial(_hub, 768, 12, 12, "mlp")
vit_large = partial(_hub, 1024, 24, 16, "mlp")
vit_giant2 = partial(_hub, 1536, 40, 24, "swiglufused")
vit_small_reg4, vit_base_reg4 = partial(vit_small, **REG4), partial(vit_base, **REG4)
vit_large_reg4, vit_giant2_reg4 = partial(vit_large, **REG4), partial(vit_giant2, **REG4)


def build_dinov2(state_dict: dict, interpolate_antialias=None, interpolate_offset=None) -> DinoVisionTransformer:
    """The tower of a DINOv2 state dict: every size is read off the tensors (width, depth, patch size, native grid, registers, FFN kind).
    The two interpolation settings are not in a state dict: by default a dict with registers gets the ``_reg4`` settings (antialias, offset 0),
    one without the plain ones (no antialias, offset 0.1), as the hub configurations pair them.  Half-precision dicts load as fp32 masters."""
    if "cls_token" not in state_dict or "patch_embed.proj.weight" not in state_dict or "blocks.0.ls1.gamma" not in state_dict:
        raise NotImplementedError("not a DINOv2 state dict (cls_token, patch_embed.proj.weight and blocks.0.ls1.gamma expected)")
    w = state_dict["patch_embed.proj.weight"]
    D, C, P = w.shape[0], w.shape[1], w.shape[-1]
    depth = len([k for k in state_dict if k.endswith(".attn.qkv.weight")])
    M = int(round((state_dict["pos_embed"].shape[1] - 1) ** 0.5))
    reg = state_dict["register_tokens"].shape[1] if "register_tokens" in state_dict else 0
    ffn = "swiglufused" if "blocks.0.mlp.w12.weight" in state_dict else "mlp"
    ratio = 4.0 if ffn != "mlp" else state_dict["blocks.0.mlp.fc1.weight"].shape[0] / D
    vit = DinoVisionTransformer(img_size=M * P, patch_size=P, in_chans=C, embed_dim=D, depth=depth, num_heads=D // HEAD_DIM, mlp_ratio=ratio,
                                ffn_layer=ffn, num_register_tokens=reg,
                                interpolate_antialias=bool(reg) if interpolate_antialias is None else interpolate_antialias,
                                interpolate_offset=(0.0 if reg else 0.1) if interpolate_offset is None else interpolate_offset)
    vit.load_state_dict({k: v.detach().float() for k, v in state_dict.items()}, strict=True)
    return vit.eval().requires_grad_(False)
