"""``PatchedUNetCondCat`` / ``unet_patched``: the conditional UNet behind the DiVAE detokenizers, inference on gfx950.

API of upstream ``fourm/vq/models/unet/unet.py`` (UNetModel :411-690, PatchedUNetCondCat :693-744, unet_patched :747-754): same
constructor arguments, same parameter tree (``time_embed.{0,2}``, ``input_blocks.i.j.{in_layers.0|in_layers.2|emb_layers.1|
out_layers.0|out_layers.3|skip_connection|norm|qkv|proj_out|op}``, ``middle_block.k``, ``output_blocks.i.j.(...|conv)``, ``out.{0,2}``:
upstream checkpoints load with strict=True), same ``forward(sample, timestep, encoder_hidden_states, cond_mask=None)``.

The torch modules below only HOLD the parameters; the forward runs on the HIP kernels (csrc/unet.hip + the NT GEMMs): feature maps as
(B * H * W, C) bf16 rows, every convolution a GEMM (3 x 3 through fm_unet_im2col), GroupNorm + SiLU in fp32 arithmetic, bf16 GEMM operands
with fp32 accumulation = upstream's autocast arithmetic.  The bf16 path is inference only (no bf16 backward).
``compute_precision = "fp32"`` (a plain attribute, set after construction like ``FourM.compute_precision``) runs the same launch sequence with
f32 feature maps and f32 master weights on csrc/unet_f32.hip + fm_gemm_f32: upstream's fp32 evaluation, for verification (_UNetEngineF32).
In that mode, in training mode with gradients enabled and a trainable parameter, the evaluation is differentiable with respect to the
PARAMETERS (_UNetTrainF32 on csrc/unet_f32_bwd.hip: the decoder trained on a frozen encoder).  The verification-mode backward: no throughput
claim, no gradient to the sample or the conditioning, square inputs only, not graph-capturable.
Not implemented (rejected loudly): class conditioning, scale-shift norm, ResBlock up / down sampling, the new attention order, dropout."""
import math
from typing import Optional, Union

import torch
import torch.nn as nn

from fourm.hip import _lib as L
from fourm.hip import ops


import os

# 3 x 3 convolutions with C % 64 == 0 input channels as implicit GEMMs (no im2col round trip; bit-identical).  FOURM_UNET_IMPLICIT_CONV=0: im2col + GEMM.
IMPLICIT_CONV = os.environ.get("FOURM_UNET_IMPLICIT_CONV", "1") == "1"


# One evaluation = ~430 launches issued from Python: at batch 8 the host needs 8.3 ms to enqueue what the GPU runs in ~6.5 ms (tools/divae_host_probe.py).
# In eval mode the launch sequence of a (shape, stream) is captured into a hipGraph after two eager evaluations and replayed from then on
# (inputs copied into static buffers, the output copied out).  FOURM_UNET_GRAPH=0: always eager.
UNET_GRAPH = os.environ.get("FOURM_UNET_GRAPH", "1") == "1"


def ru(x, m):
    return (x + m - 1) // m * m


class _Res(nn.Module):
    def __init__(self, cin, cout, emb_ch):
        super().__init__()
        self.in_layers = nn.Sequential(nn.GroupNorm(32, cin), nn.SiLU(), nn.Conv2d(cin, cout, 3, padding=1))
        self.emb_layers = nn.Sequential(nn.SiLU(), nn.Linear(emb_ch, cout))
        self.out_layers = nn.Sequential(nn.GroupNorm(32, cout), nn.SiLU(), nn.Dropout(p=0.0), nn.Conv2d(cout, cout, 3, padding=1))
        for p in self.out_layers[3].parameters():
            p.detach().zero_()                                                  # zero_module (unet.py:224-227)
        self.skip_connection = nn.Identity() if cin == cout else nn.Conv2d(cin, cout, 1)
        self.cin, self.cout = cin, cout


class _Attn(nn.Module):
    def __init__(self, ch, heads):
        super().__init__()
        self.norm = nn.GroupNorm(32, ch)
        self.qkv = nn.Conv1d(ch, 3 * ch, 1)
        self.proj_out = nn.Conv1d(ch, ch, 1)
        for p in self.proj_out.parameters():
            p.detach().zero_()
        self.ch, self.heads = ch, heads


class _Down(nn.Module):
    def __init__(self, ch):
        super().__init__()
        self.op = nn.Conv2d(ch, ch, 3, stride=2, padding=1)
        self.ch = ch


class _Up(nn.Module):
    def __init__(self, ch):
        super().__init__()
        self.conv = nn.Conv2d(ch, ch, 3, padding=1)
        self.ch = ch


class PatchedUNetCondCat(nn.Module):
    def __init__(self, in_channels: int, out_channels: int, cond_channels: int, patch_size: int, image_size=224, model_channels=256,
                 num_res_blocks=3, attention_resolutions=(8, 16), dropout=0, channel_mult=(1, 2, 4, 8), conv_resample=True, dims=2, num_classes=None,
                 use_checkpoint=False, num_heads=1, num_head_channels=-1, num_heads_upsample=-1, use_scale_shift_norm=False, resblock_updown=False,
                 use_new_attention_order=False):
        super().__init__()
        if dims != 2 or num_classes is not None or use_scale_shift_norm or resblock_updown or use_new_attention_order or not conv_resample or dropout:
            raise NotImplementedError("PatchedUNetCondCat (HIP): only the options of unet_patched are implemented (2-D, conv resampling, no class "
                                      "conditioning / scale-shift norm / ResBlock resampling / new attention order / dropout)")
        self.P_H = self.P_W = int(patch_size)
        self.in_channels, self.out_channels, self.cond_channels = in_channels, out_channels, cond_channels
        self.image_size = self.sample_size = image_size
        self.model_channels, self.num_res_blocks, self.channel_mult = model_channels, num_res_blocks, tuple(channel_mult)
        self.attention_resolutions = tuple(attention_resolutions)
        in_p, out_p = in_channels * patch_size * patch_size + cond_channels, out_channels * patch_size * patch_size
        te = model_channels * 4
        heads = lambda c: num_heads if num_head_channels == -1 else c // num_head_channels
        self.time_embed = nn.Sequential(nn.Linear(model_channels, te), nn.SiLU(), nn.Linear(te, te))
        ch = int(channel_mult[0] * model_channels)
        self.input_blocks = nn.ModuleList([nn.Sequential(nn.Conv2d(in_p, ch, 3, padding=1))])
        chans, ds = [ch], 1
        for level, mult in enumerate(channel_mult):
            for _ in range(num_res_blocks):
                layers = [_Res(ch, int(mult * model_channels), te)]
                ch = int(mult * model_channels)
                if ds in self.attention_resolutions:
                    layers.append(_Attn(ch, heads(ch)))
                self.input_blocks.append(nn.Sequential(*layers))
                chans.append(ch)
            if level != len(channel_mult) - 1:
                self.input_blocks.append(nn.Sequential(_Down(ch)))
                chans.append(ch)
                ds *= 2
        self.middle_block = nn.Sequential(_Res(ch, ch, te), _Attn(ch, heads(ch)), _Res(ch, ch, te))
        self.output_blocks = nn.ModuleList([])
        up_heads = (lambda c: num_heads_upsample if num_head_channels == -1 else c // num_head_channels) if num_heads_upsample != -1 else heads
        for level, mult in list(enumerate(channel_mult))[::-1]:
            for i in range(num_res_blocks + 1):
                layers = [_Res(ch + chans.pop(), int(model_channels * mult), te)]
                ch = int(model_channels * mult)
                if ds in self.attention_resolutions:
                    layers.append(_Attn(ch, up_heads(ch)))
                if level and i == num_res_blocks:
                    layers.append(_Up(ch))
                    ds //= 2
                self.output_blocks.append(nn.Sequential(*layers))
        self.out = nn.Sequential(nn.GroupNorm(32, ch), nn.SiLU(), nn.Conv2d(ch, out_p, 3, padding=1))
        for p in self.out[2].parameters():
            p.detach().zero_()
        self._engine = None
        self._train_engine = None                       # _UNetTrainF32, built at the first differentiable evaluation
        # "bf16" = the hot path (autocast arithmetic); "fp32" = f32 feature maps and weights on the plain kernels of csrc/unet_f32.hip.
        # Read at every evaluation; the FOURM_PRECISION environment variable is NOT consulted here (it belongs to the trunk).
        self.compute_precision = "bf16"

    @property
    def device(self):
        return next(self.parameters()).device

    @property
    def dtype(self):
        return next(self.parameters()).dtype

    def forward(self, sample: torch.Tensor, timestep: Union[torch.Tensor, float, int], encoder_hidden_states: torch.Tensor = None,
                cond_mask: Optional[torch.Tensor] = None, **kwargs) -> torch.Tensor:
        """sample (B, C, H, W); timestep: number or (B,) / (1,) tensor; encoder_hidden_states (B, D, Hc, Wc): the de-quantised latents;
        cond_mask (B, Hc, Wc) bool, True = that conditioning vector is zeroed (unet.py:727-729).  Returns f32 (B, out_channels, H, W).

        With ``compute_precision == "fp32"``, in training mode, with gradients enabled and at least one parameter that requires a gradient, the
        result carries a ``grad_fn``: its backward adds the gradient of every trainable parameter to ``.grad`` (torch semantics) on the kernels of
        csrc/unet_f32_bwd.hip.  The values are bit-identical to the eval-mode fp32 evaluation.  Scope: the decoder on a frozen encoder - the inputs
        get no gradient (a sample or conditioning that requires one is refused), no bf16 backward, square inputs, no graph capture.  Every other
        combination evaluates without a gradient path, as before."""
        prec = self.compute_precision
        if prec not in ("bf16", "fp32"):
            raise ValueError(f"compute_precision {prec!r}: 'bf16' or 'fp32'")
        if not sample.is_cuda:
            raise RuntimeError("PatchedUNetCondCat runs on the HIP kernels only: move the model and its inputs to an MI355X (there is no CPU path)")
        if prec == "fp32" and self.training and torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            if sample.requires_grad or (torch.is_tensor(encoder_hidden_states) and encoder_hidden_states.requires_grad):
                raise NotImplementedError("PatchedUNetCondCat: the backward is built for the frozen-encoder scope (parameter gradients only): the sample "
                                          "and the conditioning get no gradient - detach them")
            if self._train_engine is None:
                self._train_engine = _UNetTrainF32(self)
            anchor = next(p for p in self.parameters() if p.requires_grad)
            return _UNetTrainStep.apply(anchor, self._train_engine, sample, timestep, encoder_hidden_states, cond_mask)
        with torch.no_grad():
            return self._evaluate(prec, sample, timestep, encoder_hidden_states, cond_mask)

    def _evaluate(self, prec, sample, timestep, encoder_hidden_states, cond_mask):
        if self._engine is None or self._engine.precision != prec:
            # (a new engine: the weight images, scratch and captured graphs of the other precision go with the old one)
            self._engine = (_UNetEngineF32 if prec == "fp32" else _UNetEngine)(self)
        if prec == "fp32":                                       # always eager: the verification mode has no use for graph replay
            return self._engine.forward(sample, timestep, encoder_hidden_states, cond_mask)
        if UNET_GRAPH and not self.training and not torch.cuda.is_current_stream_capturing():
            return self._engine.forward_graphed(sample, timestep, encoder_hidden_states, cond_mask)
        return self._engine.forward(sample, timestep, encoder_hidden_states, cond_mask)


def unet_patched(**kwargs):
    return PatchedUNetCondCat(patch_size=4, model_channels=256, num_res_blocks=3, attention_resolutions=[4, 8], channel_mult=(1, 2, 2, 2), **kwargs)


class _UNetEngine:
    """Launch sequence of one UNet evaluation.  bf16 weight images are cached per parameter (refreshed when the parameter changed)."""
    precision = "bf16"

    def __init__(self, net: PatchedUNetCondCat):
        self.net = net
        self._w, self._buf = {}, {}
        res = [m for m in net.modules() if isinstance(m, _Res)]
        self._res_index = {id(m): i for i, m in enumerate(res)}
        self._res = res
        offs, o = [], 0
        for m in res:
            offs.append(o)
            o += ru(m.cout, 4)
        self._emb_off, self._emb_total = offs, ru(o, 64)

    # ---- cached operands -------------------------------------------------------------------------------------------------------------
    def _stamp(self, *ps):
        return tuple((p._version, p.data_ptr()) for p in ps)

    def w_conv(self, conv):
        """(Cout, k * k * Cin padded to 64) bf16: conv.weight with the taps outermost, the GEMM's W operand behind fm_unet_im2col."""
        w = conv.weight
        key = ("w", id(w), self.precision)
        hit = self._w.get(key)
        if hit is None or hit[0] != self._stamp(w):
            co = w.shape[0]
            flat = (w.detach().permute(0, 2, 3, 1) if w.dim() == 4 else w.detach().permute(0, 2, 1)).reshape(co, -1).float().contiguous()
            K = flat.shape[1]
            img = torch.zeros(co, ru(K, 64), dtype=torch.bfloat16, device=w.device)
            tmp = torch.empty(co * K, dtype=torch.bfloat16, device=w.device)
            ops.f32_to_bf16(flat, tmp)
            img[:, :K] = tmp.view(co, K)
            hit = self._w[key] = (self._stamp(w), img)
        return hit[1]

    def w_emb_all(self):
        """Every ResBlock's emb_layers Linear stacked into one (sum Cout, 4 mc) operand + bias: ONE GEMM per evaluation gives all the
        per-block timestep embeddings (the input silu(emb) is the same for all of them)."""
        ps = [p for m in self._res for p in (m.emb_layers[1].weight, m.emb_layers[1].bias)]
        key = ("emb_all", self.precision)
        hit = self._w.get(key)
        if hit is None or hit[0] != self._stamp(*ps):
            te = self._res[0].emb_layers[1].weight.shape[1]
            dev = ps[0].device
            wf = torch.zeros(self._emb_total, te, dtype=torch.float32, device=dev)
            bf = torch.zeros(self._emb_total, dtype=torch.float32, device=dev)
            for m, o in zip(self._res, self._emb_off):
                wf[o:o + m.cout] = m.emb_layers[1].weight.detach()
                bf[o:o + m.cout] = m.emb_layers[1].bias.detach()
            hit = self._w[key] = (self._stamp(*ps), self._emb_image(wf), bf)
        return hit[1], hit[2]

    def _emb_image(self, wf):
        img = torch.empty(wf.shape, dtype=torch.bfloat16, device=wf.device)
        ops.f32_to_bf16(wf, img)
        return img

    def buf(self, tag, rows, cols, dtype=torch.bfloat16):
        key = (tag, dtype, torch.cuda.current_stream(self.net.device).cuda_stream, ops.SCRATCH_TAG)      # one scratch set per stream / per captured graph
        b = self._buf.get(key)
        n = rows * cols
        if b is None or b.numel() < n or b.device != self.net.device:
            b = self._buf[key] = torch.empty(max(n, 1), dtype=dtype, device=self.net.device)
        return b[:n].view(rows, cols)

    # ---- building blocks -------------------------------------------------------------------------------------------------------------
    def gemm(self, x, w, bias, out, M, N, K, f32_out=False):
        ops.gemm_nt(x, w, out, epilogue=L.EPI_F32 if f32_out else L.EPI_BF16, bias=bias.detach().float().contiguous() if bias is not None else None, M=M, N=N, K=K)
        return out

    def im2col(self, tag, src1, C1, B, H, W, ksize=3, stride=1, up1=0, src2=None, C2=0, H2=0, W2=0):
        kp = ru(ksize * ksize * (C1 + C2), 64)
        pad = ksize // 2
        Ho, Wo = (H + 2 * pad - ksize) // stride + 1, (W + 2 * pad - ksize) // stride + 1
        out = self.buf(tag, B * Ho * Wo, kp)
        L.check(L.unet_im2col(ops._p(src1), src1.stride(0), C1, ops._p(src2), src2.stride(0) if src2 is not None else 0, C2, H2, W2, ops._p(out), kp, kp,
                              B, H, W, ksize, stride, up1, ops._stream()))
        return out, Ho, Wo

    def gn(self, tag, x, norm, B, HW, C, silu, add=None):
        y = self.buf(tag, B * HW, C)
        st = self.buf("gn_stats", B * norm.num_groups * ((HW + 31) // 32 + 1), 2, torch.float32)
        L.check(L.groupnorm_nhwc(ops._p(x), x.stride(0), ops._p(add), add.stride(0) if add is not None else 0, ops._p(norm.weight.detach()), ops._p(norm.bias.detach()),
                                 ops._p(y), C, ops._p(st), B, HW, C, norm.num_groups, float(norm.eps), 1 if silu else 0, ops._stream()))
        return y

    def conv3(self, tag, x, conv, B, H, W, stride=1, up1=0, out=None, f32_out=False):
        """3 x 3 convolution (padding 1) of the (B, H >> up1, W >> up1, C) rows x read on the (H, W) grid.  C % 64 == 0: implicit GEMM (the gather runs
        inside the GEMM's LDS-DMA addresses, fm_gemm_nt_args.conv_*); else fm_unet_im2col + the plain GEMM."""
        C, Co = conv.weight.shape[1], conv.weight.shape[0]
        Ho, Wo = (H + 2 - 3) // stride + 1, (W + 2 - 3) // stride + 1
        if out is None:
            out = self.buf(tag, B * Ho * Wo, Co)
        if IMPLICIT_CONV and C % 64 == 0:
            ops.gemm_nt(x, self.w_conv(conv), out, epilogue=L.EPI_F32 if f32_out else L.EPI_BF16, bias=conv.bias.detach().float().contiguous() if conv.bias is not None else None,
                        M=B * Ho * Wo, N=Co, K=9 * C, conv=dict(C=C, H=H, W=W, Ho=Ho, Wo=Wo, stride=stride, up=up1))
            return out, Ho, Wo
        col, Ho, Wo = self.im2col("col", x, C, B, H, W, 3, stride, up1)
        self.gemm(col, self.w_conv(conv), conv.bias, out, B * Ho * Wo, Co, col.shape[1], f32_out=f32_out)
        return out, Ho, Wo

    def res(self, tag, m, x, emb_all, B, H, W):
        R = B * H * W
        a = self.gn("act", x, m.in_layers[0], B, H * W, m.cin, True)
        h, _, _ = self.conv3("h1", a, m.in_layers[2], B, H, W)
        o = self._emb_off[self._res_index[id(m)]]
        a2 = self.gn("act", h, m.out_layers[0], B, H * W, m.cout, True, add=emb_all[:, o:o + m.cout])
        h2, _, _ = self.conv3("h2", a2, m.out_layers[3], B, H, W)
        if isinstance(m.skip_connection, nn.Identity):
            xs = x
        else:
            xs = self.buf("skipc", R, m.cout)
            xin = x
            if m.cin % 64:                           # the GEMM reduces over whole 64-column groups: zero-padded copy of the rows
                xin, _, _ = self.im2col("col", x, m.cin, B, H, W, ksize=1)
            self.gemm(xin, self.w_conv(m.skip_connection), m.skip_connection.bias, xs, R, m.cout, ru(m.cin, 64))
        out = torch.empty(R, m.cout, dtype=torch.bfloat16, device=x.device)
        L.check(L.add_bf16(ops._p(xs), xs.stride(0), ops._p(h2), h2.stride(0), ops._p(out), m.cout, R, m.cout, ops._stream()))
        return out

    def attn(self, m, x, B, H, W):
        T, C = H * W, m.ch
        n = self.gn("act", x, m.norm, B, T, C, False)
        qkv = self.buf("qkv", B * T, 3 * C)
        nin = n
        if C % 64:
            nin, _, _ = self.im2col("col", n, C, B, H, W, ksize=1)
        self.gemm(nin, self.w_conv(m.qkv), m.qkv.bias, qkv, B * T, 3 * C, ru(C, 64))
        a = self.buf("attn_o", B * T, ru(C, 64))
        if C % 64:
            a.zero_()
        L.check(L.unet_attention(ops._p(qkv), 3 * C, ops._p(a), a.stride(0), B, T, m.heads, C // m.heads, ops._stream()))
        pr = self.buf("h2", B * T, C)
        self.gemm(a, self.w_conv(m.proj_out), m.proj_out.bias, pr, B * T, C, ru(C, 64))
        out = torch.empty(B * T, C, dtype=torch.bfloat16, device=x.device)
        L.check(L.add_bf16(ops._p(x), x.stride(0), ops._p(pr), C, ops._p(out), C, B * T, C, ops._stream()))
        return out

    def run(self, seq, h, emb_all, B, H, W):
        for m in seq:
            if isinstance(m, _Res):
                h = self.res("r", m, h, emb_all, B, H, W)
            elif isinstance(m, _Attn):
                h = self.attn(m, h, B, H, W)
            elif isinstance(m, _Down):
                o, H, W = self.conv3("down", h, m.op, B, H, W, stride=2)
                h = o.clone()
            elif isinstance(m, _Up):
                o, H, W = self.conv3("up", h, m.conv, B, 2 * H, 2 * W, up1=1)
                h = o.clone()
            else:
                raise TypeError(type(m))
        return h, H, W

    # ---- one evaluation, replayed from a hipGraph ----------------------------------------------------------------------------------
    def _weights_stamp(self):
        return tuple((p._version, p.data_ptr()) for p in self.net.parameters())

    def forward_graphed(self, sample, timestep, cond, cond_mask):
        """forward() through a captured graph per (shapes, mask or not, stream).  The first two evaluations of a key run eagerly (they build the
        cached weight images and size every scratch buffer); the third is captured.  A parameter that changed (version / storage) drops the graphs."""
        dev = sample.device
        key = (self.precision, tuple(sample.shape), tuple(cond.shape), cond_mask is not None, torch.cuda.current_stream(dev).cuda_stream)
        stamp = self._weights_stamp()
        if getattr(self, "_graph_stamp", None) != stamp:
            self._graphs, self._graph_warm, self._graph_stamp = {}, {}, stamp
        g = self._graphs.get(key)
        if g is None:
            n = self._graph_warm.get(key, 0)
            if n < 2:
                self._graph_warm[key] = n + 1
                return self.forward(sample, timestep, cond, cond_mask)
            B = sample.shape[0]
            st = dict(x=sample.detach().float().contiguous().clone(), t=torch.zeros(B, dtype=torch.float32, device=dev), c=cond.detach().float().contiguous().clone(),
                      m=cond_mask.to(dev).clone() if cond_mask is not None else None)
            torch.cuda.current_stream(dev).synchronize()
            graph = torch.cuda.CUDAGraph()
            ops.SCRATCH_TAG = ("graph", len(self._graphs), key)          # scratch allocated during the capture lives in this graph's pool and is its alone
            try:
                with torch.cuda.graph(graph):
                    st["out"] = self.forward(st["x"], st["t"], st["c"], st["m"])
            finally:
                ops.SCRATCH_TAG = None
            while len(self._graphs) >= 6:                      # (a graph keeps its scratch: bound what a stream of changing shapes can pile up)
                self._graphs.pop(next(iter(self._graphs)))
            g = self._graphs[key] = (graph, st)
        graph, st = g
        st["x"].copy_(sample.detach())
        st["c"].copy_(cond.detach())
        if st["m"] is not None:
            st["m"].copy_(cond_mask)
        if torch.is_tensor(timestep):
            st["t"].copy_(timestep.detach().reshape(-1).float().expand(st["t"].shape[0]) if timestep.numel() == 1 else timestep.detach().reshape(-1).float())
        else:
            st["t"].fill_(float(timestep))
        graph.replay()
        return st["out"].clone()

    # ---- one evaluation --------------------------------------------------------------------------------------------------------------
    def forward(self, sample, timestep, cond, cond_mask):
        net = self.net
        dev = sample.device
        B, C, H, W = sample.shape
        P = net.P_H
        if H % P or W % P:
            raise ValueError(f"Image sizes {H}x{W} must be divisible by patch sizes {P}x{P}")
        nh, nw = H // P, W // P
        x32 = sample.detach().float().contiguous()
        CP = C * P * P
        if CP % 8 or net.cond_channels % 8:
            raise NotImplementedError("patch / conditioning widths must be multiples of 8")
        rows = self.buf("patch", B * nh * nw, CP)
        if nh == nw and H == W:
            L.check(L.vq_patchify(ops._p(x32), ops._p(rows), CP, B, C, H, W, P, ops._stream()))
        else:
            raise NotImplementedError("non-square inputs")
        cnd = cond.detach().float()
        if cond_mask is not None:
            cnd = torch.where(cond_mask[:, None].to(dev), torch.zeros((), device=dev), cnd)
        D, Hc, Wc = cnd.shape[1:]
        crow32 = cnd.permute(0, 2, 3, 1).reshape(B * Hc * Wc, D).contiguous()
        crow = self.buf("cond", B * Hc * Wc, D)
        ops.f32_to_bf16(crow32, crow)
        # timestep embedding -> time_embed MLP -> silu -> every ResBlock's projection in one GEMM
        t = torch.as_tensor(timestep, device=dev).reshape(-1).float()
        if t.numel() == 1:
            t = t.expand(B)
        t = t.contiguous()
        mc, te = net.model_channels, net.model_channels * 4
        temb = self.buf("temb", B, ru(mc, 64))
        temb.zero_()
        L.check(L.timestep_embedding(ops._p(t), ops._p(temb), temb.stride(0), B, mc, 10000.0, ops._stream()))
        l0, l2 = net.time_embed[0], net.time_embed[2]
        e1 = self.buf("e1", B, te, torch.float32)
        self.gemm(temb, self.w_conv_lin(l0), l0.bias, e1, B, te, ru(mc, 64), f32_out=True)
        s1 = self.buf("s1", B, te)
        L.check(L.silu_f32_to_bf16(ops._p(e1), ops._p(s1), B * te, ops._stream()))
        e2 = self.buf("e2", B, te, torch.float32)
        self.gemm(s1, self.w_conv_lin(l2), l2.bias, e2, B, te, te, f32_out=True)
        s2 = self.buf("s2", B, te)
        L.check(L.silu_f32_to_bf16(ops._p(e2), ops._p(s2), B * te, ops._stream()))
        wall, ball = self.w_emb_all()
        emb_all = self.buf("emb_all", B, self._emb_total, torch.float32)
        ops.gemm_nt(s2, wall, emb_all, epilogue=L.EPI_F32, bias=ball, M=B, N=self._emb_total, K=te)
        # input blocks
        first = net.input_blocks[0][0]
        col, _, _ = self.im2col("col", rows, CP, B, nh, nw, 3, 1, 0, src2=crow, C2=D, H2=Hc, W2=Wc)
        ch0 = first.weight.shape[0]
        h = torch.empty(B * nh * nw, ch0, dtype=torch.bfloat16, device=dev)
        self.gemm(col, self.w_conv(first), first.bias, h, B * nh * nw, ch0, col.shape[1])
        hs, hh, ww = [(h, nh, nw)], nh, nw
        for blk in list(net.input_blocks)[1:]:
            h, hh, ww = self.run(blk, h, emb_all, B, hh, ww)
            hs.append((h, hh, ww))
        h, hh, ww = self.run(net.middle_block, h, emb_all, B, hh, ww)
        for blk in net.output_blocks:
            skip, sh, sw = hs.pop()
            assert (sh, sw) == (hh, ww)
            C1, C2 = h.shape[1], skip.shape[1]
            cat = torch.empty(B * hh * ww, C1 + C2, dtype=torch.bfloat16, device=dev)
            L.check(L.unet_im2col(ops._p(h), h.stride(0), C1, ops._p(skip), skip.stride(0), C2, hh, ww, ops._p(cat), C1 + C2, C1 + C2, B, hh, ww, 1, 1, 0, ops._stream()))
            h, hh, ww = self.run(blk, cat, emb_all, B, hh, ww)
        a = self.gn("act", h, net.out[0], B, hh * ww, h.shape[1], True)
        conv = net.out[2]
        OP = conv.weight.shape[0]
        y = self.buf("y", B * hh * ww, ru(OP, 4), torch.float32)
        self.conv3("y", a, conv, B, hh, ww, out=y, f32_out=True)
        img = torch.empty(B, net.out_channels, H, W, dtype=torch.float32, device=dev)
        L.check(L.vq_unpatchify(ops._p(y), y.stride(0), ops._p(img), B, net.out_channels, H, W, P, ops._stream()))
        return img

    def w_conv_lin(self, lin):
        w = lin.weight
        key = ("lin", id(w), self.precision)
        hit = self._w.get(key)
        if hit is None or hit[0] != self._stamp(w):
            o, i = w.shape
            img = torch.zeros(o, ru(i, 64), dtype=torch.bfloat16, device=w.device)
            tmp = torch.empty(o, i, dtype=torch.bfloat16, device=w.device)
            ops.f32_to_bf16(w.detach().float().contiguous(), tmp)
            img[:, :i] = tmp
            hit = self._w[key] = (self._stamp(w), img)
        return hit[1]


class _UNetEngineF32(_UNetEngine):
    """The same launch sequence in fp32 (compute_precision = "fp32"): f32 feature maps and scratch, the f32 master weights with the taps outermost
    (no bf16 image, no padding to 64), csrc/unet_f32.hip for everything that is not a GEMM and fm_gemm_f32 for every convolution and Linear
    (a 3 x 3 convolution is always fm_unet_im2col_f32 + that GEMM: the implicit-GEMM and split-K paths belong to the bf16 kernels).  Always
    eager.  Upstream's fp32 evaluation (the UNet outside an autocast context), for verification; not a hot path."""
    precision = "fp32"

    # ---- cached operands -------------------------------------------------------------------------------------------------------------
    def w_conv(self, conv):
        """(Cout, k * k * Cin) f32: conv.weight with the taps outermost, the GEMM's W operand behind fm_unet_im2col_f32."""
        w = conv.weight
        key = ("w", id(w), self.precision)
        hit = self._w.get(key)
        if hit is None or hit[0] != self._stamp(w):
            flat = (w.detach().permute(0, 2, 3, 1) if w.dim() == 4 else w.detach().permute(0, 2, 1)).reshape(w.shape[0], -1).float().contiguous()
            hit = self._w[key] = (self._stamp(w), flat)
        return hit[1]

    def w_conv_lin(self, lin):
        return lin.weight.detach().float().contiguous()                  # (the f32 master itself)

    def _emb_image(self, wf):
        return wf                                                        # (the stacked f32 masters themselves)

    def buf(self, tag, rows, cols, dtype=torch.float32):
        return super().buf(tag, rows, cols, dtype)

    # ---- building blocks -------------------------------------------------------------------------------------------------------------
    def gemm(self, x, w, bias, out, M, N, K):
        ops.gemm_nt(x, w, out, epilogue=L.EPI_F32, bias=bias.detach().float().contiguous() if bias is not None else None, M=M, N=N, K=K)      # f32 operands: fm_gemm_f32
        return out

    def im2col(self, tag, src1, C1, B, H, W, ksize=3, stride=1, up1=0, src2=None, C2=0, H2=0, W2=0):
        kp = ksize * ksize * (C1 + C2)
        pad = ksize // 2
        Ho, Wo = (H + 2 * pad - ksize) // stride + 1, (W + 2 * pad - ksize) // stride + 1
        out = self.buf(tag, B * Ho * Wo, kp)
        L.check(L.unet_im2col_f32(ops._p(src1), src1.stride(0), C1, ops._p(src2), src2.stride(0) if src2 is not None else 0, C2, H2, W2, ops._p(out), kp, kp,
                                  B, H, W, ksize, stride, up1, ops._stream()))
        return out, Ho, Wo

    def gn(self, tag, x, norm, B, HW, C, silu, add=None):
        y = self.buf(tag, B * HW, C)
        L.check(L.groupnorm_nhwc_f32(ops._p(x), x.stride(0), ops._p(add), add.stride(0) if add is not None else 0, ops._p(norm.weight.detach()),
                                     ops._p(norm.bias.detach()), ops._p(y), C, B, HW, C, norm.num_groups, float(norm.eps), 1 if silu else 0, ops._stream()))
        return y

    def add(self, a, b, R, C):
        out = torch.empty(R, C, dtype=torch.float32, device=a.device)
        L.check(L.add_f32(ops._p(a), a.stride(0), ops._p(b), b.stride(0), ops._p(out), C, R, C, ops._stream()))
        return out

    def conv3(self, tag, x, conv, B, H, W, stride=1, up1=0, out=None):
        C, Co = conv.weight.shape[1], conv.weight.shape[0]
        col, Ho, Wo = self.im2col("col", x, C, B, H, W, 3, stride, up1)
        if out is None:
            out = self.buf(tag, B * Ho * Wo, Co)
        self.gemm(col, self.w_conv(conv), conv.bias, out, B * Ho * Wo, Co, 9 * C)
        return out, Ho, Wo

    def res(self, tag, m, x, emb_all, B, H, W):
        R = B * H * W
        a = self.gn("act", x, m.in_layers[0], B, H * W, m.cin, True)
        h, _, _ = self.conv3("h1", a, m.in_layers[2], B, H, W)
        o = self._emb_off[self._res_index[id(m)]]
        a2 = self.gn("act", h, m.out_layers[0], B, H * W, m.cout, True, add=emb_all[:, o:o + m.cout])
        h2, _, _ = self.conv3("h2", a2, m.out_layers[3], B, H, W)
        xs = x
        if not isinstance(m.skip_connection, nn.Identity):
            xs = self.gemm(x, self.w_conv(m.skip_connection), m.skip_connection.bias, self.buf("skipc", R, m.cout), R, m.cout, m.cin)
        return self.add(xs, h2, R, m.cout)

    def attn(self, m, x, B, H, W):
        T, C = H * W, m.ch
        n = self.gn("act", x, m.norm, B, T, C, False)
        qkv = self.gemm(n, self.w_conv(m.qkv), m.qkv.bias, self.buf("qkv", B * T, 3 * C), B * T, 3 * C, C)
        a = self.buf("attn_o", B * T, C)
        L.check(L.unet_attention_f32(ops._p(qkv), 3 * C, ops._p(a), C, B, T, m.heads, C // m.heads, ops._stream()))
        pr = self.gemm(a, self.w_conv(m.proj_out), m.proj_out.bias, self.buf("h2", B * T, C), B * T, C, C)
        return self.add(x, pr, B * T, C)

    # ---- one evaluation --------------------------------------------------------------------------------------------------------------
    def forward(self, sample, timestep, cond, cond_mask):
        net = self.net
        dev = sample.device
        f32 = torch.float32
        B, C, H, W = sample.shape
        P = net.P_H
        if H % P or W % P:
            raise ValueError(f"Image sizes {H}x{W} must be divisible by patch sizes {P}x{P}")
        nh, nw = H // P, W // P
        CP = C * P * P
        if CP % 4 or net.cond_channels % 4:
            raise NotImplementedError("patch / conditioning widths must be multiples of 4 (compute_precision = 'fp32')")
        if nh != nw or H != W:
            raise NotImplementedError("non-square inputs")
        R = B * nh * nw
        # 'b c (nh ph) (nw pw) -> (b nh nw) (c ph pw)': the rows fm_vq_patchify writes, in f32 (plumbing)
        rows = self.buf("patch", R, CP)
        rows.view(B, nh, nw, C, P, P).copy_(sample.detach().to(f32).contiguous().view(B, C, nh, P, nw, P).permute(0, 2, 4, 1, 3, 5))
        cnd = cond.detach().to(f32)
        if cond_mask is not None:
            cnd = torch.where(cond_mask[:, None].to(dev), torch.zeros((), device=dev), cnd)
        D, Hc, Wc = cnd.shape[1:]
        crow = cnd.permute(0, 2, 3, 1).reshape(B * Hc * Wc, D).contiguous()
        # timestep embedding -> time_embed MLP -> silu -> every ResBlock's projection in one GEMM
        t = torch.as_tensor(timestep, device=dev).reshape(-1).to(f32)
        if t.numel() == 1:
            t = t.expand(B)
        t = t.contiguous()
        mc, te = net.model_channels, net.model_channels * 4
        temb = self.buf("temb", B, mc)
        L.check(L.timestep_embedding_f32(ops._p(t), ops._p(temb), mc, B, mc, 10000.0, ops._stream()))
        l0, l2 = net.time_embed[0], net.time_embed[2]
        e1 = self.gemm(temb, self.w_conv_lin(l0), l0.bias, self.buf("e1", B, te), B, te, mc)
        s1 = self.buf("s1", B, te)
        L.check(L.silu_f32(ops._p(e1), ops._p(s1), B * te, ops._stream()))
        e2 = self.gemm(s1, self.w_conv_lin(l2), l2.bias, self.buf("e2", B, te), B, te, te)
        s2 = self.buf("s2", B, te)
        L.check(L.silu_f32(ops._p(e2), ops._p(s2), B * te, ops._stream()))
        wall, ball = self.w_emb_all()
        emb_all = self.gemm(s2, wall, ball, self.buf("emb_all", B, self._emb_total), B, self._emb_total, te)
        # input blocks
        first = net.input_blocks[0][0]
        col, _, _ = self.im2col("col", rows, CP, B, nh, nw, 3, 1, 0, src2=crow, C2=D, H2=Hc, W2=Wc)
        ch0 = first.weight.shape[0]
        h = self.gemm(col, self.w_conv(first), first.bias, torch.empty(R, ch0, dtype=f32, device=dev), R, ch0, col.shape[1])
        hs, hh, ww = [(h, nh, nw)], nh, nw
        for blk in list(net.input_blocks)[1:]:
            h, hh, ww = self.run(blk, h, emb_all, B, hh, ww)
            hs.append((h, hh, ww))
        h, hh, ww = self.run(net.middle_block, h, emb_all, B, hh, ww)
        for blk in net.output_blocks:
            skip, sh, sw = hs.pop()
            assert (sh, sw) == (hh, ww)
            C1, C2 = h.shape[1], skip.shape[1]
            cat = torch.empty(B * hh * ww, C1 + C2, dtype=f32, device=dev)
            L.check(L.unet_im2col_f32(ops._p(h), h.stride(0), C1, ops._p(skip), skip.stride(0), C2, hh, ww, ops._p(cat), C1 + C2, C1 + C2, B, hh, ww, 1, 1, 0,
                                      ops._stream()))
            h, hh, ww = self.run(blk, cat, emb_all, B, hh, ww)
        a = self.gn("act", h, net.out[0], B, hh * ww, h.shape[1], True)
        conv = net.out[2]
        OP = conv.weight.shape[0]
        y = self.buf("y", B * hh * ww, ru(OP, 4))
        self.conv3("y", a, conv, B, hh, ww, out=y)
        img = torch.empty(B, net.out_channels, H, W, dtype=f32, device=dev)
        L.check(L.vq_unpatchify(ops._p(y), y.stride(0), ops._p(img), B, net.out_channels, H, W, P, ops._stream()))
        return img


class _UNetTrainF32(_UNetEngineF32):
    """Training form of the fp32 launch sequence: the forward of _UNetEngineF32 launch for launch (bit-identical values), with everything the
    backward reads - the inputs of the convolutions, GroupNorms and Linears, qkv - in tensors owned by that call; the shared ``buf(tag)``
    scratch only holds what one launch hands to the next (the column matrices, re-made by fm_unet_im2col_f32 in the backward).  forward_train
    returns the image and the closure that walks the tape in reverse: out, output_blocks, middle_block, input_blocks, the time-embedding MLP.
    Parameter gradients only (the decoder on a frozen encoder): the first convolution computes its dW alone.  Every reduction of the backward
    runs in a fixed order (csrc/unet_f32_bwd.hip, fm_gemm_f32, fm_vit_colsum): two runs give the same bits.  Verification mode, not a hot path."""

    def new(self, rows, cols):
        return torch.empty(rows, cols, dtype=torch.float32, device=self.net.device)

    def _colsum_ws(self, N):
        ws = getattr(self, "_ws64", None)
        if ws is None or ws.numel() < 64 * N or ws.device != self.net.device:
            ws = self._ws64 = torch.empty(64 * N, dtype=torch.float64, device=self.net.device)
        return ws

    # ---- parameter gradients: torch semantics (added to .grad, created when None, in the parameter's own layout) -------------------------
    @staticmethod
    def _acc(p, g):
        g = g.reshape(p.shape).to(p.dtype)
        if p.grad is None:
            p.grad = g.clone(memory_format=torch.contiguous_format)
        else:
            p.grad.add_(g)

    def _wgrad(self, dout, xmat, weight, bias, M, N, K, to_param=None):
        """dW = dout^T xmat (N, K) and db = column sums of dout, for the operands that require a gradient (xmat: a callable that makes the matrix)."""
        if weight.requires_grad:
            dw = torch.zeros(N, K, dtype=torch.float32, device=dout.device)
            ops.gemm_tn(dout, xmat(), dw, N=N, K=K, R=M)
            self._acc(weight, to_param(dw) if to_param is not None else dw)
        if bias is not None and bias.requires_grad:
            db = torch.zeros(N, dtype=torch.float32, device=dout.device)
            ops.vit_colsum(dout, db, self._colsum_ws(N), R=M)
            self._acc(bias, db)

    def _dx(self, dout, wimg, out, M, N, K):
        """out (M, K) = dout (M, N) wimg (N, K): fm_gemm_f32 with the weight image read through its strides"""
        return ops._gemm_f32(dout, wimg.t(), out, epilogue=L.EPI_F32, M=M, N=K, K=N)

    # ---- building blocks: each returns (output, backward closure dout -> dx) -------------------------------------------------------------
    def lin_t(self, x, mod, wimg, M, N, K, need_dx=True):
        out = self.gemm(x, wimg, mod.bias, self.new(M, N), M, N, K)

        def bwd(dout):
            self._wgrad(dout, lambda: x, mod.weight, mod.bias, M, N, K)
            return self._dx(dout, wimg, self.new(M, K), M, N, K) if need_dx else None
        return out, bwd

    def conv3_t(self, x, conv, B, H, W, stride=1, up1=0, need_dx=True, src2=None):
        """3 x 3 convolution; src2 = (rows, C2, H2, W2): the conditioning of the first convolution (no gradient to either source then)"""
        C, Co = conv.weight.shape[1], conv.weight.shape[0]
        C1 = C - (src2[1] if src2 else 0)
        two = dict(src2=src2[0], C2=src2[1], H2=src2[2], W2=src2[3]) if src2 else {}
        col, Ho, Wo = self.im2col("col", x, C1, B, H, W, 3, stride, up1, **two)
        M = B * Ho * Wo
        wimg = self.w_conv(conv)
        out = self.gemm(col, wimg, conv.bias, self.new(M, ru(Co, 4)), M, Co, 9 * C)

        def bwd(dout):
            self._wgrad(dout, lambda: self.im2col("col", x, C1, B, H, W, 3, stride, up1, **two)[0], conv.weight, conv.bias, M, Co, 9 * C,
                        lambda dw: dw.view(Co, 3, 3, C).permute(0, 3, 1, 2))          # taps outermost -> (Cout, Cin, 3, 3)
            if not need_dx:
                return None
            dcol = self._dx(dout, wimg, self.buf("dcol", M, 9 * C), M, Co, 9 * C)
            dx = self.new(x.shape[0], C)
            L.check(L.unet_col2im_f32(ops._p(dcol), 9 * C, ops._p(dx), C, C, B, H, W, 3, stride, up1, 0, ops._stream()))
            return dx
        return out, Ho, Wo, bwd

    def gn_t(self, x, norm, B, HW, C, silu, add=None, emb_off=None, S=None):
        y = self.new(B * HW, C)
        L.check(L.groupnorm_nhwc_f32(ops._p(x), x.stride(0), ops._p(add), add.stride(0) if add is not None else 0, ops._p(norm.weight.detach()),
                                     ops._p(norm.bias.detach()), ops._p(y), C, B, HW, C, norm.num_groups, float(norm.eps), 1 if silu else 0, ops._stream()))

        def bwd(dy):
            dx = self.new(B * HW, C)
            dev = dy.device
            dw = torch.empty(C, dtype=torch.float32, device=dev) if norm.weight.requires_grad else None
            db = torch.empty(C, dtype=torch.float32, device=dev) if norm.bias.requires_grad else None
            dadd = S["demb"][:, emb_off:emb_off + C] if add is not None else None
            scratch = self.buf("gn_bwd", 2 * B, C) if dw is not None or db is not None else None
            L.check(L.groupnorm_nhwc_bwd_f32(ops._p(dy), dy.stride(0), ops._p(x), x.stride(0), ops._p(add), add.stride(0) if add is not None else 0,
                                             ops._p(norm.weight.detach()), ops._p(norm.bias.detach()), ops._p(dx), C, ops._p(dw), ops._p(db), ops._p(dadd),
                                             dadd.stride(0) if dadd is not None else 0, ops._p(scratch), B, HW, C, norm.num_groups, float(norm.eps),
                                             1 if silu else 0, ops._stream()))
            if dw is not None:
                self._acc(norm.weight, dw)
            if db is not None:
                self._acc(norm.bias, db)
            return dx
        return y, bwd

    def res_t(self, m, x, emb_all, B, H, W, S):
        R = B * H * W
        a, b_gn1 = self.gn_t(x, m.in_layers[0], B, H * W, m.cin, True)
        h, _, _, b_c1 = self.conv3_t(a, m.in_layers[2], B, H, W)
        o = self._emb_off[self._res_index[id(m)]]
        a2, b_gn2 = self.gn_t(h, m.out_layers[0], B, H * W, m.cout, True, add=emb_all[:, o:o + m.cout], emb_off=o, S=S)
        h2, _, _, b_c2 = self.conv3_t(a2, m.out_layers[3], B, H, W)
        xs, b_skip = x, None
        if not isinstance(m.skip_connection, nn.Identity):
            xs, b_skip = self.lin_t(x, m.skip_connection, self.w_conv(m.skip_connection), R, m.cout, m.cin)
        out = self.add(xs, h2, R, m.cout)

        def bwd(dout):                     # the gradient of x: through the GroupNorm branch and through the skip path
            dx = b_gn1(b_c1(b_gn2(b_c2(dout))))
            return self.add(dx, dout if b_skip is None else b_skip(dout), R, m.cin)
        return out, bwd

    def attn_t(self, m, x, B, H, W):
        T, C = H * W, m.ch
        n, b_gn = self.gn_t(x, m.norm, B, T, C, False)
        qkv, b_qkv = self.lin_t(n, m.qkv, self.w_conv(m.qkv), B * T, 3 * C, C)
        a = self.new(B * T, C)
        L.check(L.unet_attention_f32(ops._p(qkv), 3 * C, ops._p(a), C, B, T, m.heads, C // m.heads, ops._stream()))
        pr, b_proj = self.lin_t(a, m.proj_out, self.w_conv(m.proj_out), B * T, C, C)
        out = self.add(x, pr, B * T, C)

        def bwd(dout):
            da = b_proj(dout)
            dqkv = self.new(B * T, 3 * C)
            L.check(L.unet_attention_bwd_f32(ops._p(qkv), 3 * C, ops._p(da), C, ops._p(dqkv), 3 * C, ops._p(self.buf("attn_bwd", B * m.heads * T, 3)),
                                             B, T, m.heads, C // m.heads, ops._stream()))
            return self.add(b_gn(b_qkv(dqkv)), dout, B * T, C)
        return out, bwd

    def run_t(self, seq, h, emb_all, B, H, W, S):
        bwds = []
        for m in seq:
            if isinstance(m, _Res):
                h, b = self.res_t(m, h, emb_all, B, H, W, S)
            elif isinstance(m, _Attn):
                h, b = self.attn_t(m, h, B, H, W)
            elif isinstance(m, _Down):
                h, H, W, b = self.conv3_t(h, m.op, B, H, W, stride=2)
            elif isinstance(m, _Up):
                h, H, W, b = self.conv3_t(h, m.conv, B, 2 * H, 2 * W, up1=1)
            else:
                raise TypeError(type(m))
            bwds.append(b)

        def bwd(d):
            for b in reversed(bwds):
                d = b(d)
            return d
        return h, H, W, bwd

    def silu_bwd(self, dy, x):
        dx = torch.empty_like(x)
        L.check(L.silu_bwd_f32(ops._p(dy), ops._p(x), ops._p(dx), x.numel(), ops._stream()))
        return dx

    # ---- one differentiable evaluation ---------------------------------------------------------------------------------------------------
    def forward_train(self, sample, timestep, cond, cond_mask):
        """(image, backward): backward(d image) adds every trainable parameter's gradient to its .grad."""
        net = self.net
        dev = sample.device
        f32 = torch.float32
        if torch.cuda.is_current_stream_capturing():
            raise NotImplementedError("the training step of the fp32 UNet is not graph-capturable")
        B, C, H, W = sample.shape
        P = net.P_H
        if H % P or W % P:
            raise ValueError(f"Image sizes {H}x{W} must be divisible by patch sizes {P}x{P}")
        nh, nw = H // P, W // P
        CP = C * P * P
        if CP % 4 or net.cond_channels % 4:
            raise NotImplementedError("patch / conditioning widths must be multiples of 4 (compute_precision = 'fp32')")
        if nh != nw or H != W:
            raise NotImplementedError("non-square inputs")
        R = B * nh * nw
        S = {}                                                    # state of THIS call's backward (the gradient of emb_all)
        stamp = self._weights_stamp()
        rows = self.new(R, CP)
        rows.view(B, nh, nw, C, P, P).copy_(sample.detach().to(f32).contiguous().view(B, C, nh, P, nw, P).permute(0, 2, 4, 1, 3, 5))
        cnd = cond.detach().to(f32)
        if cond_mask is not None:
            cnd = torch.where(cond_mask[:, None].to(dev), torch.zeros((), device=dev), cnd)
        D, Hc, Wc = cnd.shape[1:]
        crow = cnd.permute(0, 2, 3, 1).reshape(B * Hc * Wc, D).contiguous()
        t = torch.as_tensor(timestep, device=dev).reshape(-1).to(f32)
        if t.numel() == 1:
            t = t.expand(B)
        t = t.contiguous()
        mc, te = net.model_channels, net.model_channels * 4
        temb = self.new(B, mc)
        L.check(L.timestep_embedding_f32(ops._p(t), ops._p(temb), mc, B, mc, 10000.0, ops._stream()))
        l0, l2 = net.time_embed[0], net.time_embed[2]
        w0, w2 = self.w_conv_lin(l0), self.w_conv_lin(l2)
        e1 = self.gemm(temb, w0, l0.bias, self.new(B, te), B, te, mc)
        s1 = self.new(B, te)
        L.check(L.silu_f32(ops._p(e1), ops._p(s1), B * te, ops._stream()))
        e2 = self.gemm(s1, w2, l2.bias, self.new(B, te), B, te, te)
        s2 = self.new(B, te)
        L.check(L.silu_f32(ops._p(e2), ops._p(s2), B * te, ops._stream()))
        wall, ball = self.w_emb_all()
        ET = self._emb_total
        emb_all = self.gemm(s2, wall, ball, self.new(B, ET), B, ET, te)
        # input blocks
        first = net.input_blocks[0][0]
        h, _, _, b_first = self.conv3_t(rows, first, B, nh, nw, need_dx=False, src2=(crow, D, Hc, Wc))
        hs, hh, ww, b_in = [(h, nh, nw)], nh, nw, []
        for blk in list(net.input_blocks)[1:]:
            h, hh, ww, b = self.run_t(blk, h, emb_all, B, hh, ww, S)
            hs.append((h, hh, ww))
            b_in.append(b)
        h, hh, ww, b_mid = self.run_t(net.middle_block, h, emb_all, B, hh, ww, S)
        b_out = []
        for blk in net.output_blocks:
            skip, sh, sw = hs.pop()
            assert (sh, sw) == (hh, ww)
            C1, C2 = h.shape[1], skip.shape[1]
            cat = self.new(B * hh * ww, C1 + C2)
            L.check(L.unet_im2col_f32(ops._p(h), h.stride(0), C1, ops._p(skip), skip.stride(0), C2, hh, ww, ops._p(cat), C1 + C2, C1 + C2, B, hh, ww, 1, 1, 0,
                                      ops._stream()))
            h, hh, ww, b = self.run_t(blk, cat, emb_all, B, hh, ww, S)
            b_out.append((b, C1))
        Cl = h.shape[1]
        a, b_gn = self.gn_t(h, net.out[0], B, hh * ww, Cl, True)
        conv = net.out[2]
        OP = conv.weight.shape[0]
        y, _, _, b_conv = self.conv3_t(a, conv, B, hh, ww)
        img = torch.empty(B, net.out_channels, H, W, dtype=f32, device=dev)
        L.check(L.vq_unpatchify(ops._p(y), y.stride(0), ops._p(img), B, net.out_channels, H, W, P, ops._stream()))
        res = self._res

        def backward(dimg):
            if self._weights_stamp() != stamp:
                raise RuntimeError("PatchedUNetCondCat: a parameter was modified between this evaluation and its backward")
            S["demb"] = torch.zeros(B, ET, dtype=f32, device=dev)
            # the adjoint of the un-patchify: 'b c (nh ph) (nw pw) -> (b nh nw) (c ph pw)' (plumbing, as in the forward)
            dy = dimg.detach().to(f32).contiguous().view(B, net.out_channels, nh, P, nw, P).permute(0, 2, 4, 1, 3, 5).reshape(R, OP).contiguous()
            d = b_gn(b_conv(dy))
            dskips = []                                           # the skip concatenation's adjoint: a column split, by views
            for b, C1 in reversed(b_out):
                dcat = b(d)
                d = dcat[:, :C1]
                dskips.append(dcat[:, C1:])                        # (in the order hs was filled)
            d = b_mid(d)
            for i in range(len(b_in), 0, -1):                      # hs[i] fed the next block and its skip concatenation
                d = b_in[i - 1](self.add(d, dskips[i], d.shape[0], d.shape[1]))
            b_first(self.add(d, dskips[0], d.shape[0], d.shape[1]))
            # the per-ResBlock slices of emb_all -> the stacked projection -> time_embed
            demb = S.pop("demb")
            lins = [m.emb_layers[1] for m in res]
            if any(l.weight.requires_grad for l in lins):
                dwall = torch.zeros(ET, te, dtype=f32, device=dev)
                ops.gemm_tn(demb, s2, dwall, N=ET, K=te, R=B)
            if any(l.bias.requires_grad for l in lins):
                dball = torch.zeros(ET, dtype=f32, device=dev)
                ops.vit_colsum(demb, dball, self._colsum_ws(ET), R=B)
            for m, l, o in zip(res, lins, self._emb_off):
                if l.weight.requires_grad:
                    self._acc(l.weight, dwall[o:o + m.cout])
                if l.bias.requires_grad:
                    self._acc(l.bias, dball[o:o + m.cout])
            if any(p.requires_grad for p in net.time_embed.parameters()):
                de2 = self.silu_bwd(self._dx(demb, wall, self.new(B, te), B, ET, te), e2)
                self._wgrad(de2, lambda: s1, l2.weight, l2.bias, B, te, te)
                if any(p.requires_grad for p in l0.parameters()):
                    de1 = self.silu_bwd(self._dx(de2, w2, self.new(B, te), B, te, te), e1)
                    self._wgrad(de1, lambda: temb, l0.weight, l0.bias, B, te, mc)
        return img, backward


class _UNetTrainStep(torch.autograd.Function):
    """Bridges the hand-written backward of _UNetTrainF32 into autograd: the image is a leaf of the caller's loss graph, hung on one trainable
    parameter (the anchor); the backward deposits every parameter gradient itself and hands autograd nothing."""

    @staticmethod
    def forward(ctx, anchor, engine, sample, timestep, cond, cond_mask):
        img, ctx.bwd = engine.forward_train(sample, timestep, cond, cond_mask)
        return img

    @staticmethod
    def backward(ctx, g):
        if ctx.bwd is None:
            raise RuntimeError("PatchedUNetCondCat: this evaluation's backward has run already (its saved tensors are freed)")
        ctx.bwd(g)
        ctx.bwd = None
        return None, None, None, None, None, None
