"""LPIPS perceptual loss of the tokenizer recipes on the HIP engine (upstream fourm/vq/percept_losses/lpips.py:96-109 and :112-177,
``percept_loss_type: lpips``): a FROZEN VGG16 feature stack - 13 convolutions 3 x 3 with bias and ReLU, 4 max-pools - tapped after relu1_2,
relu2_2, relu3_3, relu4_3 and relu5_3; per tap the channel-normalised features of the reconstruction and of the image are compared through a
learned per-channel weight, averaged over the pixels, and the five taps are added.  The gradient flows back to the reconstructed pixels;
the network gets none.

    targets -> stem, 12 implicit-GEMM convolutions (FM_EPI_RELU), 4 pools; the 5 tap maps kept until the distances are taken
    preds   -> the same, all 13 activation maps kept when a backward will follow
    per tap: fm_lpips_distance -> loss (B,) +=, d(loss[b]) / d(tap rows of preds)
    backward, layer 12 down to 0: fm_lpips_tap_bwd at a tap layer (ReLU mask, the tap's gradient, the pool's gradient routed to the window's
    first maximum); the dgrad convolution = the same implicit GEMM on the dgrad weight image, with the ReLU mask of the layer below in its
    epilogue (FM_EPI_RELU_BWD); fm_lpips_stem_bwd scales by 1 / scale_c and by the incoming d / d(loss[b]).
    fp32 mode: fm_unet_im2col_f32 + fm_gemm_f32 for every convolution and dgrad, the mask as fm_lpips_tap_bwd in place.

Where a pixel's feature vector is all zero the part of normalize_tensor's gradient that divides by the norm is taken as 0 (torch gives NaN);
the ReLU mask zeroes that pixel's gradient either way.

Not here: fetching ``vgg.pth`` (load it: ``LpipsPerceptualLoss(torch.load("vgg.pth"))``), the generic timm perceptual loss, a trainable
VGG or trainable lin layers, input sizes that are not multiples of 16, resizing in front of the loss."""
import torch
from torch import nn

# (slice, index inside torchvision's vgg16.features, C_in, C_out); a tap follows layers 1, 3, 6, 9, 12, a pool follows the first four taps
VGG_CONVS = [(1, 0, 3, 64), (1, 2, 64, 64), (2, 5, 64, 128), (2, 7, 128, 128), (3, 10, 128, 256), (3, 12, 256, 256), (3, 14, 256, 256),
             (4, 17, 256, 512), (4, 19, 512, 512), (4, 21, 512, 512), (5, 24, 512, 512), (5, 26, 512, 512), (5, 28, 512, 512)]
TAP_LAYERS = [1, 3, 6, 9, 12]
CHNS = [64, 128, 256, 512, 512]
EPS = 1e-10


class ScalingLayer(nn.Module):
    def __init__(self):
        super().__init__()
        self.register_buffer("shift", torch.tensor([-.030, -.088, -.188])[None, :, None, None])
        self.register_buffer("scale", torch.tensor([.458, .448, .450])[None, :, None, None])


class NetLinLayer(nn.Module):
    """Upstream's 1 x 1 convolution without bias behind a Dropout (index 0, inactive in eval mode and not built here): ``model.1.weight``."""

    def __init__(self, chn_in):
        super().__init__()
        self.model = nn.Module()
        self.model.add_module("1", nn.Conv2d(chn_in, 1, 1, stride=1, padding=0, bias=False))


def dgrad_weight_image(w):
    """(C_out, C_in, 3, 3) -> (C_in, 9 C_out): W_d[c][tap' C_out + n] = w[n][c][2 - ky'][2 - kx'].  The input gradient of the convolution is
    the same 3 x 3 convolution (padding 1) of dY with these rows as its (taps outermost) weight operand."""
    return w.flip(2, 3).permute(1, 2, 3, 0).reshape(w.shape[1], 9 * w.shape[0])


class _LpipsStep(torch.autograd.Function):
    """Bridges the hand-written backward into autograd: ``preds`` is the only differentiable input."""

    @staticmethod
    def forward(ctx, preds, module, targets):
        loss, saved = module._run(preds, targets, save=True)
        ctx.module, ctx.saved, ctx.dtype = module, saved, preds.dtype
        return loss

    @staticmethod
    def backward(ctx, g_loss):
        saved, ctx.saved = ctx.saved, None
        d = ctx.module._backward(saved, g_loss.reshape(-1).float().contiguous())
        return d.to(ctx.dtype), None, None


class LpipsPerceptualLoss(nn.Module):
    """forward(preds, targets) -> (B, 1, 1, 1) fp32, upstream's LPIPS.forward for images (B, 3, H, W) in [-1, 1] (fp32, bf16 or fp16; H and W
    multiples of 16).  Parameter and buffer names and shapes are upstream's, so ``load_state_dict(torch.load("vgg.pth"), strict=False)`` works
    as upstream's load_from_pretrained does; without a state dict the weights are seeded-random.  Everything is frozen and the module is
    always in eval mode.  ``compute_precision``: "bf16" (bf16 operands and feature maps, fp32 accumulation, fp32 distance arithmetic) or
    "fp32" (the same launch sequence on the fp32 kernels: the verification mode).
    ``targets`` never receives a gradient; ``preds`` does when it requires one and gradients are enabled.  The state of that pass lives in
    this module's workspace: one forward may be awaiting its backward at a time."""

    def __init__(self, state_dict=None, compute_precision="bf16"):
        super().__init__()
        if compute_precision not in ("bf16", "fp32"):
            raise ValueError(f"compute_precision {compute_precision!r}: 'bf16' or 'fp32'")
        self.compute_precision = compute_precision
        self.scaling_layer = ScalingLayer()
        self.chns = list(CHNS)
        self.net = nn.Module()
        for s in range(1, 6):
            self.net.add_module(f"slice{s}", nn.Module())
        for s, idx, cin, cout in VGG_CONVS:
            getattr(self.net, f"slice{s}").add_module(str(idx), nn.Conv2d(cin, cout, 3, padding=1))
        for k, c in enumerate(CHNS):
            setattr(self, f"lin{k}", NetLinLayer(c))
        g = torch.Generator().manual_seed(0)
        with torch.no_grad():
            for conv in self._convs():
                fan_in = conv.weight.shape[1] * 9
                conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * (2.0 / fan_in) ** 0.5)
                conv.bias.copy_(0.1 * torch.randn(conv.bias.shape, generator=g))
            for k, c in enumerate(CHNS):
                w = self._lin(k)
                w.copy_(torch.rand(w.shape, generator=g) / c)
        if state_dict is not None:
            self.load_state_dict(state_dict, strict=False)
        self.requires_grad_(False)
        super().train(False)
        self.__dict__["_cache"] = None          # device images of the weights
        self.__dict__["_ws"] = None             # named device buffers
        self.__dict__["_gen"] = 0               # counts the training forwards: a backward belongs to the most recent one

    # ---- module plumbing ---------------------------------------------------------------------------------------------------------
    def _convs(self):
        return [getattr(getattr(self.net, f"slice{s}"), str(idx)) for s, idx, _, _ in VGG_CONVS]

    def _lin(self, k):
        return getattr(getattr(self, f"lin{k}").model, "1").weight

    def train(self, mode: bool = True):
        """Always in eval mode, whatever the trainer sets on the modules around it."""
        return super().train(False)

    def percept_transform(self, x):
        """The identity: upstream's trainer assigns no transform in front of LPIPS."""
        return x

    def _check(self, preds, targets):
        if preds.dim() != 4 or preds.shape[1] != 3:
            raise ValueError(f"expected images (B, 3, H, W), got {tuple(preds.shape)}")
        if preds.shape != targets.shape:
            raise ValueError(f"preds {tuple(preds.shape)} and targets {tuple(targets.shape)} differ in shape")
        H, W = preds.shape[-2:]
        if H % 16 or W % 16 or H == 0 or W == 0:
            raise NotImplementedError(f"images of {H}x{W}: the four 2 x 2 max-pools of VGG16 need H and W to be multiples of 16 - resize or crop before the loss")
        if not (preds.is_cuda and targets.is_cuda):
            raise RuntimeError("LPIPS computes on an MI355X through libfourm_hip.so; move the images and the module to the GPU first (there is no CPU path)")
        if preds.dtype not in (torch.float32, torch.bfloat16, torch.float16):
            raise TypeError(f"images of dtype {preds.dtype}: fp32, bf16 or fp16 expected")

    def forward(self, preds: torch.Tensor, targets: torch.Tensor) -> torch.Tensor:
        self._check(preds, targets)
        if preds.requires_grad and torch.is_grad_enabled():
            return _LpipsStep.apply(preds, self, targets.detach())
        return self._run(preds.detach(), targets.detach(), save=False)[0]

    # ---- device state ------------------------------------------------------------------------------------------------------------
    def _prepare(self, device):
        """Weight images for the kernels, rebuilt when a parameter, the device or the precision changed: per convolution the (C_out, 9 C_in)
        rows (taps outermost) and the dgrad image (C_in, 9 C_out), bf16 or f32; the stem's (64, 27) f32 rows; ScalingLayer as mul / add."""
        from fourm.hip import ops
        from fourm.hip.engine import Workspace
        params = [p for p in self.parameters()] + [self.scaling_layer.shift, self.scaling_layer.scale]
        if params[0].device != device:
            raise RuntimeError(f"input on {device}, loss module on {params[0].device}")
        stamp = (device, self.compute_precision, tuple((p._version, p.data_ptr()) for p in params))
        c = self._cache
        if c is not None and c["stamp"] == stamp:
            return c
        dt = torch.float32 if self.compute_precision == "fp32" else torch.bfloat16

        def image(flat):
            flat = flat.float().contiguous()
            return ops.f32_to_bf16(flat, torch.empty(flat.shape, dtype=dt, device=device))

        convs = self._convs()
        with torch.no_grad():
            scale, shift = self.scaling_layer.scale.reshape(3).double(), self.scaling_layer.shift.reshape(3).double()
            c = dict(stamp=stamp, dtype=dt, mul=(1.0 / scale).float().contiguous(), add=(-shift / scale).float().contiguous(),
                     stem_w=convs[0].weight.detach().reshape(64, 27).float().contiguous(), bias=[cv.bias.detach().float().contiguous() for cv in convs],
                     w=[None] + [image(cv.weight.detach().permute(0, 2, 3, 1).reshape(cv.weight.shape[0], -1)) for cv in convs[1:]],
                     wd=[None] + [image(dgrad_weight_image(cv.weight.detach())) for cv in convs[1:]],
                     lin=[self._lin(k).detach().reshape(-1).float().contiguous() for k in range(5)])
        self.__dict__["_cache"] = c
        if self._ws is None or self._ws.device != device:
            self.__dict__["_ws"] = Workspace(device)
        return c

    def _conv(self, c, li, x, out, B, H, W, dgrad=False, mask=None):
        """Layer li's convolution (or, dgrad, its input gradient) on rows: bf16 - the implicit GEMM with the ReLU / masked epilogue;
        fp32 - fm_unet_im2col_f32 + fm_gemm_f32 (+ the in-place mask)."""
        from fourm.hip import _lib as L
        from fourm.hip import ops
        _, _, cin, cout = VGG_CONVS[li]
        Cx, N = (cout, cin) if dgrad else (cin, cout)
        w = c["wd"][li] if dgrad else c["w"][li]
        bias = None if dgrad else c["bias"][li]
        M = B * H * W
        if c["dtype"] == torch.float32:
            col = self._ws.get("col", (M, 9 * Cx), torch.float32)
            L.check(L.unet_im2col_f32(ops._p(x), x.stride(0), Cx, None, 0, 0, 0, 0, ops._p(col), 9 * Cx, 9 * Cx, B, H, W, 3, 1, 0, ops._stream()))
            ops.gemm_nt(col, w, out, epilogue=L.EPI_F32 if dgrad else L.EPI_RELU, bias=bias, M=M, N=N, K=9 * Cx)
            if mask is not None:
                ops.lpips_tap_bwd(mask, out, B, H, W, din=out)
            return out
        epi = (L.EPI_RELU_BWD if mask is not None else L.EPI_BF16) if dgrad else L.EPI_RELU
        ops.gemm_nt(x, w, out, epilogue=epi, bias=bias, res=mask, M=M, N=N, K=9 * Cx, conv=dict(C=Cx, H=H, W=W, Ho=H, Wo=W, stride=1, up=0))
        return out

    def _features(self, c, img, tag, keep_all):
        """The 13 layers on one batch of images.  Returns (activation maps by layer - all of them, or the tap layers only -, their (H, W))."""
        from fourm.hip import ops
        ws, dt = self._ws, c["dtype"]
        B, _, H, W = img.shape
        acts, sizes = {}, {}
        x = None
        for li, (_, _, cin, cout) in enumerate(VGG_CONVS):
            keep = keep_all or li in TAP_LAYERS
            out = ws.get(f"{tag}.act{li}" if keep else f"{tag}.tmp{li % 2}", (B * H * W, cout), dt)
            if li == 0:
                ops.lpips_stem(img, c["mul"], c["add"], c["stem_w"], c["bias"][0], out, B, H, W)
            else:
                self._conv(c, li, x, out, B, H, W)
            if keep:
                acts[li], sizes[li] = out, (H, W)
            x = out
            if li in TAP_LAYERS[:4]:
                pooled = ws.get(f"{tag}.pool", (B * (H // 2) * (W // 2), cout), dt)
                ops.maxpool2x2_nhwc(x, pooled, B, H, W, cout)
                x, H, W = pooled, H // 2, W // 2
        return acts, sizes

    def _run(self, preds, targets, save):
        from fourm.hip import ops
        with torch.no_grad():
            c = self._prepare(preds.device)
            ws = self._ws
            B = preds.shape[0]
            p_img, t_img = preds.float().contiguous(), targets.float().contiguous()
            ft, _ = self._features(c, t_img, "tgt", False)
            tag = "fwd" if save else "ng"
            fp, sizes = self._features(c, p_img, tag, save)
            loss = torch.zeros(B, dtype=torch.float32, device=preds.device)
            d_taps = {}
            for k, li in enumerate(TAP_LAYERS):
                H, W = sizes[li]
                P = H * W
                d = ws.get(f"fwd.dtap{k}", (B * P, CHNS[k]), torch.float32) if save else None
                scratch = ws.get("dist.scratch", (ops.lpips_distance_scratch(B, P),), torch.float32)
                ops.lpips_distance(fp[li], ft[li], c["lin"][k], B, P, loss, d, scratch)
                d_taps[li] = d
        if not save:
            return loss.view(B, 1, 1, 1), None
        self.__dict__["_gen"] += 1
        return loss.view(B, 1, 1, 1), dict(gen=self._gen, acts=fp, sizes=sizes, d_taps=d_taps, shape=tuple(preds.shape), cache=c)

    def _backward(self, saved, g_loss):
        """d loss . g_loss / d preds, f32 (B, 3, H, W)."""
        from fourm.hip import ops
        if saved["gen"] != self._gen:
            raise RuntimeError("LpipsPerceptualLoss keeps the activations of the most recent training forward only: run backward before the next forward "
                               "that requires a gradient")
        c, acts, sizes, d_taps = saved["cache"], saved["acts"], saved["sizes"], saved["d_taps"]
        ws, dt = self._ws, c["dtype"]
        B, _, H0, W0 = saved["shape"]
        with torch.no_grad():
            d = None              # masked gradient of layer li's pre-activation
            g_pool = None         # gradient of the pool output behind tap layer li (None behind the last tap)
            for li in range(12, -1, -1):
                H, W = sizes[li]
                cout = VGG_CONVS[li][3]
                if li in TAP_LAYERS:
                    d = ops.lpips_tap_bwd(acts[li], ws.get(f"bwd.d{li % 2}", (B * H * W, cout), dt), B, H, W, dtap=d_taps[li], dpool=g_pool)
                if li == 0:
                    break
                cin = VGG_CONVS[li][2]
                if li - 1 in TAP_LAYERS:          # the input of this convolution is the pooled tap map: plain dgrad, routed by the tap layer
                    g_pool = self._conv(c, li, d, ws.get("bwd.gpool", (B * H * W, cin), dt), B, H, W, dgrad=True)
                else:
                    d = self._conv(c, li, d, ws.get(f"bwd.d{(li - 1) % 2}", (B * H * W, cin), dt), B, H, W, dgrad=True, mask=acts[li - 1])
            dimg = torch.empty(B, 3, H0, W0, dtype=torch.float32, device=d.device)
            ops.lpips_stem_bwd(d, c["stem_w"], c["mul"], g_loss, dimg, B, H0, W0)
        return dimg
