"""The AlexNet tower of the LPIPS validation metric on the HIP engine (upstream's eval_metrics, run_training_vqvae.py:1486-1491 and :1549:
torchmetrics' ``LearnedPerceptualImagePatchSimilarity(net_type='alex')``).  Forward only, fp32, frozen.

    per image:  fm_conv2d_stem_f32 (11 x 11, stride 4, padding 2, straight from the NCHW pixels; ``normalize`` and the ScalingLayer folded
                into one per-channel fmaf, the optional clamp in front of it)                                                     tap 1
                fm_pool2d_nhwc_f32 (max 3 x 3, stride 2) -> fm_conv2d_nhwc_f32 5 x 5, padding 2                                   tap 2
                pool -> 3 x 3 convolutions 192 -> 384 -> 256 -> 256, padding 1                                               taps 3, 4, 5
    per tap:    fm_lpips_score onto one zeroed (B,) buffer, in tap order

The layer table, the parameter names (the ``lpips`` package's: ``net.slice1.0`` ... ``net.slice5.10``, ``lin{k}.model.1.weight``,
``scaling_layer.shift`` / ``.scale``) and the normalisation a / sqrt(1e-8 + sum a^2) are restated from memory of torchvision, ``lpips`` and
torchmetrics: none of them was available when this was written, so parity with them and with the real checkpoints is NOT pinned
("LPIPS validation metric").  No weights are shipped: without a state dict they are seeded-random.

Every kernel is batch-invariant (tiles chosen by the channel counts alone, fixed summation orders), so a sample's score is the same bits
alone, in any batch and under any internal chunking.  No host synchronisation.  Tensors on the CPU raise RuntimeError (there is no CPU path)."""
import ctypes as C
from collections import OrderedDict

import torch
from torch import nn

from .lpips_loss import NetLinLayer, ScalingLayer

__all__ = ["LpipsAlex", "ALEX_CONVS", "CHNS", "EPS", "MIN_SIZE", "conv2d_stem", "lpips_score"]

# (slice, index inside torchvision's alexnet.features, C_in, C_out, kernel, stride, padding); a tap follows every layer, a pool the first two
ALEX_CONVS = [(1, 0, 3, 64, 11, 4, 2), (2, 3, 64, 192, 5, 1, 2), (3, 6, 192, 384, 3, 1, 1), (4, 8, 384, 256, 3, 1, 1), (5, 10, 256, 256, 3, 1, 1)]
CHNS = [64, 192, 384, 256, 256]
EPS = 1e-8
MIN_SIZE = 31          # the smallest side at which both max-pools still have a 3 x 3 window: 31 -> 7 -> 3 -> 1


def _iops():
    from fourm.utils.inception import ops
    return ops


def _vec(t, n, what):
    if t is None:
        return None
    if not (torch.is_tensor(t) and t.dtype == torch.float32 and t.is_cuda and t.is_contiguous() and t.numel() == n):
        raise ValueError(f"{what} must be a contiguous fp32 ({n},) tensor on the GPU")
    return t


def conv2d_stem(img, weight, bias, KH, KW, stride, pad, mul=None, add=None, clamp=None, relu=True, out=None):
    """fm_conv2d_stem_f32.  img fp32 (B, Cin, H, W) contiguous; weight rows (Cout, KH*KW*Cin) tap-major, channel-minor; bias, mul, add fp32
    vectors or None; ``clamp``: None or (lo, hi).  Writes (and returns) ``out`` rows (B*Ho*Wo, Cout)."""
    ops = _iops()
    L = ops._lib()
    if not torch.is_tensor(img) or img.dtype != torch.float32 or img.dim() != 4:
        raise TypeError("conv2d_stem: an fp32 (B, Cin, H, W) tensor is expected")
    if not img.is_cuda:
        raise RuntimeError(f"conv2d_stem: the images are on {img.device}; the LPIPS kernels run on an MI355X only (there is no CPU path)")
    if not img.is_contiguous():
        raise ValueError("conv2d_stem: contiguous images expected")
    weight = ops._rows(weight, "conv2d_stem: weight")
    B, Cin, H, W = img.shape
    Cout = weight.shape[0]
    if weight.shape[1] != KH * KW * Cin:
        raise ValueError(f"conv2d_stem: weight {tuple(weight.shape)} does not fit Cin={Cin} KH={KH} KW={KW}")
    bias, mul, add = _vec(bias, Cout, "conv2d_stem: bias"), _vec(mul, Cin, "conv2d_stem: mul"), _vec(add, Cin, "conv2d_stem: add")
    Ho, Wo = ops.conv_out_size(H, KH, stride, pad), ops.conv_out_size(W, KW, stride, pad)
    if Ho < 1 or Wo < 1:
        raise ValueError(f"conv2d_stem: the {KH} x {KW} kernel does not fit the padded {H} x {W} image")
    if out is None:
        out = torch.empty(B * Ho * Wo, Cout, dtype=torch.float32, device=img.device)
    out = ops._rows(out, "conv2d_stem: out")
    if tuple(out.shape) != (B * Ho * Wo, Cout):
        raise ValueError(f"conv2d_stem: out {tuple(out.shape)}, expected {(B * Ho * Wo, Cout)}")
    lo, hi = (0.0, 0.0) if clamp is None else (float(clamp[0]), float(clamp[1]))
    a = L.Conv2dStemArgs(img=ops._p(img), w=ops._p(weight), bias=ops._p(bias), mul=ops._p(mul), add=ops._p(add), out=ops._p(out), B=B, Cin=Cin, H=H, W=W,
                         Cout=Cout, KH=KH, KW=KW, stride=stride, pad=pad, ldw=weight.stride(0), ldo=out.stride(0), relu=1 if relu else 0,
                         clamp=0 if clamp is None else 1, reserved=0, lo=lo, hi=hi)
    with torch.cuda.device(img.device):
        L.check(L.conv2d_stem_f32(C.byref(a), ops._stream()))
    return out


def lpips_score(a, b, w, B, P, score, eps=EPS):
    """fm_lpips_score: score (B,) fp32 += the mean over the P pixels of sum_c w_c (a^ - b^)^2 for feature rows a, b (B*P, C)."""
    ops = _iops()
    L = ops._lib()
    a, b = ops._rows(a, "lpips_score: a"), ops._rows(b, "lpips_score: b")
    Cc = a.shape[1]
    if tuple(a.shape) != (B * P, Cc) or tuple(b.shape) != (B * P, Cc):
        raise ValueError(f"lpips_score: a {tuple(a.shape)} / b {tuple(b.shape)} do not fit B={B} P={P}")
    w, score = _vec(w, Cc, "lpips_score: w"), _vec(score, B, "lpips_score: score")
    n = L.lpips_score_scratch(B, P)
    L.check(min(n, 0))
    scratch = torch.empty(n, dtype=torch.float32, device=a.device)
    with torch.cuda.device(a.device):
        L.check(L.lpips_score(ops._p(a), a.stride(0), ops._p(b), b.stride(0), ops._p(w), B, P, Cc, float(eps), ops._p(score), ops._p(scratch), ops._stream()))
    return score


def fold_input_affine(shift, scale, normalize):
    """``normalize`` (x -> 2 x - 1) and the ScalingLayer ((x - shift) / scale) as one per-channel s = v * mul + add: float64 on the host ->
    (mul, add) float64 (3,)."""
    shift, scale = shift.reshape(-1).double().cpu(), scale.reshape(-1).double().cpu()
    g, o = (2.0, -1.0) if normalize else (1.0, 0.0)
    return g / scale, (o - shift) / scale


class LpipsAlex(nn.Module):
    """``scores(img0, img1, normalize, clamp0=False)`` -> (B,) fp32, the LPIPS distance of every pair.  Images (B, 3, H, W) with H, W >= 31,
    fp32 (bf16 / fp16 are converted to fp32 first): in [0, 1] with ``normalize=True``, in [-1, 1] without.  ``clamp0``: clamp ``img0`` to that
    range inside the stem's loads (upstream's ``reconst.clamp(0, 1)``).  ``chunk``: pairs per internal pass (bounds the workspace; it does not
    show in the result).  Frozen and always in eval mode."""

    def __init__(self, state_dict=None, chunk=64):
        super().__init__()
        self.scaling_layer = ScalingLayer()
        self.chns = list(CHNS)
        self.net = nn.Module()
        for s, idx, cin, cout, k, st, p in ALEX_CONVS:
            sl = nn.Module()
            sl.add_module(str(idx), nn.Conv2d(cin, cout, k, stride=st, padding=p))
            self.net.add_module(f"slice{s}", sl)
        for k, c in enumerate(CHNS):
            setattr(self, f"lin{k}", NetLinLayer(c))
        g = torch.Generator().manual_seed(0)
        with torch.no_grad():
            for conv in self._convs():
                fan_in = conv.weight.shape[1] * conv.weight.shape[2] * conv.weight.shape[3]
                conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * (2.0 / fan_in) ** 0.5)
                conv.bias.copy_(0.1 * torch.randn(conv.bias.shape, generator=g))
            for k, c in enumerate(CHNS):
                w = self._lin(k)
                w.copy_(torch.rand(w.shape, generator=g) / c)
        if state_dict is not None:
            self.load_state_dict(state_dict, strict=True)
        self.requires_grad_(False)
        super().train(False)
        self.chunk = int(chunk)
        self.__dict__["_cache"] = None

    @classmethod
    def from_parts(cls, features_state_dict, lin_state_dict, **kw):
        """torchvision's ``alexnet().features.state_dict()`` (``0.weight`` ..., or with a ``features.`` prefix as in the full model's state
        dict; the classifier is ignored) plus the ``lpips`` package's linear-layer file (``lin{k}.model.1.weight``)."""
        m = cls(**kw)
        sd = OrderedDict()
        for s, idx, *_ in ALEX_CONVS:
            for leaf in ("weight", "bias"):
                for key in (f"features.{idx}.{leaf}", f"{idx}.{leaf}"):
                    if key in features_state_dict:
                        sd[f"net.slice{s}.{idx}.{leaf}"] = features_state_dict[key]
                        break
                else:
                    raise KeyError(f"LpipsAlex.from_parts: features.{idx}.{leaf} is missing from the features state dict")
        for k in range(5):
            key = f"lin{k}.model.1.weight"
            if key not in lin_state_dict:
                raise KeyError(f"LpipsAlex.from_parts: {key} is missing from the linear-layer state dict")
            sd[key] = lin_state_dict[key]
        sd["scaling_layer.shift"], sd["scaling_layer.scale"] = m.scaling_layer.shift, m.scaling_layer.scale
        m.load_state_dict(sd, strict=True)
        return m

    # ---- module plumbing ---------------------------------------------------------------------------------------------------------
    def _convs(self):
        return [getattr(getattr(self.net, f"slice{s}"), str(idx)) for s, idx, *_ in ALEX_CONVS]

    def _lin(self, k):
        return getattr(getattr(self, f"lin{k}").model, "1").weight

    def train(self, mode: bool = True):
        """Always in eval mode, whatever the trainer sets on the modules around it."""
        return super().train(False)

    def _prepare(self, device):
        """Weight rows for the kernels (tap-major, channel-minor), rebuilt when a parameter or the device changed; the input affine of both
        ``normalize`` settings."""
        from fourm.utils.inception.model import pack_weight
        params = list(self.parameters()) + [self.scaling_layer.shift, self.scaling_layer.scale]
        if params[0].device != device:
            raise RuntimeError(f"input on {device}, LpipsAlex on {params[0].device}")
        stamp = (device, tuple((p._version, p.data_ptr()) for p in params))
        c = self._cache
        if c is not None and c["stamp"] == stamp:
            return c
        with torch.no_grad():
            convs = self._convs()
            c = dict(stamp=stamp, w=[pack_weight(cv.weight.detach().float()) for cv in convs], bias=[cv.bias.detach().float().contiguous() for cv in convs],
                     lin=[self._lin(k).detach().reshape(-1).float().contiguous() for k in range(5)], affine={})
            for normalize in (False, True):
                mul, add = fold_input_affine(self.scaling_layer.shift, self.scaling_layer.scale, normalize)
                c["affine"][normalize] = (mul.float().to(device), add.float().to(device))
        self.__dict__["_cache"] = c
        return c

    # ---- forward ------------------------------------------------------------------------------------------------------------------
    def _check(self, img0, img1):
        for t in (img0, img1):
            if not torch.is_tensor(t) or t.dim() != 4 or t.shape[1] != 3 or t.shape[0] < 1:
                raise ValueError(f"LpipsAlex: images (N, 3, H, W) expected, got {tuple(t.shape) if torch.is_tensor(t) else type(t).__name__}")
        if img0.shape != img1.shape:
            raise ValueError(f"LpipsAlex: img0 {tuple(img0.shape)} and img1 {tuple(img1.shape)} differ in shape")
        H, W = img0.shape[-2:]
        if H < MIN_SIZE or W < MIN_SIZE:
            raise ValueError(f"LpipsAlex: images of {H} x {W}: both sides have to be at least {MIN_SIZE} (the two 3 x 3 max-pools of AlexNet)")
        for t in (img0, img1):
            if t.dtype not in (torch.float32, torch.bfloat16, torch.float16):
                raise TypeError(f"LpipsAlex: images of dtype {t.dtype}: fp32, bf16 or fp16 expected")
        if not (img0.is_cuda and img1.is_cuda):
            raise RuntimeError("LpipsAlex computes on an MI355X through libfourm_hip.so; move the images and the module to the GPU first (there is no CPU path)")

    def _taps(self, c, img, normalize, clamp):
        """One batch of images through the five layers -> [(rows (B*H*W, C), H, W)] of the five taps."""
        ops = _iops()
        B, _, H, W = img.shape
        mul, add = c["affine"][bool(normalize)]
        taps = []
        for li, (_, _, _, _, k, st, p) in enumerate(ALEX_CONVS):
            if li == 0:
                x = conv2d_stem(img, c["w"][0], c["bias"][0], k, k, st, p, mul, add, clamp, True)
            else:
                x = ops.conv2d_nhwc(x, B, H, W, c["w"][li], c["bias"][li], k, k, st, (p, p), True)
            H, W = ops.conv_out_size(H, k, st, p), ops.conv_out_size(W, k, st, p)
            taps.append((x, H, W))
            if li < 2:
                x = ops.pool2d_nhwc(x, B, H, W, "max_s2")
                H, W = ops.pool_out_size("max_s2", H, W)
        return taps

    def scores(self, img0, img1, normalize, clamp0=False, chunk=None):
        self._check(img0, img1)
        chunk = self.chunk if chunk is None else int(chunk)
        if chunk < 1:
            raise ValueError(f"LpipsAlex: chunk={chunk}")
        B = img0.shape[0]
        clamp = ((0.0, 1.0) if normalize else (-1.0, 1.0)) if clamp0 else None
        with torch.no_grad(), torch.cuda.device(img0.device):
            c = self._prepare(img0.device)
            out = torch.empty(B, dtype=torch.float32, device=img0.device)
            for b0 in range(0, B, chunk):
                x0, x1 = img0[b0:b0 + chunk].detach().float().contiguous(), img1[b0:b0 + chunk].detach().float().contiguous()
                n = x0.shape[0]
                t0, t1 = self._taps(c, x0, normalize, clamp), self._taps(c, x1, normalize, None)
                score = torch.zeros(n, dtype=torch.float32, device=img0.device)
                for k in range(5):
                    (fa, H, W), (fb, _, _) = t0[k], t1[k]
                    lpips_score(fa, fb, c["lin"][k], n, H * W, score)
                out[b0:b0 + n] = score
        return out

    def forward(self, img0, img1, normalize=False):
        return self.scores(img0, img1, normalize)
