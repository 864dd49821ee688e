"""The C entry points of csrc/inception.hip on torch tensors (include/fourm_hip.h, "Inception tower").  A feature map is a 2-D fp32 tensor of
NHWC rows ``(B * H * W, C)`` whose row stride may exceed ``C`` (a column slice of a wider buffer): concatenations are written in place."""
import ctypes as C

import numpy as np
import torch

SIZE = 299                      # FM_INCEPTION_SIZE
POOL_MODES = ("max_s2", "max_s1p1", "avg_s1p1", "global_avg")      # FM_POOL_* in order


def _lib():
    from ...hip import _lib as L
    return L


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _rows(t, what, dtype=torch.float32):
    if not torch.is_tensor(t):
        raise TypeError(f"{what}: a tensor is expected, got {type(t).__name__}")
    if t.dtype != dtype:
        raise TypeError(f"{what}: {dtype} expected, got {t.dtype}")
    if not t.is_cuda:
        raise RuntimeError(f"{what}: the tensor is on {t.device}; the Inception kernels run on an MI355X only (there is no CPU path)")
    if t.dim() != 2 or t.stride(1) != 1 or t.stride(0) < t.shape[1]:
        raise ValueError(f"{what}: 2-D rows with contiguous columns expected, got shape {tuple(t.shape)} strides {tuple(t.stride())}")
    return t


def conv_out_size(size, k, stride, pad):
    return (size + 2 * pad - k) // stride + 1


def conv2d_nhwc(x, B, H, W, weight, bias, KH, KW, stride=1, pad=(0, 0), relu=True, out=None):
    """fm_conv2d_nhwc_f32.  x rows (B*H*W, Cin); weight (Cout, KH*KW*Cin) tap-major, channel-minor; bias (Cout,) or None.  Writes (and
    returns) ``out`` rows (B*Ho*Wo, Cout) - a column slice of a wider buffer is filled in place."""
    L = _lib()
    x, weight = _rows(x, "conv2d_nhwc: x"), _rows(weight, "conv2d_nhwc: weight")
    Cin, Cout = x.shape[1], weight.shape[0]
    if x.shape[0] != B * H * W or weight.shape[1] != KH * KW * Cin:
        raise ValueError(f"conv2d_nhwc: x {tuple(x.shape)} / weight {tuple(weight.shape)} do not fit B={B} H={H} W={W} KH={KH} KW={KW}")
    if bias is not None and (bias.dtype != torch.float32 or not bias.is_cuda or bias.numel() != Cout or not bias.is_contiguous()):
        raise ValueError("conv2d_nhwc: bias must be a contiguous fp32 (Cout,) tensor on the GPU")
    Ho, Wo = conv_out_size(H, KH, stride, pad[0]), conv_out_size(W, KW, stride, pad[1])
    if Ho < 1 or Wo < 1:
        raise ValueError(f"conv2d_nhwc: the {KH} x {KW} kernel does not fit the padded {H} x {W} map")
    if out is None:
        out = torch.empty(B * Ho * Wo, Cout, dtype=torch.float32, device=x.device)
    out = _rows(out, "conv2d_nhwc: out")
    if tuple(out.shape) != (B * Ho * Wo, Cout):
        raise ValueError(f"conv2d_nhwc: out {tuple(out.shape)}, expected {(B * Ho * Wo, Cout)}")
    a = L.Conv2dArgs(x=_p(x), w=_p(weight), bias=_p(bias), out=_p(out), B=B, H=H, W=W, Cin=Cin, Cout=Cout, KH=KH, KW=KW, stride=stride,
                     pad_h=pad[0], pad_w=pad[1], ldx=x.stride(0), ldw=weight.stride(0), ldo=out.stride(0), relu=1 if relu else 0)
    with torch.cuda.device(x.device):
        L.check(L.conv2d_nhwc_f32(C.byref(a), _stream()))
    return out


def pool_out_size(mode, H, W):
    if mode == "max_s2":
        return (H - 3) // 2 + 1, (W - 3) // 2 + 1
    return (1, 1) if mode == "global_avg" else (H, W)


def pool2d_nhwc(x, B, H, W, mode, out=None):
    """fm_pool2d_nhwc_f32: ``mode`` one of POOL_MODES.  x rows (B*H*W, C) -> out rows (B*Ho*Wo, C) ((B, C) for ``global_avg``)."""
    L = _lib()
    x = _rows(x, "pool2d_nhwc: x")
    if mode not in POOL_MODES:
        raise ValueError(f"pool2d_nhwc: unknown mode {mode!r} (one of {', '.join(POOL_MODES)})")
    Cc = x.shape[1]
    if x.shape[0] != B * H * W:
        raise ValueError(f"pool2d_nhwc: x {tuple(x.shape)} does not fit B={B} H={H} W={W}")
    Ho, Wo = pool_out_size(mode, H, W)
    if Ho < 1 or Wo < 1:
        raise ValueError(f"pool2d_nhwc: the valid 3 x 3 window does not fit a {H} x {W} map")
    if out is None:
        out = torch.empty(B * Ho * Wo, Cc, dtype=torch.float32, device=x.device)
    out = _rows(out, "pool2d_nhwc: out")
    if tuple(out.shape) != (B * Ho * Wo, Cc):
        raise ValueError(f"pool2d_nhwc: out {tuple(out.shape)}, expected {(B * Ho * Wo, Cc)}")
    with torch.cuda.device(x.device):
        L.check(L.pool2d_nhwc_f32(_p(x), x.stride(0), _p(out), out.stride(0), B, H, W, Cc, POOL_MODES.index(mode), _stream()))
    return out


def resize_axis(n_in, n_out=SIZE):
    """The TF1-style bilinear axis table (no half-pixel offset): (i0, i1) int32 and w fp32, from s = n_in / n_out in double."""
    s = float(n_in) / float(n_out)
    src = np.arange(n_out, dtype=np.float64) * s
    i0 = np.floor(src)
    w = (src - i0).astype(np.float32)
    i0 = np.minimum(i0.astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    return i0.astype(np.int32), i1.astype(np.int32), w


_TABLES = {}


def _tables(H, W, device):
    key = (H, W, str(device))
    t = _TABLES.get(key)
    if t is None:
        y0, y1, wy = resize_axis(H)
        x0, x1, wx = resize_axis(W)
        idx = torch.from_numpy(np.stack([y0, y1, x0, x1])).to(device)
        wt = torch.from_numpy(np.stack([wy, wx])).to(device)
        if len(_TABLES) > 64:
            _TABLES.clear()
        t = _TABLES[key] = (idx.contiguous(), wt.contiguous())
    return t


def inception_preprocess(imgs, normalize=False, out=None):
    """fm_inception_preprocess: imgs (B, 3, H, W) uint8 (``normalize=False``) or fp32 in [0, 1] (``normalize=True``: the byte is
    trunc(255 v) clamped to [0, 255]) -> rows (B*299*299, 3) of the resized image in (v - 128) / 128."""
    L = _lib()
    if not torch.is_tensor(imgs):
        raise TypeError(f"inception_preprocess: a tensor is expected, got {type(imgs).__name__}")
    want = torch.float32 if normalize else torch.uint8
    if imgs.dtype != want:
        raise TypeError(f"inception_preprocess: {want} images expected with normalize={bool(normalize)}, got {imgs.dtype}")
    if imgs.dim() != 4 or imgs.shape[1] != 3 or imgs.shape[0] < 1 or imgs.shape[2] < 1 or imgs.shape[3] < 1:
        raise ValueError(f"inception_preprocess: images (B, 3, H, W) expected, got {tuple(imgs.shape)}")
    if not imgs.is_cuda:
        raise RuntimeError(f"inception_preprocess: the images are on {imgs.device}; the Inception kernels run on an MI355X only (there is no CPU path)")
    imgs = imgs.detach().contiguous()
    B, _, H, W = imgs.shape
    if out is None:
        out = torch.empty(B * SIZE * SIZE, 3, dtype=torch.float32, device=imgs.device)
    assert out.is_contiguous() and out.dtype == torch.float32 and tuple(out.shape) == (B * SIZE * SIZE, 3)
    idx, wt = _tables(H, W, imgs.device)
    with torch.cuda.device(imgs.device):
        L.check(L.inception_preprocess(_p(imgs), 1 if normalize else 0, B, H, W, _p(idx), _p(wt), _p(out), _stream()))
    return out


def feature_moments(feats, total, outer, count):
    """fm_feature_moments: total f64 (d,) += column sums, outer f64 (d, d) += feats^T feats, count int64 (1,) += n, for fp32 rows (n, d)."""
    L = _lib()
    feats = _rows(feats, "feature_moments: feats")
    n, d = feats.shape
    ok = total.dtype == outer.dtype == torch.float64 and count.dtype == torch.int64 and total.is_contiguous() and outer.is_contiguous() \
        and tuple(total.shape) == (d,) and tuple(outer.shape) == (d, d) and count.numel() == 1 \
        and total.device == outer.device == count.device == feats.device
    if not ok:
        raise ValueError(f"feature_moments: state of width {d} expected (sum f64 (d,), outer f64 (d, d), count int64 (1,)) on {feats.device}")
    if n == 0:
        return
    with torch.cuda.device(feats.device):
        L.check(L.feature_moments(_p(feats), feats.stride(0), n, d, _p(total), _p(outer), _p(count), _stream()))
