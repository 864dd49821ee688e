"""Differentiable image resize on the HIP engine: what upstream's tokenizer trainer does with ``F.interpolate`` on the device every iteration.

    resize_images     F.interpolate(x, size, mode='bilinear', align_corners=False[, antialias=True]) and mode='nearest', with an optional
                      per-channel affine folded into the same launch: y = scale[c] * R(x) + shift[c]; differentiable in x for the bilinear
                      modes (fm_resize_bilinear_fwd / fm_resize_bilinear_bwd, csrc/resize.hip); nearest also on int64 class maps

The contract is ``torch.nn.functional.interpolate`` on the CPU in float64 (a size is given, never a scale factor).  One axis of a bilinear
resize is a table - per output index a start, a count and the weights - made on the host in double by fm_resize_axis_table, rounded once to
fp32, and cached on the device.  The adjoint is a gather over the transposed table: no floating-point atomics, the same bits every time.

The table cache: one entry per (device, n_in, n_out, mode), built under a lock and NEVER replaced or evicted, so no launch in flight on any
stream can lose the buffer it reads (a single-entry cache did exactly that to a running GEMM once two sub-batches were in flight).  An entry
is published only after its blocking host-to-device copies have returned, so a launch on another stream that finds it reads finished data;
because of those copies the first use of a size pair cannot happen inside a hipGraph capture (use the sizes once before capturing).  Entries are
a few KiB; a trainer uses a handful of sizes.

Not here: bicubic, scale factors, align_corners=True.  The crop / flip augmentation of dataset pre-tokenization on 8-bit images (Pillow's bytes,
bicubic included) is ``fourm.data.crops``."""
import threading

import torch

MODES = ("bilinear", "nearest")
_TABLES = {}
_LOCK = threading.Lock()


def _mode_id(mode, antialias):
    from fourm.hip import _lib as L
    if mode not in MODES:
        raise ValueError(f"Unknown resize mode {mode!r}: one of {MODES} (bicubic is not built)")
    if antialias and mode != "bilinear":
        raise ValueError("antialias goes with mode='bilinear' only")
    return L.RESIZE_NEAREST if mode == "nearest" else L.RESIZE_BILINEAR_AA if antialias else L.RESIZE_BILINEAR


def axis_table(n_in, n_out, mode_id, device):
    """The cached table of one axis on ``device``: a dict of device tensors (start, count, weights, t_start, t_count) and the ints taps, t_taps."""
    from fourm.hip import ops
    device = torch.device(device)
    if device.index is None:
        device = torch.device(device.type, torch.cuda.current_device())
    key = (device, int(n_in), int(n_out), int(mode_id))
    hit = _TABLES.get(key)
    if hit is not None:
        return hit
    with _LOCK:
        hit = _TABLES.get(key)
        if hit is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f"resize {n_in} -> {n_out}: the axis table is not on the device yet and its upload cannot be captured - "
                                   "resize once at these sizes before capturing the graph")
            host = ops.resize_axis_table(int(n_in), int(n_out), int(mode_id))
            hit = {k: (v.to(device) if isinstance(v, torch.Tensor) and k != "weights_f64" else v) for k, v in host.items() if k != "weights_f64"}
            _TABLES[key] = hit          # (published after the blocking copies above)
    return hit


def _size2(size):
    if isinstance(size, int):
        return size, size
    size = tuple(int(s) for s in size)
    if len(size) != 2:
        raise ValueError(f"size: an int or (H, W), got {size}")
    return size


def _channel_vector(v, C, device, what):
    if v is None:
        return None
    v = torch.as_tensor(v, dtype=torch.float32).detach().to(device).reshape(-1).contiguous()
    if v.numel() != C:
        raise ValueError(f"{what}: one value per channel ({C}) expected, got {v.numel()}")
    return v


class _Bilinear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, th, tw, size, scale, shift):
        from fourm.hip import ops
        xc = x.detach().contiguous()
        y = torch.empty(xc.shape[0], xc.shape[1], size[0], size[1], dtype=torch.float32, device=xc.device)
        with torch.cuda.device(xc.device):
            ops.resize_bilinear_fwd(xc, y, th, tw, scale, shift)
        ctx.th, ctx.tw, ctx.scale, ctx.in_size = th, tw, scale, tuple(xc.shape)
        return y

    @staticmethod
    def backward(ctx, g):
        from fourm.hip import ops
        dy = g.detach().float().contiguous()
        dx = torch.empty(ctx.in_size, dtype=torch.float32, device=dy.device)
        with torch.cuda.device(dy.device):
            ops.resize_bilinear_bwd(dy, dx, ctx.th, ctx.tw, ctx.scale)
        return dx, None, None, None, None, None


def resize_images(x: torch.Tensor, size, mode: str = "bilinear", antialias: bool = False, scale=None, shift=None) -> torch.Tensor:
    """``F.interpolate(x, size, mode=mode, align_corners=False, antialias=antialias)`` on the HIP kernels, then ``* scale[c] + shift[c]`` in the
    same launch when a per-channel affine is given (both or neither; bilinear modes only).

    x: (B, C, H, W) fp32, or with ``mode='nearest'`` also an int64 (B, H, W) map.  size: an int or (H, W).  Differentiable in ``x`` for the
    bilinear modes (the affine's vectors get no gradient); nearest has no backward.  With the input's size and no affine the input itself is
    returned.  Tensors on the CPU raise RuntimeError: there is no CPU path."""
    from fourm.vq.training import _on_gpu
    mode_id = _mode_id(mode, antialias)
    if not isinstance(x, torch.Tensor):
        raise TypeError("resize_images: a tensor expected")
    _on_gpu("resize_images", x)
    Ho, Wo = _size2(size)
    if Ho <= 0 or Wo <= 0:
        raise ValueError(f"size {(Ho, Wo)}: positive sizes expected")
    if (scale is None) != (shift is None):
        raise ValueError("scale and shift come together")
    if mode == "nearest":
        if scale is not None:
            raise ValueError("mode='nearest' takes no affine")
        if not ((x.dtype == torch.float32 and x.dim() == 4) or (x.dtype == torch.int64 and x.dim() == 3)):
            raise TypeError(f"mode='nearest': fp32 (B, C, H, W) or int64 (B, H, W) expected, got {x.dtype} {tuple(x.shape)}")
        if x.requires_grad and torch.is_grad_enabled():
            raise NotImplementedError("mode='nearest' has no backward (detach the input)")
        Hi, Wi = x.shape[-2:]
        if (Hi, Wi) == (Ho, Wo):
            return x
        from fourm.hip import ops
        xc = x.detach().contiguous()
        y = torch.empty(*xc.shape[:-2], Ho, Wo, dtype=xc.dtype, device=xc.device)
        with torch.cuda.device(xc.device):
            ops.resize_nearest(xc, y, axis_table(Hi, Ho, mode_id, xc.device)["start"], axis_table(Wi, Wo, mode_id, xc.device)["start"])
        return y
    if x.dtype != torch.float32 or x.dim() != 4:
        raise TypeError(f"resize_images: fp32 images (B, C, H, W) expected, got {x.dtype} {tuple(x.shape)}")
    B, C, Hi, Wi = x.shape
    if (Hi, Wi) == (Ho, Wo) and scale is None:
        return x
    scale, shift = _channel_vector(scale, C, x.device, "scale"), _channel_vector(shift, C, x.device, "shift")
    th, tw = axis_table(Hi, Ho, mode_id, x.device), axis_table(Wi, Wo, mode_id, x.device)
    return _Bilinear.apply(x, th, tw, (Ho, Wo), scale, shift)
