"""The data stage of dataset pre-tokenization (upstream's save_vq_tokens.py) on the device: crop settings as upstream draws and stores them,
and the crops themselves - ``PIL.Image.crop`` + ``Image.resize`` + horizontal flip + ``to_tensor`` + ``normalize`` - byte for byte as Pillow's
8-bit path makes them (the contract is written out in include/fourm_hip.h, "Pillow-exact crops"; kernels in csrc/pil_resize.hip).

    center_crop_settings   CenterCropImageAugmenter's box (fourm/data/image_augmenter.py:101-125)
    random_crop_settings   RandomCropImageAugmenter's box and flip (:32-59): RandomResizedCrop.get_params, then random.random() < hflip
    make_crop_settings     the (n_crops, 5) array of save_vq_tokens.py:145-159: row 0 the unflipped centre crop, the rest random
    crop_resize            every crop of every image in one call: one pinned, packed host-to-device copy (job list, axis tables, lookup table,
                           image bytes), two launches
    decode_depth           a 16-bit depth PNG (Pillow mode I;16) as uint16 (H, W)
    crop_resize_depth      the same for depth maps: Pillow's 16-bit resample path (double accumulation, the clamp per byte) and upstream's
                           truncated depth standardisation per crop (include/fourm_hip.h, "Pillow-exact 16-bit depth crops"; kernels in
                           csrc/pil_resize16.hip)

Workspaces (the pinned staging buffer, its device image and the intermediates) are kept per (device, stream) and grow to the largest call;
a call waits for the previous upload from the same staging buffer before refilling it.  There is no CPU path."""
import math
import random
import threading

import numpy as np
import torch

RESAMPLE = {None: "bicubic", "bicubic": "bicubic", "bilinear": "bilinear", "nearest": "nearest"}          # None: Pillow's default
_FILTER_ID = {"nearest": 0, "bilinear": 1, "bicubic": 2}          # FM_PIL_*
_WS = {}
_WS_LOCK = threading.Lock()
_TABLES = {}
_TABLES_MAX = 4096


def center_crop_settings(H, W):
    """(top, left, h, w) of the largest centred square."""
    H, W = int(H), int(W)
    if H > W:
        return (H - W) // 2, 0, W, W
    return 0, (W - H) // 2, H, H


def random_crop_settings(H, W, scale=(0.2, 1.0), ratio=(0.75, 1.3333), hflip=0.5):
    """(top, left, h, w, flip): the torch and ``random`` calls of ``torchvision.transforms.RandomResizedCrop.get_params(img, scale, ratio)``
    in its order - ten attempts of (area uniform_, log-ratio uniform_, then two randint for an accepted box), else the central fallback -
    followed by ``random.random() < hflip``.  torchvision is not a dependency of this package and was not available to compare with: parity
    of the draw stream with upstream is NOT pinned by a test.  What is pinned: every box lies inside the image with scale and ratio in range,
    and the draws are reproducible under torch.manual_seed / random.seed."""
    H, W = int(H), int(W)
    area = H * W
    log_ratio = torch.log(torch.tensor(ratio))
    box = None
    for _ in range(10):
        target_area = area * torch.empty(1).uniform_(scale[0], scale[1]).item()
        aspect_ratio = torch.exp(torch.empty(1).uniform_(log_ratio[0], log_ratio[1])).item()
        w = int(round(math.sqrt(target_area * aspect_ratio)))
        h = int(round(math.sqrt(target_area / aspect_ratio)))
        if 0 < w <= W and 0 < h <= H:
            top = torch.randint(0, H - h + 1, size=(1,)).item()
            left = torch.randint(0, W - w + 1, size=(1,)).item()
            box = (top, left, h, w)
            break
    if box is None:          # central crop at the nearest allowed ratio
        in_ratio = float(W) / float(H)
        if in_ratio < min(ratio):
            w = W
            h = int(round(w / min(ratio)))
        elif in_ratio > max(ratio):
            h = H
            w = int(round(h * max(ratio)))
        else:
            w, h = W, H
        box = ((H - h) // 2, (W - w) // 2, h, w)
    flip = random.random() < hflip
    return (*box, 1 if flip else 0)


def make_crop_settings(H, W, n_crops=10, min_crop_scale=0.2):
    """The int array (n_crops, 5) of rows (top, left, h, w, flip) that upstream saves under crop_settings/: row 0 the unflipped centre crop
    (its augmenter draws one ``random.random()`` for a flip of probability 0, kept here so that the stream stays in step), rows 1 .. the
    random crops of scale (min_crop_scale, 1), ratio (0.75, 1.3333), flip 0.5."""
    random.random()
    rows = [(*center_crop_settings(H, W), 0)]
    for _ in range(1, int(n_crops)):
        rows.append(random_crop_settings(H, W, scale=(min_crop_scale, 1.0), ratio=(0.75, 1.3333), hflip=0.5))
    return np.array(rows)


def pil_axis_table(n, S, filt):
    """fm_pil_axis_table on the host -> one int32 array, start (S) | count (S) | coef (S, taps), and taps.  Cached per (n, S, filter)."""
    import ctypes as C
    from fourm.hip import _lib as L
    key = (int(n), int(S), filt)
    hit = _TABLES.get(key)
    if hit is not None:
        return hit
    fid = _FILTER_ID[filt]
    taps = L.pil_axis_table(key[0], key[1], fid, None, None, None)
    if taps < 1:
        L.check(-1)
    tab = np.zeros(key[1] * (2 + taps), np.int32)
    P = C.POINTER(C.c_int32)
    base = tab.ctypes.data
    if L.pil_axis_table(key[0], key[1], fid, C.cast(base, P), C.cast(base + 4 * key[1], P), C.cast(base + 8 * key[1], P)) != taps:
        L.check(-1)
    if len(_TABLES) >= _TABLES_MAX:
        _TABLES.clear()
    _TABLES[key] = (tab, taps)
    return tab, taps


def normalize_lut(C, mean, std):
    """float32 (C, 256): ``(arange(256) / 255 - mean[c]) / std[c]`` with torch's own fp32 ops - what to_tensor + normalize give for a byte."""
    mean = torch.as_tensor([0.0] * C if mean is None else mean, dtype=torch.float32).reshape(-1)
    std = torch.as_tensor([1.0] * C if std is None else std, dtype=torch.float32).reshape(-1)
    if mean.numel() != C or std.numel() != C:
        raise ValueError(f"mean / std: one value per channel ({C}) expected")
    v = torch.arange(256, dtype=torch.float32).div(255)
    return v[None, :].sub(mean[:, None]).div(std[:, None]).contiguous()


class _Workspace:
    def __init__(self):
        self.host = self.dev = self.mid = self.done = None

    def staging(self, nbytes, device):
        if self.done is not None:
            self.done.synchronize()          # the previous upload has left the pinned buffer
        if self.host is None or self.host.numel() < nbytes:
            cap = max(int(nbytes * 1.25), 1 << 16)
            self.host = torch.empty(cap, dtype=torch.uint8).pin_memory()
            self.dev = torch.empty(cap, dtype=torch.uint8, device=device)
        return self.host, self.dev

    def scratch(self, nbytes, device):
        if self.mid is None or self.mid.numel() < nbytes:
            self.mid = torch.empty(max(int(nbytes * 1.25), 1 << 16), dtype=torch.uint8, device=device)
        return self.mid


def _workspace(device):
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    with _WS_LOCK:
        ws = _WS.get(key)
        if ws is None:
            ws = _WS[key] = _Workspace()
    return ws


def _as_hwc(img, i):
    if isinstance(img, torch.Tensor):
        img = img.detach().cpu().numpy()
    img = np.asarray(img)
    if img.dtype != np.uint8:
        raise TypeError(f"image {i}: uint8 expected, got {img.dtype}")
    if img.ndim == 2:
        img = img[:, :, None]
    if img.ndim != 3 or not 1 <= img.shape[2] <= 4 or img.shape[0] < 1 or img.shape[1] < 1:
        raise ValueError(f"image {i}: (H, W, C) with 1 <= C <= 4 expected, got {img.shape}")
    return np.ascontiguousarray(img)


def _align(n, a):
    return (n + a - 1) // a * a


def _boxes(images, settings):
    """[(image, top, left, h, w, flip)] of every settings row, validated (ValueError) before the library sees a job."""
    boxes = []
    for i, (im, st) in enumerate(zip(images, settings)):
        st = np.asarray(st)
        if st.ndim != 2 or st.shape[1] != 5 or st.shape[0] < 1:
            raise ValueError(f"settings {i}: (n, 5) rows of (top, left, h, w, flip) expected, got {st.shape}")
        if not np.issubdtype(st.dtype, np.integer) and not np.array_equal(st, np.floor(st)):
            raise ValueError(f"settings {i}: integers expected")
        H, W = im.shape[:2]
        for top, left, h, w, flip in st.astype(np.int64).tolist():
            if not (h >= 1 and w >= 1 and top >= 0 and left >= 0 and top + h <= H and left + w <= W):
                raise ValueError(f"image {i}: box (top {top}, left {left}, h {h}, w {w}) leaves the {H} x {W} image")
            if flip not in (0, 1):
                raise ValueError(f"image {i}: flip {flip} (0 or 1)")
            boxes.append((i, top, left, h, w, flip))
    return boxes


def crop_resize(images, settings, size, resample=None, mean=None, std=None, invert_on_flip=(), out="float32"):
    """images: a list of uint8 (H, W, C) arrays or tensors of one channel count; settings: per image an (n_i, 5) array of rows
    (top, left, h, w, flip).  Returns the sum(n_i) crops at size x size in input order on the current device:

        out="uint8"    uint8 (N, size, size, C): Pillow's bytes
        out="float32"  float32 (N, C, size, size): (byte / 255 - mean[c]) / std[c] through a lookup table (mean 0, std 1 when not given)
        out="int64"    int64 (N, size, size): one-channel class maps, resample="nearest" only
        a tuple of these names returns a tuple of tensors from the same launches.

    resample: None (Pillow's default, bicubic), "bicubic", "bilinear", "nearest".  invert_on_flip: channels that become 255 - v in flipped
    crops.  A box that leaves its image raises ValueError before anything is launched; without a GPU RuntimeError (there is no CPU path)."""
    import ctypes as C_
    from fourm.hip import _lib as L
    if resample not in RESAMPLE:
        raise ValueError(f"resample {resample!r}: one of {list(RESAMPLE)}")
    filt = RESAMPLE[resample]
    outs = (out,) if isinstance(out, str) else tuple(out)
    if not outs or any(o not in ("float32", "uint8", "int64") for o in outs) or len(set(outs)) != len(outs):
        raise ValueError(f"out {out!r}: 'float32', 'uint8', 'int64' or a tuple of them")
    S = int(size)
    if not 1 <= S <= 16384:
        raise ValueError(f"size {size}: 1 .. 16384")
    images = [_as_hwc(im, i) for i, im in enumerate(images)]
    if len(images) == 0 or len(images) != len(settings):
        raise ValueError(f"{len(images)} images and {len(settings)} settings: one settings array per image, at least one image")
    C = images[0].shape[2]
    if any(im.shape[2] != C for im in images):
        raise ValueError("all images of a call have the same number of channels")
    if "int64" in outs and (C != 1 or filt != "nearest"):
        raise ValueError("out='int64' is for one-channel class maps with resample='nearest'")
    invert = 0
    for c in invert_on_flip:
        if not 0 <= int(c) < C:
            raise ValueError(f"invert_on_flip: channel {c} of {C}")
        invert |= 1 << int(c)
    lut = normalize_lut(C, mean, std) if "float32" in outs else None

    boxes = _boxes(images, settings)
    if not torch.cuda.is_available():
        raise RuntimeError("crop_resize runs on the HIP kernels only (an MI355X is needed; there is no CPU path)")
    device = torch.device("cuda", torch.cuda.current_device())

    # the packed buffer: jobs | tables | lookup table | images
    N = len(boxes)
    jobs = (L.PilCropJob * N)()
    tab_off, tabs, words = {}, [], 0
    for n in sorted({b[4] for b in boxes} | {b[3] for b in boxes}):          # identical (n, S, filter) axes share one table
        tab, taps = pil_axis_table(n, S, filt)
        tab_off[n] = (words, taps)
        tabs.append(tab)
        words += tab.size
    if words >= 1 << 31:
        raise ValueError("axis tables too large")
    src_off, nbytes = [], 0
    for im in images:
        src_off.append(nbytes)
        nbytes += im.size
    mid_bytes = blk_rows = blk_cols = 0
    per_cols = (S * S + 255) // 256
    for k, (i, top, left, h, w, flip) in enumerate(boxes):
        j = jobs[k]
        j.src_off, j.mid_off, j.out_slot, j.blk_rows, j.blk_cols = src_off[i], mid_bytes, k, blk_rows, blk_cols
        j.H, j.W = images[i].shape[:2]
        j.top, j.left, j.h, j.w, j.flip = top, left, h, w, flip
        (j.tab_w, j.taps_w), (j.tab_h, j.taps_h) = tab_off[w], tab_off[h]
        mid_bytes += h * S * C
        blk_rows += (h * S + 255) // 256
        blk_cols += per_cols
    o_jobs = 0
    o_tab = _align(C_.sizeof(jobs), 16)
    o_lut = _align(o_tab + 4 * words, 16)
    o_img = _align(o_lut + (4 * 256 * C if lut is not None else 0), 16)
    total = o_img + nbytes
    ws = _workspace(device)
    host, dev = ws.staging(total, device)
    hv = host.numpy()
    hv[o_jobs:o_jobs + C_.sizeof(jobs)] = np.frombuffer(jobs, dtype=np.uint8)
    hv[o_tab:o_tab + 4 * words] = np.concatenate(tabs).view(np.uint8)
    if lut is not None:
        hv[o_lut:o_lut + 4 * 256 * C] = lut.numpy().reshape(-1).view(np.uint8)
    for im, off in zip(images, src_off):
        hv[o_img + off:o_img + off + im.size] = im.reshape(-1)
    dev[:total].copy_(host[:total], non_blocking=True)
    ws.done = torch.cuda.Event()
    ws.done.record(torch.cuda.current_stream(device))
    mid = ws.scratch(mid_bytes, device)

    res = {}
    if "uint8" in outs:
        res["uint8"] = torch.empty(N, S, S, C, dtype=torch.uint8, device=device)
    if "float32" in outs:
        res["float32"] = torch.empty(N, C, S, S, dtype=torch.float32, device=device)
    if "int64" in outs:
        res["int64"] = torch.empty(N, S, S, dtype=torch.int64, device=device)
    base = dev.data_ptr()
    ptr = lambda t: C_.c_void_p(t.data_ptr()) if t is not None else None
    with torch.cuda.device(device):
        L.check(L.pil_crop_resize(jobs, C_.c_void_p(base + o_jobs), N, C_.c_void_p(base + o_img), nbytes, C_.c_void_p(base + o_tab), words, ptr(mid), mid.numel(),
                                  C, S, invert, C_.c_void_p(base + o_lut) if lut is not None else None, ptr(res.get("uint8")), ptr(res.get("float32")),
                                  ptr(res.get("int64")), N, C_.c_void_p(torch.cuda.current_stream(device).cuda_stream)))
    return res[out] if isinstance(out, str) else tuple(res[o] for o in outs)


# ---- 16-bit depth ---------------------------------------------------------------------------------------------------------------------------
_TABLES_F64 = {}


def decode_depth(path):
    """A 16-bit depth PNG -> uint16 (H, W).  Pillow opens it as mode ``I;16``; any other mode (``I``, ``F``, big-endian ``I;16B``, an 8-bit
    file) raises ValueError naming the mode: those do not go through Pillow's 16-bit resample path, which is the one restated here."""
    from PIL import Image
    with Image.open(path) as img:
        if img.mode != "I;16":
            raise ValueError(f"{path}: mode {img.mode!r}, expected a 16-bit grayscale image (mode 'I;16')")
        W, H = img.size
        return np.frombuffer(img.tobytes(), dtype="<u2").reshape(H, W).astype(np.uint16)


def pil_axis_table_f64(n, S, filt):
    """fm_pil_axis_table_f64 on the host -> one int32 array of S (2 + 2 taps) words, start (S) | count (S) | coef float64 (S, taps), and taps.
    Cached per (n, S, filter)."""
    import ctypes as C
    from fourm.hip import _lib as L
    key = (int(n), int(S), filt)
    hit = _TABLES_F64.get(key)
    if hit is not None:
        return hit
    fid = _FILTER_ID[filt]
    taps = L.pil_axis_table_f64(key[0], key[1], fid, None, None, None)
    if taps < 1:
        L.check(-1)
    tab = np.zeros(key[1] * (2 + 2 * taps), np.int32)
    P = C.POINTER(C.c_int32)
    base = tab.ctypes.data
    if L.pil_axis_table_f64(key[0], key[1], fid, C.cast(base, P), C.cast(base + 4 * key[1], P), C.cast(base + 8 * key[1], C.POINTER(C.c_double))) != taps:
        L.check(-1)
    if len(_TABLES_F64) >= _TABLES_MAX:
        _TABLES_F64.clear()
    _TABLES_F64[key] = (tab, taps)
    return tab, taps


def _as_hw16(img, i):
    if isinstance(img, torch.Tensor):
        img = img.detach().cpu().numpy()
    img = np.asarray(img)
    if img.dtype != np.uint16:
        raise TypeError(f"image {i}: uint16 expected, got {img.dtype}")
    if img.ndim == 3 and img.shape[2] == 1:
        img = img[:, :, 0]
    if img.ndim != 2 or img.shape[0] < 1 or img.shape[1] < 1:
        raise ValueError(f"image {i}: (H, W) expected, got {img.shape}")
    return np.ascontiguousarray(img)


def crop_resize_depth(images, settings, size, resample=None, standardize=True, out="float32", return_stats=False):
    """images: a list of uint16 (H, W) depth maps (``decode_depth``); settings: per image an (n_i, 5) array of rows (top, left, h, w, flip),
    as for ``crop_resize``.  Returns the sum(n_i) crops at size x size in input order on the current device, as Pillow's 16-bit resample
    path and upstream's DepthTransform make them (include/fourm_hip.h, "Pillow-exact 16-bit depth crops"):

        out="uint16"   int32 (N, size, size): Pillow's 16-bit values (torch has no arithmetic on uint16)
        out="float32"  float32 (N, 1, size, size): v / 65535, and with standardize=True upstream's truncated_depth_standardization of
                       each crop: (x - mean) / sqrt(var + 1e-6), mean and unbiased variance over the sorted ranks int(0.1 n) .. int(0.9 n) - 1
        a tuple of these names returns a tuple of tensors from the same launches.

    return_stats=True (standardize=True only) appends the float32 (N, 2) tensor of (mean, var) per crop.  The same errors before any launch
    as ``crop_resize``; size < 2 with standardize=True raises ValueError (the truncated range has fewer than two elements)."""
    import ctypes as C_
    from fourm.hip import _lib as L
    if resample not in RESAMPLE:
        raise ValueError(f"resample {resample!r}: one of {list(RESAMPLE)}")
    filt = RESAMPLE[resample]
    outs = (out,) if isinstance(out, str) else tuple(out)
    if not outs or any(o not in ("float32", "uint16") for o in outs) or len(set(outs)) != len(outs):
        raise ValueError(f"out {out!r}: 'float32', 'uint16' or a tuple of them")
    S = int(size)
    if not 1 <= S <= 16384:
        raise ValueError(f"size {size}: 1 .. 16384")
    standardize = bool(standardize) and "float32" in outs
    n = S * S
    lo, hi = int(0.1 * n), int((1 - 0.1) * n)          # upstream's slice bounds, in Python doubles
    if standardize and hi - lo < 2:
        raise ValueError(f"size {size}: the truncated range [{lo}, {hi}) of {n} values has fewer than two elements (standardize=True needs size >= 2)")
    if return_stats and not standardize:
        raise ValueError("return_stats=True needs standardize=True and out 'float32'")
    images = [_as_hw16(im, i) for i, im in enumerate(images)]
    if len(images) == 0 or len(images) != len(settings):
        raise ValueError(f"{len(images)} images and {len(settings)} settings: one settings array per image, at least one image")

    boxes = _boxes(images, settings)
    if not torch.cuda.is_available():
        raise RuntimeError("crop_resize_depth runs on the HIP kernels only (an MI355X is needed; there is no CPU path)")
    device = torch.device("cuda", torch.cuda.current_device())

    # the packed buffer: jobs | tables | images
    N = len(boxes)
    jobs = (L.PilCropJob * N)()
    tab_off, tabs, words = {}, [], 0
    for m in sorted({b[4] for b in boxes} | {b[3] for b in boxes}):
        tab, taps = pil_axis_table_f64(m, S, filt)
        tab_off[m] = (words, taps)
        tabs.append(tab)
        words += tab.size          # S (2 + 2 taps): even, the doubles stay 8-byte aligned
    if words >= 1 << 31:
        raise ValueError("axis tables too large")
    src_off, nbytes = [], 0
    for im in images:
        src_off.append(nbytes)
        nbytes += 2 * im.size
    mid_bytes = blk_rows = blk_cols = 0
    per_cols = (S * S + 255) // 256
    for k, (i, top, left, h, w, flip) in enumerate(boxes):
        j = jobs[k]
        j.src_off, j.mid_off, j.out_slot, j.blk_rows, j.blk_cols = src_off[i], mid_bytes, k, blk_rows, blk_cols
        j.H, j.W = images[i].shape
        j.top, j.left, j.h, j.w, j.flip = top, left, h, w, flip
        (j.tab_w, j.taps_w), (j.tab_h, j.taps_h) = tab_off[w], tab_off[h]
        mid_bytes += 2 * h * S
        blk_rows += (h * S + 255) // 256
        blk_cols += per_cols
    o_jobs = 0
    o_tab = _align(C_.sizeof(jobs), 16)
    o_img = _align(o_tab + 4 * words, 16)
    total = o_img + nbytes
    ws = _workspace(device)
    host, dev = ws.staging(total, device)
    hv = host.numpy()
    hv[o_jobs:o_jobs + C_.sizeof(jobs)] = np.frombuffer(jobs, dtype=np.uint8)
    hv[o_tab:o_tab + 4 * words] = np.concatenate(tabs).view(np.uint8)
    for im, off in zip(images, src_off):
        hv[o_img + off:o_img + off + 2 * im.size] = im.reshape(-1).view(np.uint8)
    dev[:total].copy_(host[:total], non_blocking=True)
    ws.done = torch.cuda.Event()
    ws.done.record(torch.cuda.current_stream(device))
    mid = ws.scratch(mid_bytes, device)

    res = {}
    need_values = "uint16" in outs or standardize          # the standardisation reads the integer values
    values = torch.empty(N, S, S, dtype=torch.int32, device=device) if need_values else None
    if "uint16" in outs:
        res["uint16"] = values
    if "float32" in outs:
        res["float32"] = torch.empty(N, 1, S, S, dtype=torch.float32, device=device)
    stats = torch.empty(N, 2, dtype=torch.float32, device=device) if return_stats else None
    base = dev.data_ptr()
    ptr = lambda t: C_.c_void_p(t.data_ptr()) if t is not None else None
    stream = C_.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    with torch.cuda.device(device):
        L.check(L.pil_crop_resize16(jobs, C_.c_void_p(base + o_jobs), N, C_.c_void_p(base + o_img), nbytes, C_.c_void_p(base + o_tab), words, ptr(mid), mid.numel(),
                                    S, ptr(values), None if standardize else ptr(res.get("float32")), N, stream))
        if standardize:
            L.check(L.depth_standardize(ptr(values), N, n, lo, hi, ptr(res["float32"]), ptr(stats), stream))
    got = tuple(res[o] for o in outs)
    if return_stats:
        return (*got, stats)
    return got[0] if isinstance(out, str) else got
