"""Pillow's 8-bit crop + resize + flip restated in numpy (the contract of include/fourm_hip.h, "Pillow-exact crops"): the coefficient tables
in Python floats (IEEE double, one rounding per operation, Pillow's order) and the two integer passes.  Independent of the library: the tests
compare fm_pil_axis_table and fm_pil_crop_resize with this, and this with Pillow (live where it is installed, and through
tests/golden/pil_crops.npz everywhere)."""
import numpy as np

PRECISION_BITS = 22
FILTERS = ("nearest", "bilinear", "bicubic")


def _bilinear(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def _bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def nearest_index(n, S):
    """Pillow's affine scaler: repeated addition of a = n / S starting at a / 2."""
    a = n / S
    xo = a * 0.5
    idx = []
    for _ in range(S):
        idx.append(min(int(xo), n - 1))
        xo += a
    return np.asarray(idx, dtype=np.int32)


def nearest_index_closed_form(n, S):
    """int((o + 0.5) * a): NOT Pillow's table (it differs on some axes); here so that the tests can pick those axes."""
    a = n / S
    return np.asarray([min(int((o + 0.5) * a), n - 1) for o in range(S)], dtype=np.int32)


def axis_table(n, S, filt):
    """(start int32 (S), count int32 (S), coef int32 (S, taps)) of one axis n -> S, rows padded with zeros.  ``nearest`` and n == S: one tap."""
    assert filt in FILTERS and n >= 1 and S >= 1
    if n == S:
        return np.arange(S, dtype=np.int32), np.ones(S, np.int32), np.full((S, 1), 1 << PRECISION_BITS, np.int32)
    if filt == "nearest":
        return nearest_index(n, S), np.ones(S, np.int32), np.full((S, 1), 1 << PRECISION_BITS, np.int32)
    f, fsup = (_bilinear, 1.0) if filt == "bilinear" else (_bicubic, 2.0)
    scale = n / S
    fs = max(scale, 1.0)
    support = fsup * fs
    ss = 1.0 / fs
    rows, start = [], []
    for o in range(S):
        center = (o + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n)
        k = [f((x + xmin - center + 0.5) * ss) for x in range(xmax - xmin)]
        ww = 0.0
        for v in k:
            ww += v
        if ww != 0.0:
            k = [v / ww for v in k]
        rows.append([int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS)) for v in k])
        start.append(xmin)
    taps = max(len(r) for r in rows)
    coef = np.zeros((S, taps), np.int32)
    for o, r in enumerate(rows):
        coef[o, :len(r)] = r
    return np.asarray(start, np.int32), np.asarray([len(r) for r in rows], np.int32), coef


def _pass(x, table, axis, stats=None):
    """One 8-bit pass along ``axis`` of x uint8 (h, w, C).  stats: a dict whose "lo" / "hi" collect the extremes of acc >> 22 before the clamp."""
    start, count, coef = table
    x = np.moveaxis(x, axis, 0).astype(np.int64)
    out = np.empty((len(start),) + x.shape[1:], np.uint8)
    for o in range(len(start)):
        acc = (1 << (PRECISION_BITS - 1)) + np.tensordot(coef[o, :count[o]].astype(np.int64), x[start[o]:start[o] + count[o]], axes=(0, 0))
        assert np.all(np.abs(acc) < 2 ** 31)          # the int32 accumulator of the C code does not wrap
        if stats is not None:
            stats["lo"] = min(stats.get("lo", 0), int((acc >> PRECISION_BITS).min()))
            stats["hi"] = max(stats.get("hi", 255), int((acc >> PRECISION_BITS).max()))
        out[o] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def crop_resize(img, setting, S, filt="bicubic", invert_on_flip=(), stats=None):
    """img uint8 (H, W, C); setting (top, left, h, w, flip) -> uint8 (S, S, C): the crop, the horizontal pass over its rows (rounded to uint8),
    the vertical pass, then the flip with ``255 - v`` on the channels of invert_on_flip."""
    top, left, h, w, flip = (int(v) for v in setting)
    H, W, _ = img.shape
    if not (h >= 1 and w >= 1 and top >= 0 and left >= 0 and top + h <= H and left + w <= W):
        raise ValueError(f"box {(top, left, h, w)} leaves the {H} x {W} image")
    x = np.ascontiguousarray(img[top:top + h, left:left + w])
    x = _pass(x, axis_table(w, S, filt), 1, stats)
    x = _pass(x, axis_table(h, S, filt), 0, stats)
    if flip:
        x = x[:, ::-1].copy()
        for c in invert_on_flip:
            x[..., c] = 255 - x[..., c]
    return np.ascontiguousarray(x)


PIL_MODES = {1: "L", 3: "RGB", 4: "CMYK"}          # four plain 8-bit planes: RGBA would be premultiplied around the resize


def pillow_crop_resize(img, setting, S, filt="bicubic", invert_on_flip=()):
    """The same through Pillow itself (needs Pillow; C in PIL_MODES)."""
    from PIL import Image
    top, left, h, w, flip = (int(v) for v in setting)
    C = img.shape[2]
    pil = Image.fromarray(img[..., 0] if C == 1 else img, mode=PIL_MODES[C])
    resample = {"nearest": Image.NEAREST, "bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC, None: None}[filt]
    out = np.asarray(pil.crop((left, top, left + w, top + h)).resize((S, S), resample)).reshape(S, S, C)
    if flip:
        out = out[:, ::-1].copy()
        for c in invert_on_flip:
            out[..., c] = 255 - out[..., c]
    return np.ascontiguousarray(out)
