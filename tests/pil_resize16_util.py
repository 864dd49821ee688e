"""Pillow's 16-bit ("I;16") crop + resize + flip and upstream's truncated depth standardisation restated in numpy and Python integers (the
contract of include/fourm_hip.h, "Pillow-exact 16-bit depth crops").  Independent of the library: the tests compare fm_pil_axis_table_f64,
fm_pil_crop_resize16 and fm_depth_standardize with this, and this with Pillow (live where it is installed, and through
tests/golden/depth_crops.npz everywhere) and with upstream's own function (recorded in the same file).

The resize: float64 coefficients (Python floats, one rounding per operation, Pillow's order), float64 accumulation tap by tap in order,
rounding half away from zero, the clamp per byte.  The statistics: Python big integers for M1, M2 and the variance numerator."""
import numpy as np

from tests import pil_resize_util as U8

FILTERS = U8.FILTERS


def nearest_index16(n, S):
    """int((o + 0.5) * a): Pillow sends I;16 through its generic affine transform, which evaluates every coordinate in closed form - not
    through the 8-bit affine scaler's repeated addition (pil_resize_util.nearest_index), from which it differs on some axes."""
    return U8.nearest_index_closed_form(n, S)


def axis_table_f64(n, S, filt):
    """(start int32 (S), count int32 (S), coef float64 (S, taps)) of one axis n -> S: the doubles the 8-bit table quantises."""
    assert filt in FILTERS and n >= 1 and S >= 1
    if n == S:
        return np.arange(S, dtype=np.int32), np.ones(S, np.int32), np.ones((S, 1), np.float64)
    if filt == "nearest":
        return nearest_index16(n, S), np.ones(S, np.int32), np.ones((S, 1), np.float64)
    f, fsup = (U8._bilinear, 1.0) if filt == "bilinear" else (U8._bicubic, 2.0)
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
        rows.append(k)
        start.append(xmin)
    taps = max(len(r) for r in rows)
    coef = np.zeros((S, taps), np.float64)
    for o, r in enumerate(rows):
        coef[o, :len(r)] = r
    return np.asarray(start, np.int32), np.asarray([len(r) for r in rows], np.int32), coef


def quantise(coef):
    """The 8-bit path's 22-bit fixed point of a float64 table."""
    return np.asarray([[int(-0.5 + v * (1 << 22)) if v < 0 else int(0.5 + v * (1 << 22)) for v in row] for row in coef.tolist()], np.int32)


def _clip8(v):
    return np.clip(v, 0, 255)


def _store(ss, plain_clamp):
    """float64 sums -> uint16 as Pillow stores them: r rounded half away from zero; low byte clip8(r % 256) with C's remainder sign, high byte
    clip8(r >> 8).  plain_clamp: clamp r to 0 .. 65535 instead - NOT Pillow; here so that the tests can show the difference."""
    r = np.where(ss < 0, ss - 0.5, ss + 0.5).astype(np.int64)          # astype truncates towards zero, as the C cast
    if plain_clamp:
        return np.clip(r, 0, 65535).astype(np.uint16)
    low = np.where(r < 0, -((-r) % 256), r % 256)
    return (_clip8(low) | (_clip8(r >> 8) << 8)).astype(np.uint16)


def _pass(x, table, axis, plain_clamp=False):
    """One 16-bit pass along ``axis`` of x uint16 (h, w)."""
    start, count, coef = table
    x = np.moveaxis(x, axis, 0).astype(np.float64)
    out = np.empty((len(start),) + x.shape[1:], np.uint16)
    for o in range(len(start)):
        ss = np.zeros(x.shape[1:], np.float64)
        for i in range(count[o]):
            ss = ss + x[start[o] + i] * coef[o, i]          # the product and the sum rounded separately
        out[o] = _store(ss, plain_clamp)
    return np.moveaxis(out, 0, axis)


def crop_resize16(img, setting, S, filt="bicubic", plain_clamp=False):
    """img uint16 (H, W); setting (top, left, h, w, flip) -> uint16 (S, S): the crop, the horizontal pass (rounded to uint16), the vertical
    pass, the flip.  An axis whose length is S is not resampled; ``nearest`` gathers on both axes (nearest_index16)."""
    top, left, h, w, flip = (int(v) for v in setting)
    H, W = img.shape
    if not (h >= 1 and w >= 1 and top >= 0 and left >= 0 and top + h <= H and left + w <= W):
        raise ValueError(f"box {(top, left, h, w)} leaves the {H} x {W} image")
    x = np.ascontiguousarray(img[top:top + h, left:left + w])
    if filt == "nearest":
        x = x[nearest_index16(h, S) if h != S else np.arange(S)][:, nearest_index16(w, S) if w != S else np.arange(S)]
    else:
        if w != S:
            x = _pass(x, axis_table_f64(w, S, filt), 1, plain_clamp)
        if h != S:
            x = _pass(x, axis_table_f64(h, S, filt), 0, plain_clamp)
    if flip:
        x = x[:, ::-1]
    return np.ascontiguousarray(x)


def pillow_crop_resize16(img, setting, S, filt="bicubic"):
    """The same through Pillow itself (needs Pillow), the image opened as mode I;16."""
    from PIL import Image
    top, left, h, w, flip = (int(v) for v in setting)
    H, W = img.shape
    pil = Image.frombytes("I;16", (W, H), np.ascontiguousarray(img).astype("<u2").tobytes())
    resample = {"nearest": Image.NEAREST, "bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC, None: None}[filt]
    res = pil.crop((left, top, left + w, top + h)).resize((S, S), resample)
    assert res.mode == "I;16"
    out = np.frombuffer(res.tobytes(), dtype="<u2").reshape(S, S).astype(np.uint16)
    return np.ascontiguousarray(out[:, ::-1] if flip else out)


def unit_f32(v):
    """float32 of v / 65535 in double: torch.Tensor(np.array(img) / (2 ** 16 - 1.0))."""
    return (np.asarray(v).astype(np.float64) / 65535.0).astype(np.float32)


def rank_range(n, thresh=0.1):
    """upstream's slice bounds, in Python doubles."""
    return int(thresh * n), int((1 - thresh) * n)


def truncated_stats(values):
    """values: integers 0 .. 65535 of one crop -> (mean32, var32) float32: exact integer moments of the sorted ranks lo .. hi - 1."""
    v = sorted(int(t) for t in np.asarray(values).reshape(-1))
    lo, hi = rank_range(len(v))
    m = hi - lo
    assert m >= 2
    M1 = sum(v[lo:hi])
    M2 = sum(t * t for t in v[lo:hi])
    mean = M1 / (m * 65535)          # int / int: correctly rounded
    var = float(m * M2 - M1 * M1) / float(m * (m - 1) * 65535 ** 2)          # each integer rounded once, then the quotient
    return np.float32(mean), np.float32(var)


def standardize(values):
    """values uint16 (S, S) -> (float32 (S, S), (mean32, var32)): (x - mean32) / sqrt(var32 + 1e-6) in float32 operations."""
    mean32, var32 = truncated_stats(values)
    x = unit_f32(values)
    sd = np.sqrt(np.float32(var32 + np.float32(1e-6)), dtype=np.float32)
    return ((x - mean32) / sd).astype(np.float32), (mean32, var32)


def ulp_distance(a, b):
    """Largest distance of two float32 arrays in units in the last place (ordered-integer distance; +0 and -0 coincide)."""
    def key(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return int(np.max(np.abs(key(a) - key(b)))) if np.size(a) else 0
