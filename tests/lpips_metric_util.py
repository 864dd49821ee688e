"""The definitions behind the LPIPS validation metric ("LPIPS validation metric") restated in plain torch on the CPU: AlexNet's
five convolutions as F.conv2d + ReLU with F.max_pool2d(3, 2) behind the first two, the input scaling, the per-pixel normalisation
a / sqrt(eps + sum a^2), the weighted squared difference and the spatial mean.  Evaluated in float64 it is the reference; the same code at
dtype=torch.float32 gives the comparison baseline.  Nothing here looks at what the kernels return, and nothing is imported from the package.

Bounds, from the formats (U = 2^-24, the fp32 unit roundoff):
    stem      (K + 4) U (sum |s||w| + |bias|), K = KH KW Cin: the K-term fp32 chain, the bias add, the rounding of s = fmaf(v, mul, add) and
              second-order terms.
    score     4 x the error of this restatement in fp32 against float64 on the same inputs + 4 fp32 ulps of the value (FACTOR, FLOOR_ULPS:
              the TOWER_FACTOR / TOWER_FLOOR_ULPS margin of tests/inception_util.py).  The same rule end to end."""
import functools
import math
from collections import OrderedDict

import torch
import torch.nn.functional as F

U = 2.0 ** -24
EPS = 1e-8
FACTOR = 4.0
FLOOR_ULPS = 4.0
SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
# (slice, index in torchvision's alexnet.features, Cin, Cout, kernel, stride, padding)
CONVS = ((1, 0, 3, 64, 11, 4, 2), (2, 3, 64, 192, 5, 1, 2), (3, 6, 192, 384, 3, 1, 1), (4, 8, 384, 256, 3, 1, 1), (5, 10, 256, 256, 3, 1, 1))
CHNS = (64, 192, 384, 256, 256)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def state_dict_shapes():
    S = OrderedDict()
    S["scaling_layer.shift"] = (1, 3, 1, 1)
    S["scaling_layer.scale"] = (1, 3, 1, 1)
    for s, idx, cin, cout, k, _, _ in CONVS:
        S[f"net.slice{s}.{idx}.weight"] = (cout, cin, k, k)
        S[f"net.slice{s}.{idx}.bias"] = (cout,)
    for i, c in enumerate(CHNS):
        S[f"lin{i}.model.1.weight"] = (1, c, 1, 1)
    return S


def seeded_state_dict(seed=5):
    """He-scaled convolutions, small biases, positive lin weights of mean 1 / (2 C)."""
    g = gen(seed)
    sd = OrderedDict()
    sd["scaling_layer.shift"] = torch.tensor(SHIFT)[None, :, None, None]
    sd["scaling_layer.scale"] = torch.tensor(SCALE)[None, :, None, None]
    for s, idx, cin, cout, k, _, _ in CONVS:
        sd[f"net.slice{s}.{idx}.weight"] = torch.randn(cout, cin, k, k, generator=g) * math.sqrt(2.0 / (cin * k * k))
        sd[f"net.slice{s}.{idx}.bias"] = 0.1 * torch.randn(cout, generator=g)
    for i, c in enumerate(CHNS):
        sd[f"lin{i}.model.1.weight"] = torch.rand(1, c, 1, 1, generator=g) / c
    return sd


def parts(sd):
    """The same weights under torchvision's ``features.*`` names and the ``lpips`` package's lin file."""
    feats = OrderedDict()
    for s, idx, *_ in CONVS:
        for leaf in ("weight", "bias"):
            feats[f"features.{idx}.{leaf}"] = sd[f"net.slice{s}.{idx}.{leaf}"]
    lins = OrderedDict((k, v) for k, v in sd.items() if k.startswith("lin"))
    return feats, lins


def images(B, H, W, seed, lo=0.0, hi=1.0):
    """A smooth random field plus noise in [lo, hi]."""
    g = gen(seed)
    coarse = torch.rand(B, 3, 5, 4, generator=g)
    field = F.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=False)
    v = (0.7 * field + 0.3 * torch.rand(B, 3, H, W, generator=g)).clamp(0, 1)
    return (lo + (hi - lo) * v).float()


def to_rows(x):
    """(B, C, H, W) -> NHWC rows (B*H*W, C)."""
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]).contiguous()


def taps(sd, img, normalize, dtype, clamp=None):
    """img (B, 3, H, W) -> the five tap maps (B, C, h, w) in ``dtype``."""
    x = img.to(dtype)
    if clamp is not None:
        x = x.clamp(clamp[0], clamp[1])
    if normalize:
        x = 2 * x - 1
    x = (x - sd["scaling_layer.shift"].to(dtype)) / sd["scaling_layer.scale"].to(dtype)
    out = []
    for li, (s, idx, _, _, _, st, p) in enumerate(CONVS):
        x = F.relu(F.conv2d(x, sd[f"net.slice{s}.{idx}.weight"].to(dtype), sd[f"net.slice{s}.{idx}.bias"].to(dtype), stride=st, padding=p))
        out.append(x)
        if li < 2:
            x = F.max_pool2d(x, 3, 2)
    return out


def layer_score(a, b, w, eps=EPS):
    """a, b (B, C, h, w), w (C,) -> (B,): mean over the pixels of sum_c w_c (a^ - b^)^2, a^ = a / sqrt(eps + sum_c a_c^2)."""
    na = torch.sqrt(eps + (a * a).sum(dim=1, keepdim=True))
    nb = torch.sqrt(eps + (b * b).sum(dim=1, keepdim=True))
    d = (a / na - b / nb) ** 2
    return (d * w.reshape(1, -1, 1, 1)).sum(dim=1).mean(dim=(1, 2))


def rows_score(a, b, w, B, P, dtype, eps=EPS):
    """layer_score on rows (B*P, C)."""
    def img(t):
        return t.to(dtype).reshape(B, P, 1, -1).permute(0, 3, 1, 2)
    return layer_score(img(a), img(b), w.to(dtype), eps)


def lpips(sd, img0, img1, normalize, dtype, clamp0=None):
    """-> (B,) in ``dtype``: the five layer scores added in tap order."""
    t0, t1 = taps(sd, img0, normalize, dtype, clamp0), taps(sd, img1, normalize, dtype)
    total = None
    for k in range(5):
        s = layer_score(t0[k], t1[k], sd[f"lin{k}.model.1.weight"].to(dtype).reshape(-1))
        total = s if total is None else total + s
    return total


def tol(ref64, ref32):
    """-> (bound, base) on the absolute error of every element: FACTOR x the fp32 restatement's own worst error + FLOOR_ULPS fp32 ulps of
    the largest value."""
    base = float((ref32.double() - ref64).abs().max())
    return FACTOR * base + FLOOR_ULPS * 2.0 ** -23 * float(ref64.abs().max()), base


@functools.lru_cache(maxsize=4)
def fixture(B, H, W, normalize):
    """Shared and never modified: seeded weights, an image pair (the second a perturbed copy of the first: a distance well inside (0, 1)), and
    the float64 / fp32 restatement on it."""
    sd = seeded_state_dict()
    lo, hi = (0.0, 1.0) if normalize else (-1.0, 1.0)
    img0 = images(B, H, W, 100 + H + W, lo, hi)
    img1 = (img0 + 0.25 * (hi - lo) * (torch.rand(img0.shape, generator=gen(7 + H)) - 0.5)).clamp(lo, hi)
    with torch.no_grad():
        ref64 = lpips(sd, img0, img1, normalize, torch.float64)
        ref32 = lpips(sd, img0, img1, normalize, torch.float32)
    return dict(sd=sd, img0=img0, img1=img1, ref64=ref64, ref32=ref32)
