"""The definitions behind fourm.utils.inception ("FID and Inception score") restated in plain torch on the CPU: the FID variant
of InceptionV3 as F.conv2d + batch norm + ReLU with F.max_pool2d / F.avg_pool2d(count_include_pad=False), the TF1-style bilinear resize, FID by
two float64 routes and the Inception score.  Evaluated in float64 it is the reference; the same graph at dtype=torch.float32 gives the comparison
baseline of the end-to-end test.  Nothing here looks at what the kernels return, and nothing is imported from the package.

Bounds, from the formats (U = 2^-24, the fp32 unit roundoff):
    conv      (K + 2) U (sum |x||w| + |bias|): a K-term fp32 chain (K U sum|x w| to first order, doubled terms covered by the + 2) and the bias add.
    avg pool  10 U max|x|: 8 adds, the reciprocal and the multiply.       global avg  (HW + 1) U mean|x|.
    resize    8 U 255 on the 0..255 scale: six roundings of the two lerp levels plus two weight roundings.
    tower     4 x the error of this restatement in fp32 against float64 + 4 fp32 ulps (TOWER_FACTOR, TOWER_FLOOR_ULPS: the margin of the
              SSIM tests, tests/vq_metrics_util.py)."""
import functools
import math
from collections import OrderedDict

import torch
import torch.nn.functional as F

U = 2.0 ** -24
SIZE = 299
BN_EPS = 1e-3
TOWER_FACTOR = 4.0
TOWER_FLOOR_ULPS = 4.0
FIXTURE_SEED = 7
GEOMETRY = (299, 149, 147, 73, 71, 35, 17, 8)
WIDTHS = (256, 288, 288, 768, 1280, 2048)


def gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- the unit table: name -> (Cin, Cout, KH, KW, stride, pad_h, pad_w) ----------------------------------------------------------------------
def unit_table():
    T = OrderedDict()
    T["Conv2d_1a_3x3"] = (3, 32, 3, 3, 2, 0, 0)
    T["Conv2d_2a_3x3"] = (32, 32, 3, 3, 1, 0, 0)
    T["Conv2d_2b_3x3"] = (32, 64, 3, 3, 1, 1, 1)
    T["Conv2d_3b_1x1"] = (64, 80, 1, 1, 1, 0, 0)
    T["Conv2d_4a_3x3"] = (80, 192, 3, 3, 1, 0, 0)
    for blk, cin, pf in (("Mixed_5b", 192, 32), ("Mixed_5c", 256, 64), ("Mixed_5d", 288, 64)):
        T[f"{blk}.branch1x1"] = (cin, 64, 1, 1, 1, 0, 0)
        T[f"{blk}.branch5x5_1"] = (cin, 48, 1, 1, 1, 0, 0)
        T[f"{blk}.branch5x5_2"] = (48, 64, 5, 5, 1, 2, 2)
        T[f"{blk}.branch3x3dbl_1"] = (cin, 64, 1, 1, 1, 0, 0)
        T[f"{blk}.branch3x3dbl_2"] = (64, 96, 3, 3, 1, 1, 1)
        T[f"{blk}.branch3x3dbl_3"] = (96, 96, 3, 3, 1, 1, 1)
        T[f"{blk}.branch_pool"] = (cin, pf, 1, 1, 1, 0, 0)
    T["Mixed_6a.branch3x3"] = (288, 384, 3, 3, 2, 0, 0)
    T["Mixed_6a.branch3x3dbl_1"] = (288, 64, 1, 1, 1, 0, 0)
    T["Mixed_6a.branch3x3dbl_2"] = (64, 96, 3, 3, 1, 1, 1)
    T["Mixed_6a.branch3x3dbl_3"] = (96, 96, 3, 3, 2, 0, 0)
    for blk, c7 in (("Mixed_6b", 128), ("Mixed_6c", 160), ("Mixed_6d", 160), ("Mixed_6e", 192)):
        T[f"{blk}.branch1x1"] = (768, 192, 1, 1, 1, 0, 0)
        T[f"{blk}.branch7x7_1"] = (768, c7, 1, 1, 1, 0, 0)
        T[f"{blk}.branch7x7_2"] = (c7, c7, 1, 7, 1, 0, 3)
        T[f"{blk}.branch7x7_3"] = (c7, 192, 7, 1, 1, 3, 0)
        T[f"{blk}.branch7x7dbl_1"] = (768, c7, 1, 1, 1, 0, 0)
        T[f"{blk}.branch7x7dbl_2"] = (c7, c7, 7, 1, 1, 3, 0)
        T[f"{blk}.branch7x7dbl_3"] = (c7, c7, 1, 7, 1, 0, 3)
        T[f"{blk}.branch7x7dbl_4"] = (c7, c7, 7, 1, 1, 3, 0)
        T[f"{blk}.branch7x7dbl_5"] = (c7, 192, 1, 7, 1, 0, 3)
        T[f"{blk}.branch_pool"] = (768, 192, 1, 1, 1, 0, 0)
    T["Mixed_7a.branch3x3_1"] = (768, 192, 1, 1, 1, 0, 0)
    T["Mixed_7a.branch3x3_2"] = (192, 320, 3, 3, 2, 0, 0)
    T["Mixed_7a.branch7x7x3_1"] = (768, 192, 1, 1, 1, 0, 0)
    T["Mixed_7a.branch7x7x3_2"] = (192, 192, 1, 7, 1, 0, 3)
    T["Mixed_7a.branch7x7x3_3"] = (192, 192, 7, 1, 1, 3, 0)
    T["Mixed_7a.branch7x7x3_4"] = (192, 192, 3, 3, 2, 0, 0)
    for blk, cin in (("Mixed_7b", 1280), ("Mixed_7c", 2048)):
        T[f"{blk}.branch1x1"] = (cin, 320, 1, 1, 1, 0, 0)
        T[f"{blk}.branch3x3_1"] = (cin, 384, 1, 1, 1, 0, 0)
        T[f"{blk}.branch3x3_2a"] = (384, 384, 1, 3, 1, 0, 1)
        T[f"{blk}.branch3x3_2b"] = (384, 384, 3, 1, 1, 1, 0)
        T[f"{blk}.branch3x3dbl_1"] = (cin, 448, 1, 1, 1, 0, 0)
        T[f"{blk}.branch3x3dbl_2"] = (448, 384, 3, 3, 1, 1, 1)
        T[f"{blk}.branch3x3dbl_3a"] = (384, 384, 1, 3, 1, 0, 1)
        T[f"{blk}.branch3x3dbl_3b"] = (384, 384, 3, 1, 1, 1, 0)
        T[f"{blk}.branch_pool"] = (cin, 192, 1, 1, 1, 0, 0)
    return T


def state_dict_shapes():
    """name -> shape of every entry of the state dict."""
    S = OrderedDict()
    for name, (cin, cout, kh, kw, _, _, _) in unit_table().items():
        S[f"{name}.conv.weight"] = (cout, cin, kh, kw)
        for leaf in ("weight", "bias", "running_mean", "running_var"):
            S[f"{name}.bn.{leaf}"] = (cout,)
    S["fc.weight"] = (1008, 2048)
    S["fc.bias"] = (1008,)
    return S


def seeded_state_dict(seed=FIXTURE_SEED):
    """He-scaled conv weights (std = sqrt(2 / fan_in)), BN weight and running_var near 1, small running_mean and bias: activations keep a
    scale of order 1 through the 94 units (the fixture condition is checked by tests/test_inception_cpu.py)."""
    g = gen(seed)
    sd = OrderedDict()
    for name, (cin, cout, kh, kw, _, _, _) in unit_table().items():
        sd[f"{name}.conv.weight"] = torch.randn(cout, cin, kh, kw, generator=g) * math.sqrt(2.0 / (cin * kh * kw))
        sd[f"{name}.bn.weight"] = 1.0 + 0.1 * (torch.rand(cout, generator=g) - 0.5)
        sd[f"{name}.bn.bias"] = 0.05 * torch.randn(cout, generator=g)
        sd[f"{name}.bn.running_mean"] = 0.05 * torch.randn(cout, generator=g)
        sd[f"{name}.bn.running_var"] = 1.0 + 0.2 * (torch.rand(cout, generator=g) - 0.5)
    sd["fc.weight"] = torch.randn(1008, 2048, generator=g) * math.sqrt(1.0 / 2048)
    sd["fc.bias"] = 0.1 * torch.randn(1008, generator=g)
    return sd


def fixture_images(B=2, H=64, W=48, seed=11):
    """uint8 (B, 3, H, W): a smooth random field plus noise, so that neighbouring pixels differ and the resize has something to blend."""
    g = gen(seed)
    coarse = torch.rand(B, 3, 6, 5, generator=g)
    field = F.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=False)
    return ((0.75 * field + 0.25 * torch.rand(B, 3, H, W, generator=g)) * 255.0).clamp(0, 255).to(torch.uint8)



# ---- preprocessing ------------------------------------------------------------------------------------------------------------------
def to_bytes(imgs, normalize):
    """-> float64 byte values.  normalize: trunc(255 v) with the fp32 product, clamped to [0, 255]."""
    if not normalize:
        assert imgs.dtype == torch.uint8
        return imgs.double()
    assert imgs.dtype == torch.float32
    return torch.trunc(imgs * 255.0).clamp(0, 255).double()


def axis_table(n_in, n_out=SIZE):
    s = n_in / n_out                                                   # Python float: double
    src = torch.arange(n_out, dtype=torch.float64) * s
    i0 = torch.floor(src)
    w = (src - i0).float().double()                                    # the weight the kernel receives, rounded to fp32
    i0 = i0.long().clamp(max=n_in - 1)
    return i0, (i0 + 1).clamp(max=n_in - 1), w


def tf1_resize(v, dtype=torch.float64):
    """(B, 3, H, W) byte values -> (B, 3, 299, 299) on the 0..255 scale: rows first, top = l + (r - l) wx, then top + (bottom - top) wy."""
    v = v.to(dtype)
    y0, y1, wy = axis_table(v.shape[2])
    x0, x1, wx = axis_table(v.shape[3])
    y0, y1, x0, x1 = (t.to(v.device) for t in (y0, y1, x0, x1))
    wy, wx = wy.to(v.device, dtype), wx.to(v.device, dtype)
    top = v[:, :, y0][:, :, :, x0] + (v[:, :, y0][:, :, :, x1] - v[:, :, y0][:, :, :, x0]) * wx
    bot = v[:, :, y1][:, :, :, x0] + (v[:, :, y1][:, :, :, x1] - v[:, :, y1][:, :, :, x0]) * wx
    return top + (bot - top) * wy[:, None]


def preprocess(imgs, normalize=False, dtype=torch.float64):
    """-> (B, 3, 299, 299) in (v - 128) / 128."""
    return (tf1_resize(to_bytes(imgs, normalize), dtype) - 128.0) / 128.0


def to_rows(x):
    """(B, C, H, W) -> NHWC rows (B*H*W, C)."""
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]).contiguous()


def from_rows(rows, B, H, W):
    return rows.reshape(B, H, W, -1).permute(0, 3, 1, 2).contiguous()


# ---- the graph ----------------------------------------------------------------------------------------------------------------------
def tower(sd, x, trace=None):
    """x (B, 3, 299, 299) in (v - 128) / 128, any floating dtype; sd a state dict (cast to x's dtype) -> dict(pool, logits_unbiased, logits).
    ``trace``: a list that receives (name, channels, H, W) after every stage."""
    T = unit_table()
    dt = x.dtype
    P = {k: v.to(dt) for k, v in sd.items()}

    def cv(name, t):
        _, _, _, _, s, ph, pw = T[name]
        t = F.conv2d(t, P[f"{name}.conv.weight"], None, stride=s, padding=(ph, pw))
        t = F.batch_norm(t, P[f"{name}.bn.running_mean"], P[f"{name}.bn.running_var"], P[f"{name}.bn.weight"], P[f"{name}.bn.bias"], False, 0.0, BN_EPS)
        return F.relu(t)

    def avg(t):
        return F.avg_pool2d(t, 3, 1, 1, count_include_pad=False)

    def note(name, t):
        if trace is not None:
            trace.append((name, t.shape[1], t.shape[2], t.shape[3]))
        return t

    note("input", x)
    x = note("Conv2d_1a_3x3", cv("Conv2d_1a_3x3", x))
    x = note("Conv2d_2a_3x3", cv("Conv2d_2a_3x3", x))
    x = cv("Conv2d_2b_3x3", x)
    x = note("maxpool1", F.max_pool2d(x, 3, 2))
    x = cv("Conv2d_3b_1x1", x)
    x = note("Conv2d_4a_3x3", cv("Conv2d_4a_3x3", x))
    x = note("maxpool2", F.max_pool2d(x, 3, 2))
    for b in ("Mixed_5b", "Mixed_5c", "Mixed_5d"):
        x = note(b, torch.cat([cv(f"{b}.branch1x1", x), cv(f"{b}.branch5x5_2", cv(f"{b}.branch5x5_1", x)),
                               cv(f"{b}.branch3x3dbl_3", cv(f"{b}.branch3x3dbl_2", cv(f"{b}.branch3x3dbl_1", x))), cv(f"{b}.branch_pool", avg(x))], 1))
    b = "Mixed_6a"
    x = note(b, torch.cat([cv(f"{b}.branch3x3", x), cv(f"{b}.branch3x3dbl_3", cv(f"{b}.branch3x3dbl_2", cv(f"{b}.branch3x3dbl_1", x))), F.max_pool2d(x, 3, 2)], 1))
    for b in ("Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"):
        t = cv(f"{b}.branch7x7dbl_1", x)
        for i in (2, 3, 4, 5):
            t = cv(f"{b}.branch7x7dbl_{i}", t)
        x = note(b, torch.cat([cv(f"{b}.branch1x1", x), cv(f"{b}.branch7x7_3", cv(f"{b}.branch7x7_2", cv(f"{b}.branch7x7_1", x))), t, cv(f"{b}.branch_pool", avg(x))], 1))
    b = "Mixed_7a"
    t = cv(f"{b}.branch7x7x3_1", x)
    for i in (2, 3, 4):
        t = cv(f"{b}.branch7x7x3_{i}", t)
    x = note(b, torch.cat([cv(f"{b}.branch3x3_2", cv(f"{b}.branch3x3_1", x)), t, F.max_pool2d(x, 3, 2)], 1))
    for b, pool in (("Mixed_7b", avg), ("Mixed_7c", lambda t: F.max_pool2d(t, 3, 1, 1))):
        t3 = cv(f"{b}.branch3x3_1", x)
        td = cv(f"{b}.branch3x3dbl_2", cv(f"{b}.branch3x3dbl_1", x))
        x = note(b, torch.cat([cv(f"{b}.branch1x1", x), cv(f"{b}.branch3x3_2a", t3), cv(f"{b}.branch3x3_2b", t3),
                               cv(f"{b}.branch3x3dbl_3a", td), cv(f"{b}.branch3x3dbl_3b", td), cv(f"{b}.branch_pool", pool(x))], 1))
    pool = x.mean(dim=(2, 3))
    unbiased = pool @ P["fc.weight"].t()
    return dict(pool=pool, logits_unbiased=unbiased, logits=unbiased + P["fc.bias"])


@functools.lru_cache(maxsize=2)
def fixture(seed=FIXTURE_SEED):
    """The shared fixture, computed once per process and never modified: the seeded weights, the test images, the float64 reference of the
    tower on them, the fp32 run of the same restatement and the geometry trace."""
    sd = seeded_state_dict(seed)
    imgs = fixture_images()
    trace = []
    with torch.no_grad():
        ref64 = tower(sd, preprocess(imgs, False, torch.float64), trace)
        ref32 = tower(sd, preprocess(imgs, False, torch.float32))
    return dict(sd=sd, imgs=imgs, ref64=ref64, ref32=ref32, trace=trace)


def tower_tol(ref64, ref32):
    """-> (bound, base) on max-abs error over max|ref|: TOWER_FACTOR x the fp32 restatement's own error + TOWER_FLOOR_ULPS fp32 ulps."""
    scale = float(ref64.abs().max())
    base = float((ref32.double() - ref64).abs().max()) / scale
    return TOWER_FACTOR * base + TOWER_FLOOR_ULPS * 2.0 ** -23, base


# ---- FID and the Inception score ----------------------------------------------------------------------------------------------------
def moments(feats):
    """The sequential float64 sums of fp32 rows, in numpy (row by row, ascending): (sum (d,), outer (d, d), n)."""
    import numpy as np
    x = feats.detach().cpu().numpy().astype(np.float64)
    s, o = np.zeros(x.shape[1]), np.zeros((x.shape[1], x.shape[1]))
    for r in range(x.shape[0]):
        s += x[r]
        o += np.outer(x[r], x[r])
    return s, o, x.shape[0]


def mean_cov(s, o, n):
    s, o = torch.as_tensor(s, dtype=torch.float64), torch.as_tensor(o, dtype=torch.float64)
    mu = s / n
    return mu, (o - n * torch.outer(mu, mu)) / (n - 1)


def fid_eigvals(m1, m2):
    """FID = |mu1 - mu2|^2 + tr S1 + tr S2 - 2 sum sqrt(eigvals(S1 S2)).real from two (sum, outer, n) triples."""
    (mu1, S1), (mu2, S2) = mean_cov(*m1), mean_cov(*m2)
    ev = torch.linalg.eigvals(S1 @ S2)
    return float(((mu1 - mu2) ** 2).sum() + torch.trace(S1) + torch.trace(S2) - 2.0 * torch.sqrt(ev).real.sum())


def fid_eigh(m1, m2):
    """The same number by a second float64 route: tr sqrt(S1 S2) = tr sqrt(S1^(1/2) S2 S1^(1/2)), both square roots by eigh."""
    (mu1, S1), (mu2, S2) = mean_cov(*m1), mean_cov(*m2)
    w, V = torch.linalg.eigh(S1)
    R = (V * torch.sqrt(w.clamp(min=0.0))) @ V.t()
    ev = torch.linalg.eigvalsh(R @ S2 @ R)
    return float(((mu1 - mu2) ** 2).sum() + torch.trace(S1) + torch.trace(S2) - 2.0 * torch.sqrt(ev.clamp(min=0.0)).sum())


def fid_tol(m1, m2):
    """-> (bound, spread): 16 x the spread between the two float64 routes on this input + 1e-12 (tr S1 + tr S2)."""
    (_, S1), (_, S2) = mean_cov(*m1), mean_cov(*m2)
    spread = abs(fid_eigvals(m1, m2) - fid_eigh(m1, m2))
    return 16.0 * spread + 1e-12 * float(torch.trace(S1) + torch.trace(S2)), spread


def inception_score(logits, splits, perm):
    """(mean, std) in float64 of exp(mean_i sum_c p (log p - log mean_i p)) over torch.chunk(splits) of the rows permuted by ``perm``."""
    x = logits.detach().cpu().double()[perm]
    p = torch.softmax(x, dim=1)
    scores = []
    for c in torch.chunk(p, splits, dim=0):
        m = c.mean(dim=0, keepdim=True)
        scores.append(torch.exp((c * (torch.log(c) - torch.log(m))).sum(dim=1).mean()))
    scores = torch.stack(scores)
    return float(scores.mean()), float(scores.std())
