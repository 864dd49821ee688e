"""The definitions of the tokenizer validation metrics ("tokenizer validation metrics"; fourm.vq.metrics, csrc/metrics.hip)
restated in plain torch on the CPU: F.conv2d with the outer-product window and groups = C, F.avg_pool2d, sums.  Evaluated in float64 on the
fp32 inputs it is the reference; the same code evaluated at dtype=torch.float32 gives the comparison baseline of the SSIM / MS-SSIM tests.
Nothing here looks at what the kernels return.

Bounds of the sums (MSE, MAE, PSNR), from the formats: U = 2^-24 is the fp32 unit roundoff.  A term d = p - t rounds once (U |d|); d * d adds
U and doubles the relative error of d (3 U d^2), |d| adds nothing (U |d|).  First-order bounds are doubled for the second-order terms.  The sums
are carried in double: n 2^-53 relative.  The quotient is formed in double and rounded to fp32 once: U.
    MSE: (6 + 1) U MSE + n 2^-53 MSE        MAE: (2 + 1) U MAE + n 2^-53 MAE
    PSNR = 10 log10(L^2 / MSE): (10 / ln 10) (6 U + n 2^-53) + U |PSNR|
With the sigmoid in the load (1 / (1 + expf(-v)): expf within 2 ulp, the sum and the correctly rounded quotient one each, p <= 1) the
prediction carries an absolute error of at most EPS_SIGMOID = 5 U: + 2 mean|d| EPS_SIGMOID on the MSE, + EPS_SIGMOID on the MAE, both doubled.

Bound of the SSIM / MS-SSIM comparisons: the error of this restatement evaluated in fp32 against float64 on the same inputs, times
SSIM_FACTOR = 4 (the row / column split adds a rounding per moment, the tile partials reorder the mean), plus a floor of SSIM_FLOOR_ULPS = 4
fp32 ulps (2^-23) of the value for the cases where the fp32 restatement happens to land exactly.  The figure of a case is the largest error the
fp32 restatement shows over the values of that case (the per-image ssim and cs of one shape; the metric of one shape and noise level): single
values are sums of few rounding errors of either sign, and the ratio of two of those has no bound."""
import math

import torch
import torch.nn.functional as F

U = 2.0 ** -24
EPS_SIGMOID = 5 * U
SSIM_FACTOR = 4.0
SSIM_FLOOR_ULPS = 4.0
BETAS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
DENSE_FEAT_MODALITIES = ['CLIP-B16', 'CLIP-L14', 'DINOv2-B14', 'DINOv2-G14', 'ImageBind-H14']


def gen(seed):
    return torch.Generator().manual_seed(seed)


def window(kernel_size=11, sigma=1.5):
    """fp32 taps: normalised to sum 1 in float64, rounded once."""
    i = torch.arange(kernel_size, dtype=torch.float64) - (kernel_size - 1) / 2.0
    g = torch.exp(-(i / sigma) ** 2 / 2.0)
    return (g / g.sum()).float()


def convert(pred, target, c_use, transform):
    """The conversion of the kernels' loads on fp32 CPU tensors -> float64 (pred, target) of c_use channels.  'denorm' is the fp32 add and the
    exact halving (every value is an fp32 number); 'sigmoid_pred' is the exact sigmoid of the fp32 prediction."""
    p, t = pred[:, :c_use].float(), target[:, :c_use].float()
    if transform == "denorm":
        return ((p + 1.0) * 0.5).double(), ((t + 1.0) * 0.5).double()
    if transform == "sigmoid_pred":
        return torch.sigmoid(p.double()), t.double()
    assert transform == "raw"
    return p.double(), t.double()


def error_sums(p, t, data_range=1.0):
    """-> dict(mse, mae, psnr, n) in float64 from converted tensors."""
    d = p.double() - t.double()
    mse, mae = (d * d).mean(), d.abs().mean()
    return dict(mse=mse, mae=mae, psnr=10.0 * torch.log10(data_range ** 2 / mse), n=d.numel())


def error_bounds(ref, sigmoid=False):
    n, mse, mae = ref["n"], float(ref["mse"]), float(ref["mae"])
    acc = n * 2.0 ** -53
    e_mse, e_mae = (6 * U + acc) * mse, (2 * U + acc) * mae
    if sigmoid:
        e_mse, e_mae = e_mse + 2 * (2 * mae * EPS_SIGMOID), e_mae + 2 * EPS_SIGMOID
    return dict(mse=e_mse + U * mse, mae=e_mae + U * mae, psnr=(10 / math.log(10)) * (e_mse / mse if mse > 0 else 0.0) + U * abs(float(ref["psnr"])))


def iou_counts(p, t, threshold=0.5):
    """-> (tp, fp, fn, n) as Python ints from converted float64 tensors."""
    pp, tp_ = p.clamp(0, 1) > threshold, t == 1
    return int((pp & tp_).sum()), int((pp & ~tp_).sum()), int((~pp & tp_).sum()), p.numel()


def ssim_scale(x, y, win, c1, c2):
    """One scale on (B, C, H, W) tensors of any floating dtype -> per-image (ssim, cs), the means over channels and valid window positions."""
    C = x.shape[1]
    w = torch.outer(win.to(x.dtype), win.to(x.dtype)).expand(C, 1, -1, -1).contiguous()
    mu_x, mu_y = F.conv2d(x, w, groups=C), F.conv2d(y, w, groups=C)
    var_x = F.conv2d(x * x, w, groups=C) - mu_x * mu_x
    var_y = F.conv2d(y * y, w, groups=C) - mu_y * mu_y
    cov = F.conv2d(x * y, w, groups=C) - mu_x * mu_y
    cs = (2 * cov + c2) / (var_x + var_y + c2)
    ssim = (2 * mu_x * mu_y + c1) / (mu_x * mu_x + mu_y * mu_y + c1) * cs
    return ssim.flatten(1).mean(1), cs.flatten(1).mean(1)


def ms_ssim(x, y, data_range=1.0, kernel_size=11, sigma=1.5, betas=BETAS, normalize=None):
    """-> (per-image MS-SSIM (B,), the per-scale terms (S, B)) at the dtype of x."""
    win = window(kernel_size, sigma)
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    terms = []
    for s in range(len(betas)):
        ssim, cs = ssim_scale(x, y, win, c1, c2)
        terms.append(ssim if s == len(betas) - 1 else cs)
        if s + 1 < len(betas):
            x, y = F.avg_pool2d(x, 2), F.avg_pool2d(y, 2)
    terms = torch.stack(terms)
    used = torch.relu(terms) if normalize == "relu" else terms
    return torch.prod(used ** torch.tensor(betas, dtype=x.dtype)[:, None], 0), terms


def ssim_tol(ref64, ref32):
    """-> the bound of a case from the float64 and the fp32 restatement of its values (tensors of the same shape)."""
    ref64 = ref64.double().reshape(-1)
    base = float((ref32.double().reshape(-1) - ref64).abs().max())
    return SSIM_FACTOR * base + SSIM_FLOOR_ULPS * 2.0 ** -23 * float(ref64.abs().max()), base


def structured_pair(shape, sigma, seed):
    """target = 0.7 * a bilinearly upsampled coarse random field + 0.3 * uniform noise, clamped to [0, 1]; prediction = target + sigma * Gaussian
    noise.  fp32 CPU tensors."""
    g = gen(seed)
    B, C, H, W = shape
    coarse = torch.rand(B, C, max(2, -(-H // 16)), max(2, -(-W // 16)), generator=g)
    field = F.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=False)
    target = (0.7 * field + 0.3 * torch.rand(shape, generator=g)).clamp(0, 1)
    pred = target + sigma * torch.randn(shape, generator=g)
    return pred.float().contiguous(), target.float().contiguous()


def sentinel_view(shape, dtype, device, value, pad=64):
    """-> (buffer, view): a contiguous view of ``shape`` in the middle of a buffer filled with ``value``; pad elements on either side."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * pad,), value, dtype=dtype, device=device)
    return buf, buf[pad:pad + n].view(shape)


def sentinels_intact(buf, n, value, pad=64):
    return bool((buf[:pad] == value).all()) and bool((buf[pad + n:] == value).all())
