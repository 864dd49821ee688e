"""Tokenizer validation metrics on the HIP engine: the image metrics of upstream's ``eval_metrics`` (run_training_vqvae.py:1427-1632,
run_training_divae.py:1298 ff.), which upstream takes from torchmetrics, as a library an evaluation loop can sit on.

    MeanSquaredError, MeanAbsoluteError, PeakSignalNoiseRatio, MultiScaleStructuralSimilarityIndexMeasure, BinaryJaccardIndex
                             the constructor calls of eval_metrics verbatim; ``update(preds, target)`` / ``compute()`` / ``reset()`` / ``.to(device)``
    LearnedPerceptualImagePatchSimilarity
                             the AlexNet LPIPS metric of :1486-1491 on fourm.vq.percept_losses.lpips_alex.LpipsAlex (csrc/lpips_metric.hip)
    ReconstructionMetrics    the per-domain part of eval_metrics (:1469-1480, :1513-1553, :1557-1575): takes the decoder output and the prepared
                             input as they are and converts them inside the kernels' loads
    token_histogram          the ``np.bincount`` of :1622 on the device

Everything is fp32 in, float64 sums and int64 counts in device tensors; the kernels are csrc/metrics.hip.  ``update`` never synchronises with the
host; ``compute`` is where a number is asked for.  The definitions ("tokenizer validation metrics") are the contract: torchmetrics
is not a dependency, and parity with it is not pinned.  Tensors on the CPU raise RuntimeError (there is no CPU path).

Not here: pretrained weights of any kind (the LPIPS metric takes a loaded ``LpipsAlex``; without one its weights are seeded-random) and the trainer
scripts themselves (FID and the Inception score: fourm.utils.inception); codebook usage is ``fourm.vq.vq_utils.compute_codebook_usage``."""
from typing import Dict, Optional, Sequence, Tuple

import torch

from fourm.vq.training import _on_gpu

DENSE_FEAT_MODALITIES = ['CLIP-B16', 'CLIP-L14', 'DINOv2-B14', 'DINOv2-G14', 'ImageBind-H14']
UNIT_RANGE_1CH = ['edge_occlusion', 'edge_texture', 'keypoints2d', 'keypoints3d', 'reshading']
MAX_KERNEL_SIZE = 11          # FM_SSIM_MAX_KERNEL
RAW, DENORM, SIGMOID_PRED = "raw", "denorm", "sigmoid_pred"

__all__ = ["MeanSquaredError", "MeanAbsoluteError", "PeakSignalNoiseRatio", "MultiScaleStructuralSimilarityIndexMeasure", "BinaryJaccardIndex",
           "LearnedPerceptualImagePatchSimilarity", "ReconstructionMetrics", "token_histogram", "domain_spec", "gaussian_window", "DENSE_FEAT_MODALITIES"]


def _transform_id(transform):
    from fourm.hip import _lib as L
    return {RAW: L.METRIC_RAW, DENORM: L.METRIC_DENORM, SIGMOID_PRED: L.METRIC_SIGMOID_PRED}[transform]


def _accept(cls, kwargs, **allowed):
    """torchmetrics keywords that upstream passes: known names with their one supported value, anything else is refused."""
    for k, v in kwargs.items():
        if k not in allowed:
            raise TypeError(f"{cls}: unexpected keyword {k!r}")
        if not any(v is a or (type(v) is type(a) and v == a) for a in allowed[k]):
            raise ValueError(f"{cls}: {k}={v!r} is not built (supported: {', '.join(repr(a) for a in allowed[k])})")


_COMMON = dict(sync_on_compute=(True, False), compute_on_cpu=(False, True))          # no process group is touched and nothing moves to the CPU either way


def _check_pair(what, preds, target, same_channels=True):
    if not (torch.is_tensor(preds) and torch.is_tensor(target)) or preds.dim() != 4 or target.dim() != 4:
        raise ValueError(f"{what}: two (B, C, H, W) tensors expected")
    if preds.dtype != torch.float32 or target.dtype != torch.float32:
        raise TypeError(f"{what}: fp32 tensors expected, got {preds.dtype} / {target.dtype}")
    ps, ts = tuple(preds.shape), tuple(target.shape)
    if (ps != ts) if same_channels else (ps[:1] + ps[2:] != ts[:1] + ts[2:]):
        raise ValueError(f"{what}: preds {ps} and target {ts} differ in shape")
    if preds.numel() == 0:
        raise ValueError(f"{what}: empty batch {ps}")


class _Metric:
    """State in device tensors, created on the device of the first ``update`` (or moved there)."""
    _STATE = ()          # (name, dtype, numel)

    def __init__(self):
        self._device = None
        self.reset()

    def reset(self):
        for name, dtype, n in self._STATE:
            cur = getattr(self, name, None)
            setattr(self, name, None if cur is None else torch.zeros(n, dtype=dtype, device=cur.device))

    def to(self, device):
        self._device = torch.device(device) if device is not None else None
        for name, _, _ in self._STATE:
            cur = getattr(self, name)
            if cur is not None:
                setattr(self, name, cur.to(self._device))
        return self

    def _state_on(self, device):
        for name, dtype, n in self._STATE:
            cur = getattr(self, name)
            if cur is None:
                setattr(self, name, torch.zeros(n, dtype=dtype, device=device))
            elif cur.device != device:
                setattr(self, name, cur.to(device))

    def _nan(self):
        return torch.tensor(float("nan"), dtype=torch.float32)          # (nothing was seen: 0 / 0)


def _accumulate_sums(what, preds, target, sums, counts, c_use=None, transform=RAW, iou=False, threshold=0.5):
    from fourm.hip import ops
    _on_gpu(what, preds, target)
    with torch.no_grad(), torch.cuda.device(preds.device):
        p, t = preds.detach().contiguous(), target.detach().contiguous()
        ops.metric_sums(p, t, p.shape[1] if c_use is None else c_use, _transform_id(transform), sums, counts, iou=iou, threshold=threshold)


class _ErrorSums(_Metric):
    """sum d^2, sum |d| and the element count since ``reset``: one pass of fm_metric_sums per ``update``."""
    _STATE = (("sums", torch.float64, 2), ("counts", torch.int64, 5))

    def update(self, preds: torch.Tensor, target: torch.Tensor) -> None:
        what = type(self).__name__
        _check_pair(what, preds, target)
        _on_gpu(what, preds, target)
        self._state_on(preds.device)
        _accumulate_sums(what, preds, target, self.sums, self.counts)

    def _mean(self, i):
        return self.sums[i] / self.counts[3].double()


class MeanSquaredError(_ErrorSums):
    """sum (preds - target)^2 / n over everything seen since ``reset`` (the difference rounded once, the square in fp32, the sum in double)."""

    def __init__(self, squared=True, num_outputs=1, **kwargs):
        _accept("MeanSquaredError", dict(squared=squared, num_outputs=num_outputs, **kwargs), squared=(True,), num_outputs=(1,), **_COMMON)
        super().__init__()

    def compute(self) -> torch.Tensor:
        return self._nan() if self.sums is None else self._mean(0).float()


class MeanAbsoluteError(_ErrorSums):
    """sum |preds - target| / n over everything seen since ``reset``."""

    def __init__(self, **kwargs):
        _accept("MeanAbsoluteError", kwargs, **_COMMON)
        super().__init__()

    def compute(self) -> torch.Tensor:
        return self._nan() if self.sums is None else self._mean(1).float()


def _psnr(mse, data_range):
    return 10.0 * torch.log10(data_range * data_range / mse)


class PeakSignalNoiseRatio(_ErrorSums):
    """10 log10(data_range^2 / MSE) from the global sums since ``reset`` (not a mean of per-batch values).  ``data_range`` has to be given."""

    def __init__(self, data_range=None, base=10.0, reduction='elementwise_mean', dim=None, **kwargs):
        _accept("PeakSignalNoiseRatio", dict(base=base, reduction=reduction, dim=dim, **kwargs), base=(10.0, 10), reduction=('elementwise_mean',), dim=(None,), **_COMMON)
        if isinstance(data_range, bool) or not isinstance(data_range, (int, float)) or not data_range > 0:
            raise ValueError(f"PeakSignalNoiseRatio: data_range={data_range!r}: a positive number is required (it is not inferred from the data)")
        self.data_range = float(data_range)
        super().__init__()

    def compute(self) -> torch.Tensor:
        return self._nan() if self.sums is None else _psnr(self._mean(0), self.data_range).float()


class BinaryJaccardIndex(_Metric):
    """tp / (tp + fp + fn): the prediction is positive where clamp(preds, 0, 1) > threshold, the target where it equals 1.  Targets have to be
    exactly 0 or 1; others are counted on the device and raise ValueError at ``compute``.  No positive anywhere: nan (0 / 0)."""
    _STATE = (("counts", torch.int64, 5),)

    def __init__(self, threshold=0.5, ignore_index=None, validate_args=True, **kwargs):
        _accept("BinaryJaccardIndex", dict(ignore_index=ignore_index, validate_args=validate_args, **kwargs), ignore_index=(None,), validate_args=(True,), **_COMMON)
        if isinstance(threshold, bool) or not isinstance(threshold, (int, float)) or not 0.0 <= threshold <= 1.0:
            raise ValueError(f"BinaryJaccardIndex: threshold={threshold!r}: a number in [0, 1] expected")
        self.threshold = float(threshold)
        super().__init__()

    def update(self, preds: torch.Tensor, target: torch.Tensor) -> None:
        _check_pair("BinaryJaccardIndex", preds, target)
        _on_gpu("BinaryJaccardIndex", preds, target)
        self._state_on(preds.device)
        sums = torch.zeros(2, dtype=torch.float64, device=preds.device)
        _accumulate_sums("BinaryJaccardIndex", preds, target, sums, self.counts, iou=True, threshold=self.threshold)

    def compute(self) -> torch.Tensor:
        return self._nan() if self.counts is None else _iou(self.counts)


def _iou(counts):
    tp, fp, fn, _, bad = counts.tolist()
    if bad:
        raise ValueError(f"BinaryJaccardIndex: {bad} target values are neither 0 nor 1")
    return (counts[0].double() / (counts[0] + counts[1] + counts[2]).double()).float()


def gaussian_window(kernel_size: int, sigma: float) -> torch.Tensor:
    """g_i proportional to exp(-((i - (k - 1) / 2) / sigma)^2 / 2), normalised to sum 1 in float64 and rounded to fp32 once (a CPU tensor)."""
    i = torch.arange(kernel_size, dtype=torch.float64) - (kernel_size - 1) / 2.0
    g = torch.exp(-(i / float(sigma)) ** 2 / 2.0)
    return (g / g.sum()).float()


class MultiScaleStructuralSimilarityIndexMeasure(_Metric):
    """Mean over all images since ``reset`` of  prod_{i < S - 1} cs_i^beta_i * ssim_{S - 1}^beta_{S - 1},  S = len(betas) scales, each the 2 x 2
    mean of the one before; cs_i / ssim_i the per-image means over channels and valid window positions (separable Gaussian window).

    ``normalize`` None or False (upstream's setting): nothing is done to the per-scale terms, so a negative one (anti-correlated images) makes
    that image's value, and with it the metric, NaN.  'relu': negative terms become 0.  Images need min(H, W) > (kernel_size - 1) * 2^(S - 1)."""
    _STATE = (("similarity", torch.float64, 1), ("total", torch.int64, 1))

    def __init__(self, gaussian_kernel=True, kernel_size=11, sigma=1.5, reduction='elementwise_mean', data_range=None, k1=0.01, k2=0.03,
                 betas: Sequence[float] = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333), normalize=None, **kwargs):
        name = "MultiScaleStructuralSimilarityIndexMeasure"
        _accept(name, dict(gaussian_kernel=gaussian_kernel, reduction=reduction, **kwargs), gaussian_kernel=(True,), reduction=('elementwise_mean',), **_COMMON)
        if normalize is not None and normalize is not False and normalize != 'relu':
            raise ValueError(f"{name}: normalize={normalize!r} is not built (None, False or 'relu')")
        if isinstance(kernel_size, bool) or not isinstance(kernel_size, int) or kernel_size < 1 or kernel_size % 2 == 0 or kernel_size > MAX_KERNEL_SIZE:
            raise ValueError(f"{name}: kernel_size={kernel_size!r}: an odd integer in [1, {MAX_KERNEL_SIZE}] expected")
        if isinstance(sigma, bool) or not isinstance(sigma, (int, float)) or not sigma > 0:
            raise ValueError(f"{name}: sigma={sigma!r}: a positive number expected")
        if isinstance(data_range, bool) or not isinstance(data_range, (int, float)) or not data_range > 0:
            raise ValueError(f"{name}: data_range={data_range!r}: a positive number is required (it is not inferred from the data)")
        betas = tuple(float(b) for b in betas)
        if not betas or not all(b >= 0 for b in betas):
            raise ValueError(f"{name}: betas={betas!r}: a non-empty sequence of non-negative numbers expected")
        self.kernel_size, self.sigma, self.data_range, self.betas, self.normalize = kernel_size, float(sigma), float(data_range), betas, normalize or None
        self.c1, self.c2 = (float(k1) * self.data_range) ** 2, (float(k2) * self.data_range) ** 2
        self._window = gaussian_window(kernel_size, sigma)
        super().__init__()

    def _check_size(self, H, W):
        limit = (self.kernel_size - 1) * 2 ** (len(self.betas) - 1)
        if min(H, W) <= limit:
            raise ValueError(f"MultiScaleStructuralSimilarityIndexMeasure: images of {H} x {W}: the smaller side has to exceed (kernel_size - 1) * 2^(scales - 1) = {limit}")

    def update(self, preds: torch.Tensor, target: torch.Tensor) -> None:
        _check_pair(type(self).__name__, preds, target)
        self._update(preds, target, preds.shape[1], RAW)

    def _update(self, preds, target, c_use, transform):
        from fourm.hip import _lib as L
        from fourm.hip import ops
        self._check_size(preds.shape[2], preds.shape[3])
        _on_gpu(type(self).__name__, preds, target)
        device = preds.device
        self._state_on(device)
        if self._window.device != device:
            self._window = self._window.to(device)
        B, S = preds.shape[0], len(self.betas)
        with torch.no_grad(), torch.cuda.device(device):
            x, y, tr = preds.detach().contiguous(), target.detach().contiguous(), _transform_id(transform)
            ssim = torch.empty(S, B, dtype=torch.float64, device=device)
            cs = torch.empty(S, B, dtype=torch.float64, device=device)
            for s in range(S):
                ops.ssim_scale(x, y, c_use, tr, self._window, self.c1, self.c2, ssim[s], cs[s])
                if s + 1 < S:
                    x, y = ops.avgpool2x2_pair(x, y, c_use, tr)
                    tr = L.METRIC_RAW
            # the combination over the scales: float64 torch ops on the device (a negative base to a fractional power is nan, as documented)
            terms = torch.cat([cs[:S - 1], ssim[S - 1:]], 0)
            if self.normalize == 'relu':
                terms = torch.relu(terms)
            per_image = torch.prod(terms ** torch.tensor(self.betas, dtype=torch.float64, device=device)[:, None], 0)
            self.similarity += per_image.sum()
            self.total += B

    def compute(self) -> torch.Tensor:
        return self._nan() if self.similarity is None else (self.similarity[0] / self.total[0].double()).float()


# ---- LPIPS ----------------------------------------------------------------------------------------------------------------------------------------
class LearnedPerceptualImagePatchSimilarity(_Metric):
    """Mean (or sum) over all pairs since ``reset`` of the AlexNet LPIPS distance.  ``update(img1, img2)``: (N, 3, H, W) images, H, W >= 31, in
    [-1, 1], or in [0, 1] with ``normalize=True`` (mapped by 2 x - 1 inside the stem's loads).  ``net``: a ``LpipsAlex`` (load the
    checkpoints into it: ``LpipsAlex.from_parts``); None builds one with SEEDED-RANDOM weights - no weights are shipped, and such a number
    compares two tokenizers under one fixed random network, not with published LPIPS values.  The metric owns the network: it follows the
    metric to the device of the images.

    State: ``sum_scores`` float64 (1,) and ``total`` int64 (1,) on the device, additive (all-reduce them across ranks before ``compute``).
    ``update`` never synchronises; the per-sample fp32 scores are added to the float64 sum one by one in row order, so two updates of two
    pairs leave the same state bits as one update of four.  ``compute`` (the one synchronisation): sum / total for 'mean', the sum for
    'sum', as fp32; NaN when nothing was seen.

    Unlike torchmetrics the input VALUES are not range-checked (that would synchronise): out-of-range pixels are simply evaluated."""
    _STATE = (("sum_scores", torch.float64, 1), ("total", torch.int64, 1))

    def __init__(self, net_type='alex', reduction='mean', normalize=False, net=None, **kwargs):
        name = "LearnedPerceptualImagePatchSimilarity"
        _accept(name, kwargs, **_COMMON)
        if net_type in ('vgg', 'squeeze'):
            raise ValueError(f"{name}: net_type={net_type!r} is not built (supported: 'alex')")
        if net_type != 'alex':
            raise ValueError(f"{name}: net_type={net_type!r}: 'alex' expected")
        if reduction not in ('mean', 'sum'):
            raise ValueError(f"{name}: reduction={reduction!r}: 'mean' or 'sum' expected")
        if not isinstance(normalize, bool):
            raise ValueError(f"{name}: normalize={normalize!r}: a bool expected")
        from fourm.vq.percept_losses.lpips_alex import LpipsAlex
        if net is not None and not isinstance(net, LpipsAlex):
            raise TypeError(f"{name}: net has to be a LpipsAlex, got {type(net).__name__}")
        self.net_type, self.reduction, self.normalize = net_type, reduction, normalize
        self.net = LpipsAlex() if net is None else net
        super().__init__()

    def to(self, device):
        super().to(device)
        if device is not None:
            self.net.to(device)
        return self

    def update(self, img1: torch.Tensor, img2: torch.Tensor) -> None:
        self._update(img1, img2, self.normalize, False)

    def _update(self, img1, img2, normalize, clamp0):
        from fourm.utils.inception import ops as iops
        name = type(self).__name__
        for t in (img1, img2):
            if not torch.is_tensor(t) or t.dim() != 4 or t.shape[1] != 3 or t.shape[0] < 1:
                raise ValueError(f"{name}: images of shape (N, 3, H, W) expected, got {tuple(t.shape) if torch.is_tensor(t) else type(t).__name__}")
        if img1.shape != img2.shape:
            raise ValueError(f"{name}: img1 {tuple(img1.shape)} and img2 {tuple(img2.shape)} differ in shape")
        _on_gpu(name, img1, img2)
        device = img1.device
        self._state_on(device)
        if next(self.net.parameters()).device != device:
            self.net.to(device)
        scores = self.net.scores(img1, img2, normalize, clamp0=clamp0)
        with torch.no_grad(), torch.cuda.device(device):
            # the float64 column sum of fm_feature_moments: rows ascending, one thread, continuing from the stored sum; the count rides along
            iops.feature_moments(scores.view(-1, 1), self.sum_scores, torch.zeros(1, 1, dtype=torch.float64, device=device), self.total)

    def compute(self) -> torch.Tensor:
        if self.sum_scores is None:
            return self._nan()
        s, n = self.sum_scores[0], self.total[0]
        if self.reduction == 'mean':
            return (s / n.double()).float()
        return torch.where(n > 0, s, torch.full_like(s, float("nan"))).float()


# ---- the per-domain part of eval_metrics ----------------------------------------------------------------------------------------------------------
def domain_spec(domain: str) -> Tuple[Optional[int], str, bool, bool]:
    """-> (channels compared (None: all), transform, MS-SSIM?, IoU?) of a domain, upstream's table (run_training_vqvae.py:1469-1480, :1513-1537)."""
    dense = domain in DENSE_FEAT_MODALITIES
    sam = 'sam_mask' in domain
    ms_ssim, iou = not dense and not sam, not dense and sam
    if domain in ['rgb', 'normal']:
        return 3, DENORM, ms_ssim, iou
    if domain in ['depth']:
        return 1, RAW, ms_ssim, iou
    if domain in UNIT_RANGE_1CH:
        return 1, DENORM, ms_ssim, iou
    if sam:
        return 1, SIGMOID_PRED, ms_ssim, iou
    if domain in ['principal_curvature']:
        return 2, DENORM, ms_ssim, iou
    return None, RAW, ms_ssim, iou


class ReconstructionMetrics:
    """MSE, MAE, PSNR and MS-SSIM or IoU of one domain, as eval_metrics reports them.  ``update(output, images)`` takes the decoder output and the
    prepared input as they are (extra channels such as a validity mask included): the channel slice, the denormalisation (v + 1) / 2, the
    sigmoid of a ``sam_mask`` prediction and the clamp in front of the IoU happen in the kernels' loads, with no intermediate tensor.  One pass
    gives the three error metrics (and the IoU counts); MS-SSIM takes its pass per scale.

    ``lpips``: a ``LearnedPerceptualImagePatchSimilarity`` for domain ``rgb`` or ``normal`` (upstream's :1549): every ``update`` then also feeds
    it the first three channels of ``output``, clamped to [-1, 1] inside the stem's loads, and of ``images`` - upstream's
    ``lpips_metric.update(reconst.clamp(0, 1), gt)`` with ``normalize=True`` expressed on the raw [-1, 1] tensors, without the denormalise /
    renormalise round trip (the instance's own ``normalize`` setting is not consulted) - and ``compute`` reports ``LPIPS`` after ``MS-SSIM``.
    With the default None the keys and values are unchanged."""

    def __init__(self, domain: str, data_range: float = 1., lpips=None):
        self.domain = domain
        self.channels, self.transform, has_ms_ssim, self.has_iou = domain_spec(domain)
        if isinstance(data_range, bool) or not isinstance(data_range, (int, float)) or not data_range > 0:
            raise ValueError(f"ReconstructionMetrics: data_range={data_range!r}: a positive number expected")
        self.data_range = float(data_range)
        self.threshold = 0.5
        self.ms_ssim = MultiScaleStructuralSimilarityIndexMeasure(data_range=self.data_range, reduction='elementwise_mean', normalize=False) if has_ms_ssim else None
        self.sums = self.counts = None
        if lpips is not None:
            if not isinstance(lpips, LearnedPerceptualImagePatchSimilarity):
                raise TypeError(f"ReconstructionMetrics: lpips has to be a LearnedPerceptualImagePatchSimilarity, got {type(lpips).__name__}")
            if domain not in ('rgb', 'normal'):
                raise ValueError(f"ReconstructionMetrics: lpips is reported for the domains 'rgb' and 'normal' only, not for {domain!r}")
        self.lpips = lpips

    def reset(self):
        if self.sums is not None:
            self.sums.zero_()
            self.counts.zero_()
        if self.ms_ssim is not None:
            self.ms_ssim.reset()
        if self.lpips is not None:
            self.lpips.reset()

    def to(self, device):
        if self.sums is not None:
            self.sums, self.counts = self.sums.to(device), self.counts.to(device)
        if self.ms_ssim is not None:
            self.ms_ssim.to(device)
        if self.lpips is not None:
            self.lpips.to(device)
        return self

    def update(self, output: torch.Tensor, images: torch.Tensor) -> None:
        what = f"ReconstructionMetrics({self.domain!r})"
        _check_pair(what, output, images, same_channels=self.channels is None)
        c_use = output.shape[1] if self.channels is None else self.channels
        if c_use > min(output.shape[1], images.shape[1]):
            raise ValueError(f"{what}: {c_use} channels are compared, got output {tuple(output.shape)} and images {tuple(images.shape)}")
        if self.ms_ssim is not None:
            self.ms_ssim._check_size(output.shape[2], output.shape[3])
        _on_gpu(what, output, images)
        if self.sums is None or self.sums.device != output.device:
            old = self.sums, self.counts
            self.sums = torch.zeros(2, dtype=torch.float64, device=output.device) if old[0] is None else old[0].to(output.device)
            self.counts = torch.zeros(5, dtype=torch.int64, device=output.device) if old[1] is None else old[1].to(output.device)
        _accumulate_sums(what, output, images, self.sums, self.counts, c_use=c_use, transform=self.transform, iou=self.has_iou, threshold=self.threshold)
        if self.ms_ssim is not None:
            self.ms_ssim._update(output, images, c_use, self.transform)
        if self.lpips is not None:
            self.lpips._update(output[:, :3], images[:, :3], False, True)

    def compute(self, prefix: str = '[Eval]', eval_size=None) -> Dict[str, float]:
        """upstream's result keys, f'{prefix} MSE@{eval_size}' and so on, with Python floats (the one host synchronisation)."""
        key = lambda name: f'{prefix} {name}@{eval_size}'
        nan = float("nan")
        if self.sums is None:
            mse = mae = psnr = nan
        else:
            n = self.counts[3].double()
            m = self.sums[0] / n
            mse, mae, psnr = m.float().item(), (self.sums[1] / n).float().item(), _psnr(m, self.data_range).float().item()
        results = {key('MSE'): mse, key('MAE'): mae, key('PSNR'): psnr}
        if self.ms_ssim is not None:
            results[key('MS-SSIM')] = self.ms_ssim.compute().item()
        if self.lpips is not None:
            results[key('LPIPS')] = self.lpips.compute().item()
        if self.has_iou:
            results[key('IoU')] = nan if self.counts is None else _iou(self.counts).item()
        return results


# ---- token histogram -----------------------------------------------------------------------------------------------------------------------------
def token_histogram(tokens: torch.Tensor, codebook_size: int) -> torch.Tensor:
    """int64 (codebook_size,) occurrences of every token value (``np.bincount(tokens, minlength=codebook_size)``) on the device, by integer
    atomics.  ``tokens``: an integer tensor of any shape on the GPU.  ValueError: tokens outside [0, codebook_size) (counted on the device;
    reading that count is this call's one synchronisation)."""
    from fourm.hip import ops
    codebook_size = int(codebook_size)
    if not 1 <= codebook_size < 2 ** 31:
        raise ValueError(f"codebook_size {codebook_size}")
    if not torch.is_tensor(tokens) or tokens.is_floating_point() or tokens.is_complex() or tokens.dtype == torch.bool:
        raise ValueError("token_histogram: an integer tensor expected")
    _on_gpu("token_histogram", tokens)
    t = tokens.detach().reshape(-1)
    if t.dtype not in (torch.int64, torch.int32, torch.int16):
        t = t.to(torch.int64)
    t = t.contiguous()
    hist = torch.zeros(codebook_size, dtype=torch.int64, device=t.device)
    if t.numel() == 0:
        return hist
    bad = torch.empty(1, dtype=torch.int32, device=t.device)
    with torch.cuda.device(t.device):
        ops.token_histogram(t, codebook_size, hist, bad)
    n_bad = int(bad.item())
    if n_bad:
        raise ValueError(f"{n_bad} tokens lie outside [0, {codebook_size})")
    return hist
