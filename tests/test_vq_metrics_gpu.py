"""The tokenizer validation metrics on a real MI355X (fourm.vq.metrics, csrc/metrics.hip) against the float64 restatement of their definitions
on the CPU (tests/vq_metrics_util.py, whose docstring derives every bound): the sums (MSE, MAE, PSNR) within bounds from the formats, the IoU
counts exactly, SSIM at one scale and MS-SSIM within 4 x the error the same restatement shows in fp32 plus a floor of 4 fp32 ulps,
ReconstructionMetrics against the single metrics on converted tensors, token_histogram against torch.bincount."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from tests import vq_metrics_util as MU
from tests.parity_log import record

pytestmark = pytest.mark.gpu

DEV = "cuda"
TILE = 32          # FM_SSIM_TILE


def _M():
    from fourm.vq import metrics
    return metrics


def _ops():
    from fourm.hip import _lib as L, ops
    return L, ops


def _tid(transform):
    L, _ = _ops()
    return {"raw": L.METRIC_RAW, "denorm": L.METRIC_DENORM, "sigmoid_pred": L.METRIC_SIGMOID_PRED}[transform]


# ---- sums ------------------------------------------------------------------------------------------------------------------------------------------
SUM_CASES = [((3, 4, 37, 29), 3, "denorm"), ((2, 3, 96, 96), 3, "raw"), ((1, 1, 1, 1), 1, "raw")]


def _run_sums(pred, target, c_use, transform, iou=False):
    """fm_metric_sums with its accumulators in the middle of sentinel buffers -> (sums (2,) f64, counts (5,) int64) on the CPU."""
    _, ops = _ops()
    sbuf, sums = MU.sentinel_view((2,), torch.float64, DEV, -7.0)
    cbuf, counts = MU.sentinel_view((5,), torch.int64, DEV, -7)
    sums.zero_()
    counts.zero_()
    ops.metric_sums(pred, target, c_use, _tid(transform), sums, counts, iou=iou)
    assert MU.sentinels_intact(sbuf, 2, -7.0) and MU.sentinels_intact(cbuf, 5, -7), "fm_metric_sums wrote outside its accumulators"
    return sums.cpu(), counts.cpu()


@pytest.mark.parametrize("shape,c_use,transform", SUM_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_sums_against_float64(shape, c_use, transform):
    """MSE, MAE and PSNR against float64 on the converted fp32 inputs; bounds (6 + 1) U MSE, (2 + 1) U MAE, (10 / ln 10) 6 U + U |PSNR|, each
    with n 2^-53 for the double accumulation (tests/vq_metrics_util.py).  37 x 29 x 3 of 4 channels: the odd tail of a chunk and the channel
    stride; 2 x 3 x 96 x 96: 14 workgroups; one element.  Two runs give the same bits; nothing is written outside the accumulators; the public
    classes, fed the converted tensors, hold the same sums."""
    g = MU.gen(11 + shape[2])
    pred, target = (0.6 * torch.randn(shape, generator=g)).float(), (torch.rand(shape, generator=g) * 2 - 1).float()
    p64, t64 = MU.convert(pred, target, c_use, transform)
    ref = MU.error_sums(p64, t64)
    tol = MU.error_bounds(ref)
    sums, counts = _run_sums(pred.to(DEV), target.to(DEV), c_use, transform)
    sums2, counts2 = _run_sums(pred.to(DEV), target.to(DEV), c_use, transform)
    assert torch.equal(sums, sums2) and torch.equal(counts, counts2), "two runs differ"
    n = ref["n"]
    assert counts.tolist() == [0, 0, 0, n, 0]
    got = dict(mse=float(sums[0]) / n, mae=float(sums[1]) / n)
    got["psnr"] = 10 * math.log10(1.0 / got["mse"])
    ratios = {}
    for k in ("mse", "mae", "psnr"):
        err = abs(got[k] - float(ref[k]))
        ratios[k] = err / tol[k]
        print(f"{k}: got {got[k]!r} ref {float(ref[k])!r} err {err:.3e} tol {tol[k]:.3e}")
    record("test_sums_against_float64", shape=list(shape), **{f"{k}_err_over_tol": v for k, v in ratios.items()})
    assert all(v <= 1.0 for v in ratios.values()), ratios
    # the public classes on the converted tensors (the same elements in the same partition: the same bits)
    M = _M()
    pc, tc = p64.float().to(DEV), t64.float().to(DEV)
    mse, mae, psnr = M.MeanSquaredError(squared=True).to(DEV), M.MeanAbsoluteError().to(DEV), M.PeakSignalNoiseRatio(data_range=1.).to(DEV)
    for m in (mse, mae, psnr):
        m.update(pc, tc)
        assert torch.equal(m.sums.cpu(), sums) and m.counts.cpu().tolist() == [0, 0, 0, n, 0]
        out = m.compute()
        assert out.dim() == 0 and out.dtype == torch.float32
    assert abs(mse.compute().item() - float(ref["mse"])) <= tol["mse"] and abs(mae.compute().item() - float(ref["mae"])) <= tol["mae"]
    assert abs(psnr.compute().item() - float(ref["psnr"])) <= tol["psnr"]
    mse.reset()
    assert mse.sums.tolist() == [0.0, 0.0] and mse.counts.tolist() == [0] * 5


def test_updates_accumulate():
    """Three updates with batches 1, 2, 3 against one update of the concatenation: the counts exactly, the double sums within n 2^-53 of their
    value (the partition into workgroups differs), for the error sums and for MS-SSIM (whose per-image values do not depend on the batch)."""
    M = _M()
    pred, target = MU.structured_pair((6, 1, 176, 176), 0.1, 5)
    pred, target = pred.to(DEV), target.to(DEV)
    one_e, three_e = M.MeanSquaredError().to(DEV), M.MeanSquaredError().to(DEV)
    one_s, three_s = (M.MultiScaleStructuralSimilarityIndexMeasure(data_range=1.).to(DEV) for _ in range(2))
    one_e.update(pred, target)
    one_s.update(pred, target)
    for lo, hi in ((0, 1), (1, 3), (3, 6)):
        three_e.update(pred[lo:hi], target[lo:hi])
        three_s.update(pred[lo:hi], target[lo:hi])
    assert torch.equal(one_e.counts, three_e.counts) and one_e.counts[3].item() == pred.numel()
    assert torch.equal(one_s.total, three_s.total) and one_s.total.item() == 6
    rel = pred.numel() * 2.0 ** -53
    for a, b in zip(one_e.sums.tolist() + one_s.similarity.tolist(), three_e.sums.tolist() + three_s.similarity.tolist()):
        assert abs(a - b) <= rel * abs(a), (a, b)


# ---- IoU ---------------------------------------------------------------------------------------------------------------------------------------------
def _iou_inputs(seed, shape=(2, 1, 37, 29)):
    g = MU.gen(seed)
    pred = torch.rand(shape, generator=g) * 1.6 - 0.3          # below 0 and above 1 included
    pred.view(-1)[::7] = 0.5                                    # exactly at the threshold: not positive
    pred.view(-1)[3::11] = -0.25
    pred.view(-1)[5::13] = 1.5
    target = (torch.rand(shape, generator=g) < 0.4).float()
    return pred.float(), target


def test_iou_counts_are_exact():
    """BinaryJaccardIndex on predictions that include exactly 0.5, values below 0 and above 1: tp, fp, fn and n equal the host's.  The sam_mask
    path of ReconstructionMetrics (sigmoid in the load): logits are 0 exactly (sigmoid = 0.5 exactly, not positive) or at least 1e-3 away
    from it, where the sigmoid is 2.5e-4 from the threshold - four orders above the fp32 sigmoid's error - so the counts are exact too."""
    M = _M()
    pred, target = _iou_inputs(3)
    tp, fp, fn, n = MU.iou_counts(pred.double(), target.double())
    assert tp > 50 and fp > 50 and fn > 50
    m = M.BinaryJaccardIndex().to(DEV)
    m.update(pred.to(DEV), target.to(DEV))
    assert m.counts.tolist() == [tp, fp, fn, n, 0]
    out = m.compute()
    assert out.dim() == 0 and out.item() == torch.tensor(tp / (tp + fp + fn), dtype=torch.float64).float().item()
    m.update(pred.to(DEV), target.to(DEV))
    assert m.counts.tolist() == [2 * tp, 2 * fp, 2 * fn, 2 * n, 0]
    m.reset()
    assert m.counts.tolist() == [0] * 5
    # sigmoid path
    g = MU.gen(4)
    logits = torch.randn(2, 2, 37, 29, generator=g) * 3
    logits = torch.where(logits.abs() < 1e-3, torch.full_like(logits, 1e-3), logits)
    logits.view(-1)[::9] = 0.0
    images = torch.cat([target, torch.rand(2, 2, 37, 29, generator=g)], 1)          # extra channels hold anything
    p64, t64 = MU.convert(logits, images, 1, "sigmoid_pred")
    tp, fp, fn, n = MU.iou_counts(p64, t64)
    r = M.ReconstructionMetrics('sam_mask_x')
    r.update(logits.to(DEV), images.to(DEV))
    assert r.counts.tolist() == [tp, fp, fn, n, 0]
    assert r.compute('[Eval]', 224)['[Eval] IoU@224'] == torch.tensor(tp / (tp + fp + fn), dtype=torch.float64).float().item()


def test_iou_refuses_other_targets_at_compute():
    M = _M()
    pred, target = _iou_inputs(6)
    target.view(-1)[17] = 0.3
    target.view(-1)[400] = 0.3
    m = M.BinaryJaccardIndex().to(DEV)
    m.update(pred.to(DEV), target.to(DEV))          # counted on the device, no synchronisation here
    assert m.counts[4].item() == 2
    with pytest.raises(ValueError, match="2 target values are neither 0 nor 1"):
        m.compute()
    r = M.ReconstructionMetrics('sam_mask')
    r.update(pred.to(DEV), target.to(DEV))
    with pytest.raises(ValueError, match="neither 0 nor 1"):
        r.compute()


# ---- SSIM at one scale -----------------------------------------------------------------------------------------------------------------------------
SCALE_SHAPES = [(2, 3, 11, 11), (1, 1, 12, 43), (2, 2, 45, 33),
                (1, 2, TILE + 9, 2 * TILE + 10), (1, 1, TILE + 10, TILE + 11), (1, 1, TILE + 11, TILE + 10), (2, 1, 2 * TILE + 10, TILE + 9)]


def _run_scale(x, y, c_use, transform, c1=1e-4, c2=9e-4):
    _, ops = _ops()
    B = x.shape[0]
    sbuf, ssim = MU.sentinel_view((B,), torch.float64, DEV, -7.0)
    cbuf, cs = MU.sentinel_view((B,), torch.float64, DEV, -7.0)
    ops.ssim_scale(x, y, c_use, _tid(transform), MU.window().to(DEV), c1, c2, ssim, cs)
    assert MU.sentinels_intact(sbuf, B, -7.0) and MU.sentinels_intact(cbuf, B, -7.0), "fm_ssim_scale wrote outside its outputs"
    return ssim.cpu(), cs.cpu()


@pytest.mark.parametrize("shape", SCALE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_ssim_scale_against_float64(shape):
    """Per-image ssim and cs of one scale against the float64 restatement.  A single window; one row of windows; two channels and images; then,
    with the kernel's tile edge T = 32, heights and widths T + 9, T + 10, T + 11 and 2 T + 10, i.e. T - 1, T, T + 1 and 2 T window positions: a
    tile one row / column short of full, exactly full, a second tile that holds a single row / column, two full tiles.  The bound of a shape: 4 x the largest error of the fp32 restatement
    over its per-image ssim and cs values + 4 fp32 ulps of the value (tests/vq_metrics_util.py).  Two runs give the same bits."""
    pred, target = MU.structured_pair(shape, 0.1, 20 + shape[2] + shape[3])
    win = MU.window()
    s64, c64 = MU.ssim_scale(pred.double(), target.double(), win, 1e-4, 9e-4)
    s32, c32 = MU.ssim_scale(pred, target, win, 1e-4, 9e-4)
    tol, base = MU.ssim_tol(torch.cat([s64, c64]), torch.cat([s32, c32]))
    ssim, cs = _run_scale(pred.to(DEV), target.to(DEV), shape[1], "raw")
    ssim2, cs2 = _run_scale(pred.to(DEV), target.to(DEV), shape[1], "raw")
    assert torch.equal(ssim, ssim2) and torch.equal(cs, cs2), "two runs differ"
    err = max(float((ssim - s64).abs().max()), float((cs - c64).abs().max()))
    print(f"{shape}: ssim {ssim.tolist()} cs {cs.tolist()} err {err:.3e} fp32 restatement {base:.3e} tol {tol:.3e}")
    record("test_ssim_scale_against_float64", shape=list(shape), err=err, fp32_restatement_err=base, tol=tol, err_over_fp32=err / base if base else None)
    assert err <= tol, (err, base, tol)


def test_ssim_scale_and_pooling_convert_in_the_load():
    """The channel slice and the denormalisation inside the loads: images with 3 and 2 channels of which 2 are compared, against the same kernel
    on the converted tensors (the same values reach the same arithmetic: the same bits).  fm_avgpool2x2_pair on odd sizes against the float64
    mean of the converted values: ((a + b) + (c + d)) / 4 rounds twice on the way and once at the end, 3 U of the mean of the magnitudes."""
    _, ops = _ops()
    g = MU.gen(8)
    x, y = (torch.rand(2, 3, 45, 33, generator=g) * 2 - 1).float(), (torch.rand(2, 2, 45, 33, generator=g) * 2 - 1).float()
    x64, y64 = MU.convert(x, y, 2, "denorm")
    a = _run_scale(x.to(DEV), y.to(DEV), 2, "denorm")
    b = _run_scale(x64.float().to(DEV), y64.float().to(DEV), 2, "raw")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    xbuf, xo = MU.sentinel_view((2, 2, 22, 16), torch.float32, DEV, -7.0)
    ybuf, yo = MU.sentinel_view((2, 2, 22, 16), torch.float32, DEV, -7.0)
    ops.avgpool2x2_pair(x.to(DEV), y.to(DEV), 2, _tid("denorm"), xo, yo)
    assert MU.sentinels_intact(xbuf, xo.numel(), -7.0) and MU.sentinels_intact(ybuf, yo.numel(), -7.0), "fm_avgpool2x2_pair wrote outside its outputs"
    for got, src in ((xo, x64), (yo, y64)):
        want, mag = F.avg_pool2d(src, 2), F.avg_pool2d(src.abs(), 2)
        assert want.shape == got.shape
        assert bool(((got.cpu().double() - want).abs() <= 3 * MU.U * mag).all())


# ---- MS-SSIM -----------------------------------------------------------------------------------------------------------------------------------------
MS_SHAPES = [(2, 3, 176, 176), (3, 1, 181, 176), (2, 2, 176, 200)]
MS_SIGMAS = [0.02, 0.1, 0.3]


@functools.lru_cache(maxsize=None)
def _ms_case(shape, sigma):
    pred, target = MU.structured_pair(shape, sigma, 40 + shape[3] + int(100 * sigma))
    v64, t64 = MU.ms_ssim(pred.double(), target.double())
    v32, _ = MU.ms_ssim(pred, target)
    return pred, target, v64, t64, v32


@pytest.mark.parametrize("sigma", MS_SIGMAS)
@pytest.mark.parametrize("shape", MS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_ms_ssim_against_float64(shape, sigma):
    """The metric (mean over the images of prod cs_i^beta_i ssim_4^beta_4, five scales) against the float64 restatement, normalize=False as
    upstream sets it.  Every per-scale term of the reference is positive on these inputs, so the reference is finite: asserted, nothing is
    skipped or masked.  181 rows: an odd size through the pooling.  Bound: 4 x the error of the fp32 restatement of this case + 4 fp32 ulps
    of the value.  The float64 state is compared; compute() is its fp32 rounding."""
    M = _M()
    pred, target, v64, t64, v32 = _ms_case(shape, sigma)
    assert bool((t64 > 0).all()) and bool(torch.isfinite(v64).all()), "the reference has to be finite on these inputs"
    want, base32 = v64.mean(), v32.mean().double()
    tol, base = MU.ssim_tol(want, base32)
    m = M.MultiScaleStructuralSimilarityIndexMeasure(data_range=1., reduction='elementwise_mean', normalize=False, sync_on_compute=True, compute_on_cpu=False).to(DEV)
    m.update(pred.to(DEV), target.to(DEV))
    got = (m.similarity[0] / m.total[0].double()).item()
    err = abs(got - float(want))
    print(f"{shape} sigma {sigma}: got {got!r} ref {float(want)!r} smallest term {float(t64.min()):.3f} err {err:.3e} fp32 restatement {base:.3e} tol {tol:.3e}")
    record("test_ms_ssim_against_float64", shape=list(shape), sigma=sigma, value=float(want), err=err, fp32_restatement_err=base, tol=tol, err_over_fp32=err / base if base else None)
    assert math.isfinite(got) and err <= tol, (got, float(want), err, base, tol)
    out = m.compute()
    assert out.dim() == 0 and out.dtype == torch.float32 and out.item() == torch.tensor(got, dtype=torch.float64).float().item()
    m2 = M.MultiScaleStructuralSimilarityIndexMeasure(data_range=1.).to(DEV)
    m2.update(pred.to(DEV), target.to(DEV))
    assert torch.equal(m2.similarity, m.similarity), "two runs differ"


def test_ms_ssim_of_anticorrelated_images_is_nan_unless_relu():
    M = _M()
    _, target = MU.structured_pair((2, 1, 176, 176), 0.0, 2)
    pred = 1 - target
    _, terms = MU.ms_ssim(pred.double(), target.double())
    assert bool((terms < 0).any())
    for normalize in (None, False):
        m = M.MultiScaleStructuralSimilarityIndexMeasure(data_range=1., normalize=normalize).to(DEV)
        m.update(pred.to(DEV), target.to(DEV))
        assert math.isnan(m.compute().item())
    m = M.MultiScaleStructuralSimilarityIndexMeasure(data_range=1., normalize='relu').to(DEV)
    m.update(pred.to(DEV), target.to(DEV))
    want, _ = MU.ms_ssim(pred.double(), target.double(), normalize="relu")
    assert math.isfinite(m.compute().item()) and abs(m.compute().item() - float(want.mean())) <= 1e-5


# ---- ReconstructionMetrics ---------------------------------------------------------------------------------------------------------------------------
RECON_CASES = [("rgb", (2, 4, 176, 176), (2, 5, 176, 176)), ("depth", (2, 2, 176, 181), (2, 3, 176, 181)), ("sam_mask_x", (2, 2, 37, 29), (2, 3, 37, 29)),
               ("CLIP-B16", (2, 6, 14, 14), (2, 6, 14, 14))]


@pytest.mark.parametrize("domain,oshape,ishape", RECON_CASES, ids=[c[0] for c in RECON_CASES])
def test_reconstruction_metrics_equal_the_single_metrics(domain, oshape, ishape):
    """update(output, images) on tensors with extra channels against the single metrics fed the converted tensors, which are built with torch
    ops on the CPU as eval_metrics builds them.  Slice and denormalisation are exact in fp32 and the kernels partition the compared elements
    alike, so 'rgb', 'depth' and 'CLIP-B16' agree to the bit.  'sam_mask_x': the sigmoid of the load and torch's differ by rounding, each
    within EPS_SIGMOID of the exact one: MSE and MAE agree within the sum of both bounds (error_bounds(sigmoid=True)), the IoU exactly (logits
    at least 1e-3 from 0)."""
    M = _M()
    channels, transform, has_ms, has_iou = M.domain_spec(domain)
    if has_ms:
        sp, st = MU.structured_pair((oshape[0], max(oshape[1], ishape[1]), oshape[2], oshape[3]), 0.1, 9)
        scale = (lambda v: v * 2 - 1) if transform == "denorm" else (lambda v: v)
        output, images = scale(sp[:, :oshape[1]]).contiguous(), scale(st[:, :ishape[1]]).contiguous()
    else:
        g = MU.gen(10)
        output, images = torch.randn(oshape, generator=g) * 2, torch.randn(ishape, generator=g)
        if has_iou:
            output = torch.where(output.abs() < 1e-3, torch.full_like(output, 1e-3), output)
            images[:, :1] = (images[:, :1] > 0.3).float()
    # eval_metrics' conversion, fp32 torch ops on the CPU
    if transform == "denorm":
        gt, reconst = (images[:, :channels] + 1.0) / 2.0, (output[:, :channels] + 1.0) / 2.0
    elif transform == "sigmoid_pred":
        gt, reconst = images[:, :1], torch.sigmoid(output)[:, :1]
    elif channels is not None:
        gt, reconst = images[:, :channels], output[:, :channels]
    else:
        gt, reconst = images.contiguous(), output.contiguous()
    gt, reconst = gt.contiguous().to(DEV), reconst.contiguous().to(DEV)
    single = {"MSE": M.MeanSquaredError(squared=True), "MAE": M.MeanAbsoluteError(), "PSNR": M.PeakSignalNoiseRatio(data_range=1.)}
    if has_ms:
        single["MS-SSIM"] = M.MultiScaleStructuralSimilarityIndexMeasure(data_range=1., reduction='elementwise_mean', normalize=False)
    if has_iou:
        single["IoU"] = M.BinaryJaccardIndex()
    want = {}
    for name, m in single.items():
        m.to(DEV).update(reconst.clamp(0, 1) if name == "IoU" else reconst, gt)
        want[f"[Val] {name}@224"] = m.compute().item()
    r = M.ReconstructionMetrics(domain)
    for _ in range(2):          # reset() gives the same again
        r.update(output.to(DEV), images.to(DEV))
        got = r.compute('[Val]', 224)
        assert set(got) == set(want) and all(isinstance(v, float) for v in got.values())
        if transform != "sigmoid_pred":
            assert got == want, (got, want)
        else:
            p64, t64 = MU.convert(output, images, 1, "sigmoid_pred")
            tol = MU.error_bounds(MU.error_sums(p64, t64), sigmoid=True)
            assert got["[Val] IoU@224"] == want["[Val] IoU@224"]
            for name, k in (("MSE", "mse"), ("MAE", "mae"), ("PSNR", "psnr")):
                assert abs(got[f"[Val] {name}@224"] - want[f"[Val] {name}@224"]) <= 2 * tol[k], (name, got, want, tol)
        r.reset()


# ---- token histogram -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [64, 16384])
@pytest.mark.parametrize("dtype", [torch.int16, torch.int32, torch.int64], ids=["int16", "int32", "int64"])
def test_token_histogram_equals_bincount(dtype, K):
    M = _M()
    g = MU.gen(K)
    tokens = torch.cat([torch.randint(0, K, (40000,), generator=g), torch.full((777,), K - 1), torch.zeros(13, dtype=torch.int64)]).to(dtype).view(10, -1)
    want = torch.bincount(tokens.flatten().long(), minlength=K)
    got = M.token_histogram(tokens.to(DEV), K)
    assert got.dtype == torch.int64 and got.shape == (K,) and got.is_cuda and torch.equal(got.cpu(), want)
    assert torch.equal(M.token_histogram(tokens.to(DEV), K), got)
    for bad_value in (K, -1):
        bad = tokens.clone()
        bad[3, 5] = bad_value
        with pytest.raises(ValueError, match="1 tokens lie outside"):
            M.token_histogram(bad.to(DEV), K)
