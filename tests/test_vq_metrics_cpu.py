"""The tokenizer validation metrics without a GPU: the C ABI additions (header, exports, ctypes prototypes, the build), the refusals of
fourm.vq.metrics, the domain table of ReconstructionMetrics, and the float64 restatement of the definitions (tests/vq_metrics_util.py) against
closed forms.  The kernels themselves are tested on the GPU (tests/test_vq_metrics_gpu.py)."""
import ctypes
import importlib.util
import math
import os
import re

import pytest
import torch

from tests import vq_metrics_util as MU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["fm_metric_sums_scratch", "fm_metric_sums", "fm_ssim_scale_scratch", "fm_ssim_scale", "fm_avgpool2x2_pair", "fm_token_histogram"]


def _header():
    return open(os.path.join(ROOT, "include", "fourm_hip.h")).read()


def test_abi_additions_are_declared_exported_and_built():
    from fourm.hip import _lib
    header = _header()
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib.EXPORTS and hasattr(_lib.lib, name), name
    assert _lib.ABI_VERSION == 11 and _lib.lib.fm_abi_version() == 11 and re.search(r"#define FM_ABI_VERSION 11\b", header)          # purely additive
    for name, val in dict(FM_METRIC_RAW=_lib.METRIC_RAW, FM_METRIC_DENORM=_lib.METRIC_DENORM, FM_METRIC_SIGMOID_PRED=_lib.METRIC_SIGMOID_PRED,
                          FM_METRIC_CHUNK=_lib.METRIC_CHUNK, FM_SSIM_TILE=_lib.SSIM_TILE, FM_SSIM_MAX_KERNEL=_lib.SSIM_MAX_KERNEL).items():
        assert re.search(rf"{name}\s*(=|\s)\s*{val}\b", header), name
    spec = importlib.util.spec_from_file_location("build_ext", os.path.join(ROOT, "ml-4m_amd", "build_ext.py"))
    be = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(be)
    assert "metrics.hip" in be.SOURCES and "-ffp-contract=off" in be.EXTRA_FLAGS["metrics.hip"]
    assert os.path.exists(os.path.join(ROOT, "ml-4m_amd", "csrc", "metrics.hip"))


def test_ctypes_prototypes_of_the_new_entry_points():
    """Parameter by parameter against the header: pointers void*, float c_float (c1, c2, threshold: no double crosses the ABI), int64_t c_int64,
    the stream last."""
    from fourm.hip import _lib
    header = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name in NEW:
        params = re.search(r"\bint %s\(([^)]*)\)\s*;" % name, header).group(1)
        plist = [p.strip() for p in params.split(",")]
        fn = getattr(_lib.lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == len(plist), name
        assert "double" not in params
        for at, decl in zip(fn.argtypes, plist):
            want = ctypes.c_void_p if "*" in decl else ctypes.c_float if decl.startswith("float") else ctypes.c_int64 if decl.startswith("int64_t") else ctypes.c_int
            assert at is want, (name, decl, at)
        if not name.endswith("_scratch"):
            assert plist[-1] == "void* stream", name


def test_constructors_take_upstreams_calls_and_refuse_other_values():
    from fourm.vq import metrics as M
    for compute_on_cpu in (False, True):          # eval_metrics' constructor calls, verbatim
        M.MeanSquaredError(squared=True, sync_on_compute=True, compute_on_cpu=compute_on_cpu).to("cpu")
        M.MeanAbsoluteError(sync_on_compute=True, compute_on_cpu=compute_on_cpu).to("cpu")
        M.PeakSignalNoiseRatio(data_range=1., reduction='elementwise_mean', sync_on_compute=True, compute_on_cpu=compute_on_cpu).to("cpu")
        M.MultiScaleStructuralSimilarityIndexMeasure(data_range=1., reduction='elementwise_mean', normalize=False, sync_on_compute=True, compute_on_cpu=compute_on_cpu).to("cpu")
    M.BinaryJaccardIndex().to("cpu")
    m = M.MultiScaleStructuralSimilarityIndexMeasure(data_range=1.)
    assert (m.kernel_size, m.sigma, m.betas, m.normalize) == (11, 1.5, (0.0448, 0.2856, 0.3001, 0.2363, 0.1333), None)
    assert M.MultiScaleStructuralSimilarityIndexMeasure(data_range=1., normalize='relu').normalize == 'relu'
    assert M.BinaryJaccardIndex().threshold == 0.5 and M.BinaryJaccardIndex(threshold=0.25).threshold == 0.25
    for make in (lambda: M.MeanSquaredError(squared=False), lambda: M.MeanSquaredError(sync_on_compute="yes"), lambda: M.MeanAbsoluteError(compute_on_cpu=1),
                 lambda: M.PeakSignalNoiseRatio(data_range=1., reduction='sum'), lambda: M.PeakSignalNoiseRatio(data_range=1., reduction=None),
                 lambda: M.PeakSignalNoiseRatio(), lambda: M.MultiScaleStructuralSimilarityIndexMeasure(data_range=1., reduction='none'),
                 lambda: M.MultiScaleStructuralSimilarityIndexMeasure(data_range=1., normalize='simple'), lambda: M.MultiScaleStructuralSimilarityIndexMeasure(data_range=1., kernel_size=8),
                 lambda: M.MultiScaleStructuralSimilarityIndexMeasure(data_range=1., kernel_size=13), lambda: M.MultiScaleStructuralSimilarityIndexMeasure(),
                 lambda: M.BinaryJaccardIndex(threshold=1.5), lambda: M.BinaryJaccardIndex(compute_on_cpu="no")):
        with pytest.raises(ValueError):
            make()
    with pytest.raises(TypeError):
        M.MeanAbsoluteError(average="macro")
    # nothing seen: nan, no state, no device touched
    assert math.isnan(M.MeanSquaredError().compute().item()) and M.MeanSquaredError().compute().dim() == 0


def test_updates_refuse_before_any_launch():
    from fourm.vq import metrics as M
    x, t = torch.rand(2, 3, 176, 176), torch.rand(2, 3, 176, 176)
    every = [M.MeanSquaredError(), M.MeanAbsoluteError(), M.PeakSignalNoiseRatio(data_range=1.), M.MultiScaleStructuralSimilarityIndexMeasure(data_range=1.),
             M.BinaryJaccardIndex(), M.ReconstructionMetrics('rgb'), M.ReconstructionMetrics('sam_mask_x'), M.ReconstructionMetrics('CLIP-B16')]
    for m in every:
        with pytest.raises(RuntimeError, match="HIP kernels only"):          # CPU tensors: the convention of fourm.vq.training
            m.update(x, t)
        with pytest.raises(ValueError, match="differ in shape"):
            m.update(x, t[:, :, :175])
        with pytest.raises(TypeError, match="fp32"):
            m.update(x.double(), t.double())
        with pytest.raises(TypeError, match="fp32"):
            m.update(x, t.half())
        with pytest.raises(ValueError):
            m.update(x[0], t[0])
    with pytest.raises(ValueError, match="differ in shape"):
        M.MeanSquaredError().update(x, t[:, :2])
    with pytest.raises(ValueError, match="channels"):
        M.ReconstructionMetrics('rgb').update(x[:, :2], t)
    # MS-SSIM: min(H, W) <= (kernel_size - 1) * 2^(scales - 1) = 160 with the defaults
    small = torch.rand(1, 3, 200, 160)
    for m in (M.MultiScaleStructuralSimilarityIndexMeasure(data_range=1.), M.ReconstructionMetrics('rgb'), M.ReconstructionMetrics('semseg_coco')):
        with pytest.raises(ValueError, match="160"):
            m.update(small, small)
    with pytest.raises(RuntimeError, match="HIP kernels only"):          # 161 passes the size check and reaches the device check
        M.MultiScaleStructuralSimilarityIndexMeasure(data_range=1.).update(torch.rand(1, 1, 161, 161), torch.rand(1, 1, 161, 161))
    with pytest.raises(ValueError, match="40"):
        M.MultiScaleStructuralSimilarityIndexMeasure(data_range=1., betas=(0.3, 0.3, 0.4)).update(small[:, :, :40, :40], small[:, :, :40, :40])
    with pytest.raises(RuntimeError, match="HIP kernels only"):          # domains without MS-SSIM take small images
        M.ReconstructionMetrics('sam_mask').update(small[:, :1], small[:, :1])
    with pytest.raises(RuntimeError, match="HIP kernels only"):
        M.token_histogram(torch.zeros(4, dtype=torch.int64), 8)
    with pytest.raises(ValueError):
        M.token_histogram(torch.zeros(4), 8)
    with pytest.raises(ValueError, match="codebook_size"):
        M.token_histogram(torch.zeros(4, dtype=torch.int64), 0)


def test_domain_table_follows_upstreams_eval_metrics():
    """(channels, transform, MS-SSIM, IoU) of every domain eval_metrics names (run_training_vqvae.py:1469-1480, :1513-1537)."""
    from fourm.vq import metrics as M
    want = {"rgb": (3, "denorm", True, False), "normal": (3, "denorm", True, False), "depth": (1, "raw", True, False),
            "edge_occlusion": (1, "denorm", True, False), "edge_texture": (1, "denorm", True, False), "keypoints2d": (1, "denorm", True, False),
            "keypoints3d": (1, "denorm", True, False), "reshading": (1, "denorm", True, False), "principal_curvature": (2, "denorm", True, False),
            "sam_mask": (1, "sigmoid_pred", False, True), "sam_mask_x": (1, "sigmoid_pred", False, True),
            "semseg_coco": (None, "raw", True, False)}
    want.update({d: (None, "raw", False, False) for d in MU.DENSE_FEAT_MODALITIES})
    assert M.DENSE_FEAT_MODALITIES == MU.DENSE_FEAT_MODALITIES == ['CLIP-B16', 'CLIP-L14', 'DINOv2-B14', 'DINOv2-G14', 'ImageBind-H14']
    for domain, spec in want.items():
        assert M.domain_spec(domain) == spec, domain
        r = M.ReconstructionMetrics(domain)
        assert (r.channels, r.transform, r.ms_ssim is not None, r.has_iou) == spec, domain
        keys = set(r.compute('[Eval]', 224))
        assert keys == {'[Eval] MSE@224', '[Eval] MAE@224', '[Eval] PSNR@224'} | ({'[Eval] MS-SSIM@224'} if spec[2] else set()) | ({'[Eval] IoU@224'} if spec[3] else set())
    r = M.ReconstructionMetrics('rgb')
    assert r.ms_ssim.normalize is None and r.ms_ssim.data_range == 1.0 and r.ms_ssim.kernel_size == 11          # upstream's normalize=False


def test_window_sums_to_one_and_is_symmetric():
    from fourm.vq import metrics as M
    for k, sigma in ((11, 1.5), (7, 1.0), (3, 0.5), (1, 1.5)):
        g = MU.window(k, sigma)
        assert g.dtype == torch.float32 and g.shape == (k,) and torch.equal(g, g.flip(0))
        assert abs(float(g.double().sum()) - 1.0) <= k * MU.U          # each tap rounded once
        assert torch.equal(M.gaussian_window(k, sigma), g)
    g = MU.window().double()
    assert abs(float(g[5] / g[4]) - math.exp(1 / (2 * 1.5 ** 2))) < 1e-6          # g_i proportional to exp(-((i - 5) / sigma)^2 / 2)


def test_restatement_of_identical_images_is_one():
    x, _ = MU.structured_pair((2, 3, 176, 181), 0.1, 0)
    ssim, cs = MU.ssim_scale(x.double(), x.double(), MU.window(), 1e-4, 9e-4)
    assert torch.allclose(ssim, torch.ones(2, dtype=torch.float64), rtol=0, atol=1e-12) and torch.allclose(cs, torch.ones(2, dtype=torch.float64), rtol=0, atol=1e-12)
    val, terms = MU.ms_ssim(x.double(), x.double())
    assert terms.shape == (5, 2) and torch.allclose(val, torch.ones(2, dtype=torch.float64), rtol=0, atol=1e-12)


def test_restatement_of_constant_images_has_the_closed_form():
    """Two constant images a, b: the variances and the covariance vanish, cs = 1 and ssim = (2 a b + c1) / (a^2 + b^2 + c1) at every scale -
    up to what the window's fp32 taps miss a sum of 1 by: with s = (sum g)^2 the moments are s a, s a^2, ..., so a variance is a^2 (s - s^2)
    instead of 0 and cs = 1 + (s - s^2) (2 a b - a^2 - b^2) / c2 to first order; the luminance term moves by at most 2 |s^2 - 1|."""
    a, b, c1, c2 = 0.25, 0.75, 1e-4, 9e-4
    x, y = torch.full((1, 2, 176, 176), a, dtype=torch.float64), torch.full((1, 2, 176, 176), b, dtype=torch.float64)
    want = (2 * a * b + c1) / (a * a + b * b + c1)
    s = float(MU.window().double().sum()) ** 2
    tol_cs = 2 * abs(s - s * s) * (a + b) ** 2 / c2 + 1e-12
    tol_ssim = tol_cs + 2 * abs(s * s - 1) + 1e-12
    assert tol_ssim < 1e-3
    val, terms = MU.ms_ssim(x, y)
    assert torch.allclose(terms[:4], torch.ones(4, 1, dtype=torch.float64), rtol=0, atol=tol_cs)
    assert abs(float(terms[4]) - want) <= tol_ssim and abs(float(val) - want ** MU.BETAS[4]) <= 4 * tol_cs + tol_ssim
    for size in (11, 12, 43):          # one scale, down to a single window
        ssim, cs = MU.ssim_scale(x[:, :, :size, :size], y[:, :, :size, :size], MU.window(), c1, c2)
        assert abs(float(ssim) - want) <= tol_ssim and abs(float(cs) - 1.0) <= tol_cs


def test_restatement_psnr_of_a_constant_offset():
    t = torch.rand(2, 3, 8, 8, generator=MU.gen(1)).double()
    for delta in (0.5, 0.1, 1e-3):
        ref = MU.error_sums(t + delta, t)
        assert abs(float(ref["psnr"]) + 20 * math.log10(delta)) < 1e-9 and abs(float(ref["mse"]) - delta ** 2) < 1e-12 and abs(float(ref["mae"]) - delta) < 1e-12


def test_restatement_anticorrelated_images_are_nan_unless_relu():
    _, t = MU.structured_pair((1, 1, 176, 176), 0.0, 2)
    val, terms = MU.ms_ssim((1 - t).double(), t.double())
    assert bool((terms < 0).any()) and math.isnan(float(val))
    val, _ = MU.ms_ssim((1 - t).double(), t.double(), normalize="relu")
    assert math.isfinite(float(val))


def test_restatement_conversions_and_iou():
    p = torch.tensor([-1.0, 0.0, 0.5, 1.0]).view(1, 1, 2, 2)
    a, b = MU.convert(torch.cat([p, p + 7], 1), torch.cat([p.flip(3), p], 1), 1, "denorm")
    assert a.dtype == torch.float64 and torch.equal(a, torch.tensor([0.0, 0.5, 0.75, 1.0], dtype=torch.float64).view(1, 1, 2, 2)) and b.shape == (1, 1, 2, 2)
    s, _ = MU.convert(p, p, 1, "sigmoid_pred")
    assert float(s.flatten()[1]) == 0.5
    pred = torch.tensor([0.5, 0.6, -3.0, 4.0, 0.2, 0.9], dtype=torch.float64)
    targ = torch.tensor([1.0, 1.0, 1.0, 0.0, 0.0, 0.0], dtype=torch.float64)
    assert MU.iou_counts(pred, targ) == (1, 2, 2, 6)          # exactly 0.5 is not positive; 4.0 clamps to 1


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """-1 with a message, decided on the host before the first launch (so it can be seen without a GPU): null and misaligned pointers, sizes,
    C_use above a channel count, an unknown transform, windows that are even, too long or longer than the image.  The scratch sizes of valid
    shapes: two doubles per workgroup of the main launch."""
    from fourm.hip import _lib as L
    assert L.metric_sums_scratch(2, 3, 96 * 96) == 2 * 14 and L.metric_sums_scratch(1, 1, 1) == 2 and L.metric_sums_scratch(3, 3, 37 * 29) == 2 * 3
    assert L.ssim_scale_scratch(2, 3, 11, 11, 11) == 2 * 6 and L.ssim_scale_scratch(1, 2, 41, 74, 11) == 2 * 2 * 2 and L.ssim_scale_scratch(1, 1, 43, 42, 11) == 2 * 2
    assert L.ssim_scale_scratch(1, 1, 42, 42, 11) == 2 and L.ssim_scale_scratch(2, 3, 176, 176, 11) == 2 * 6 * 36
    for bad in (L.metric_sums_scratch(0, 1, 1), L.metric_sums_scratch(1, 0, 1), L.metric_sums_scratch(1, 1, 0), L.ssim_scale_scratch(1, 1, 10, 11, 11),
                L.ssim_scale_scratch(1, 1, 11, 10, 11), L.ssim_scale_scratch(1, 1, 64, 64, 12), L.ssim_scale_scratch(1, 1, 64, 64, 13), L.ssim_scale_scratch(1, 1, 64, 64, 0),
                L.ssim_scale_scratch(0, 1, 64, 64, 11)):
        assert bad == -1 and L.lib.fm_last_error()
    buf = (ctypes.c_double * 64)()          # host memory: never reached, every call below is refused first
    p = ctypes.addressof(buf)
    ok = dict(B=1, Cp=2, Ct=2, C_use=2, HW=16, transform=L.METRIC_RAW)

    def sums(pred=p, target=p, scratch=p, sums_=p, counts=p, **kw):
        a = dict(ok, **kw)
        return L.metric_sums(pred, target, a["B"], a["Cp"], a["Ct"], a["C_use"], a["HW"], a["transform"], 0, 0.5, scratch, sums_, counts, None)
    for rc in (sums(pred=None), sums(target=None), sums(scratch=None), sums(sums_=None), sums(counts=None), sums(C_use=3), sums(Ct=1), sums(B=0), sums(HW=0),
               sums(transform=3), sums(transform=-1), sums(pred=p + 2), sums(sums_=p + 4), sums(counts=p + 4), sums(scratch=p + 4)):
        assert rc == -1

    def scale(x=p, y=p, window=p, scratch=p, ssim=p, cs=p, B=1, Cx=1, Cy=1, C_use=1, H=16, W=16, transform=0, k=11):
        return L.ssim_scale(x, y, B, Cx, Cy, C_use, H, W, transform, window, k, 1e-4, 9e-4, scratch, ssim, cs, None)
    for rc in (scale(x=None), scale(window=None), scale(ssim=None), scale(cs=None), scale(scratch=None), scale(C_use=2), scale(H=10), scale(W=10), scale(k=4), scale(k=13),
               scale(transform=5), scale(y=p + 1), scale(ssim=p + 4)):
        assert rc == -1
    assert L.avgpool2x2_pair(p, p, 1, 1, 1, 1, 1, 8, 0, p, p, None) == -1 and L.avgpool2x2_pair(p, p, 1, 1, 1, 2, 8, 8, 0, p, p, None) == -1
    assert L.avgpool2x2_pair(p, None, 1, 1, 1, 1, 8, 8, 0, p, p, None) == -1 and L.avgpool2x2_pair(p, p, 1, 1, 1, 1, 8, 8, 9, p, p, None) == -1
    assert L.token_histogram(p, 3, 16, 8, p, p, None) == -1 and L.token_histogram(p, 8, 0, 8, p, p, None) == -1 and L.token_histogram(p, 8, 16, 0, p, p, None) == -1
    assert L.token_histogram(None, 8, 16, 8, p, p, None) == -1 and L.token_histogram(p, 8, 16, 8, p + 4, p, None) == -1
    assert all(v == 0.0 for v in buf)
