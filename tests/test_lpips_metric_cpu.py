"""The LPIPS validation metric without a GPU: LpipsAlex's parameter table and loading, the refusals of the metric and of the C side, the new
entry points against the header, and the reference restatement's own properties (tests/lpips_metric_util.py)."""
import ctypes
import os
import re

import pytest
import torch

from tests import lpips_metric_util as MU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _alex(*a, **kw):
    from fourm.vq.percept_losses.lpips_alex import LpipsAlex
    return LpipsAlex(*a, **kw)


def _metric(*a, **kw):
    from fourm.vq.metrics import LearnedPerceptualImagePatchSimilarity
    return LearnedPerceptualImagePatchSimilarity(*a, **kw)


def test_state_dict_names_and_shapes():
    want = MU.state_dict_shapes()
    m = _alex()
    got = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert set(got) == set(want), set(got) ^ set(want)
    assert got == dict(want)
    assert torch.equal(m.scaling_layer.shift.reshape(-1), torch.tensor(MU.SHIFT)) and torch.equal(m.scaling_layer.scale.reshape(-1), torch.tensor(MU.SCALE))
    assert not any(p.requires_grad for p in m.parameters()) and not m.training and not m.train().training
    for s, idx, cin, cout, k, st, p in MU.CONVS:
        conv = getattr(getattr(m.net, f"slice{s}"), str(idx))
        assert (conv.in_channels, conv.out_channels, conv.kernel_size, conv.stride, conv.padding) == (cin, cout, (k, k), (st, st), (p, p))
    # seeded: two instances agree, and the weights are not degenerate
    other = _alex()
    for (k, a), b in zip(m.state_dict().items(), other.state_dict().values()):
        assert torch.equal(a, b), k
    assert float(getattr(m.net.slice1, "0").weight.std()) > 0.01 and float(m.lin2.model.get_submodule("1").weight.min()) >= 0


def test_strict_round_trip_and_from_parts():
    from fourm.vq.percept_losses.lpips_alex import LpipsAlex
    sd = MU.seeded_state_dict()
    m = _alex(sd)
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd[k]), k
    m2 = _alex()
    m2.load_state_dict(m.state_dict(), strict=True)
    missing = dict(sd)
    del missing["lin3.model.1.weight"]
    with pytest.raises(RuntimeError, match="lin3"):
        _alex(missing)
    extra = dict(sd)
    extra["net.slice1.1.weight"] = torch.zeros(1)
    with pytest.raises(RuntimeError, match="slice1.1"):
        _alex(extra)
    feats, lins = MU.parts(sd)
    feats["classifier.1.weight"] = torch.zeros(3, 3)                   # the full torchvision model's extras are ignored
    p = LpipsAlex.from_parts(feats, lins)
    for k, v in p.state_dict().items():
        assert torch.equal(v, sd[k]), k
    bare = {k[len("features."):]: v for k, v in feats.items() if k.startswith("features.")}      # alexnet().features.state_dict()
    p = LpipsAlex.from_parts(bare, lins)
    assert torch.equal(p.state_dict()["net.slice4.8.weight"], sd["net.slice4.8.weight"])
    del bare["6.bias"]
    with pytest.raises(KeyError, match="features.6.bias"):
        LpipsAlex.from_parts(bare, lins)
    with pytest.raises(KeyError, match="lin0"):
        LpipsAlex.from_parts(feats, {})


def test_input_affine_is_folded_in_float64():
    from fourm.vq.percept_losses.lpips_alex import fold_input_affine
    m = _alex()
    x = torch.linspace(-1.0, 1.0, 7, dtype=torch.float64)
    for normalize in (False, True):
        mul, add = fold_input_affine(m.scaling_layer.shift, m.scaling_layer.scale, normalize)
        assert mul.dtype == add.dtype == torch.float64 and tuple(mul.shape) == (3,)
        for c in range(3):
            v = (x + 1) / 2 if normalize else x
            want = ((2 * v - 1 if normalize else v) - float(torch.tensor(MU.SHIFT[c]))) / float(torch.tensor(MU.SCALE[c]))
            assert float((v * mul[c] + add[c] - want).abs().max()) <= 1e-14


def test_metric_refusals():
    for nt in ("vgg", "squeeze"):
        with pytest.raises(ValueError, match="not built"):
            _metric(net_type=nt)
    with pytest.raises(ValueError, match="net_type"):
        _metric(net_type="resnet")
    for red in ("none", "elementwise_mean", None):
        with pytest.raises(ValueError, match="reduction"):
            _metric(reduction=red)
    with pytest.raises(TypeError):
        _metric(no_such_keyword=1)
    with pytest.raises(TypeError, match="LpipsAlex"):
        _metric(net=torch.nn.Identity())
    m = _metric(net_type='alex', reduction='mean', normalize=True, sync_on_compute=True, compute_on_cpu=False)
    ok = torch.zeros(2, 3, 40, 40)
    for bad in (torch.zeros(2, 1, 40, 40), torch.zeros(3, 40, 40), torch.zeros(2, 4, 40, 40)):
        with pytest.raises(ValueError, match=r"\(N, 3, H, W\)"):
            m.update(bad, bad)
    with pytest.raises(ValueError, match="differ in shape"):
        m.update(ok, torch.zeros(2, 3, 40, 41))
    with pytest.raises(ValueError, match="differ in shape"):
        m.update(ok, torch.zeros(1, 3, 40, 40))
    assert torch.isnan(m.compute()) and m.sum_scores is None and m.total is None


def test_no_cpu_path():
    m = _metric()
    x = torch.zeros(1, 3, 32, 32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.update(x, x)
    net = _alex()
    with pytest.raises(RuntimeError, match="no CPU path"):
        net.scores(x, x, False)
    with pytest.raises(RuntimeError, match="no CPU path"):
        net(x, x)
    with pytest.raises(ValueError, match="at least 31"):
        net.scores(torch.zeros(1, 3, 30, 64), torch.zeros(1, 3, 30, 64), False)
    with pytest.raises(TypeError, match="dtype"):
        net.scores(x.double(), x.double(), False)
    from fourm.vq.percept_losses.lpips_alex import conv2d_stem, lpips_score
    with pytest.raises(RuntimeError, match="no CPU path"):
        conv2d_stem(x, torch.zeros(4, 27), None, 3, 3, 1, 1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        lpips_score(torch.zeros(4, 8), torch.zeros(4, 8), torch.zeros(8), 1, 4, torch.zeros(1))


def test_new_entry_points_are_declared_and_bound():
    from fourm.hip import _lib
    header = open(os.path.join(ROOT, "include", "fourm_hip.h")).read()
    assert re.search(r"#define FM_ABI_VERSION 11\b", header) and _lib.ABI_VERSION == 11 and _lib.lib.fm_abi_version() == 11
    for sym in ("fm_conv2d_stem_f32", "fm_lpips_score_scratch", "fm_lpips_score"):
        assert re.search(r"\bint %s\(" % sym, header) and sym in _lib.EXPORTS and hasattr(_lib.lib, sym), sym
    for name, val in dict(FM_STEM_MAX_CIN=_lib.STEM_MAX_CIN, FM_STEM_MAX_COUT=_lib.STEM_MAX_COUT, FM_STEM_MAX_K=_lib.STEM_MAX_K, FM_STEM_MAX_STRIDE=_lib.STEM_MAX_STRIDE,
                          FM_STEM_MAX_PAD=_lib.STEM_MAX_PAD, FM_LPIPS_SCORE_CHUNK=_lib.LPIPS_SCORE_CHUNK, FM_LPIPS_SCORE_MAX_C=_lib.LPIPS_SCORE_MAX_C).items():
        assert re.search(rf"#define {name} {val}\b", header), name
    assert (_lib.STEM_MAX_CIN, _lib.STEM_MAX_COUT, _lib.STEM_MAX_K, _lib.STEM_MAX_STRIDE, _lib.STEM_MAX_PAD, _lib.LPIPS_SCORE_MAX_C) == (4, 128, 11, 4, 5, 512)
    # the prototypes: the parameter list of the header, type by type, against the ctypes argtypes
    kinds = {"const void*": _lib.vp, "void*": _lib.vp, "int": _lib.i32, "float": _lib.f32}
    for sym, fn in (("fm_lpips_score_scratch", _lib.lpips_score_scratch), ("fm_lpips_score", _lib.lpips_score)):
        params = re.search(r"\bint %s\((.*?)\);" % sym, header, re.S).group(1)
        want = [kinds[re.sub(r"\s+", " ", p.strip()).rsplit(" ", 1)[0]] for p in params.split(",")]
        assert list(fn.argtypes) == want, sym
    params = re.search(r"\bint fm_conv2d_stem_f32\((.*?)\);", header, re.S).group(1)
    assert re.sub(r"\s+", " ", params.strip()) == "const fm_conv2d_stem_args* a, void* stream"
    assert _lib.conv2d_stem_f32.argtypes[0]._type_ is _lib.Conv2dStemArgs and _lib.conv2d_stem_f32.argtypes[1] is _lib.vp
    # the struct: field names in header order; 6 pointers, 14 ints, 2 floats with natural alignment
    body = re.search(r"typedef struct fm_conv2d_stem_args \{(.*?)\} fm_conv2d_stem_args;", header, re.S).group(1)
    names = [re.search(r"([A-Za-z_][A-Za-z0-9_]*)\s*$", part.strip()).group(1) for decl in body.split(";") if decl.strip() for part in decl.split(",")]
    assert names == [f[0] for f in _lib.Conv2dStemArgs._fields_]
    assert ctypes.sizeof(_lib.Conv2dStemArgs) == 6 * 8 + 14 * 4 + 2 * 4
    assert _lib.Conv2dStemArgs.lo.offset == 6 * 8 + 14 * 4
    # refusals of the C side need no GPU: nothing is launched
    a = _lib.Conv2dStemArgs()
    assert _lib.conv2d_stem_f32(ctypes.byref(a), None) == -1 and b"null pointer" in _lib.lib.fm_last_error()
    assert _lib.conv2d_stem_f32(None, None) == -1
    assert _lib.lpips_score(None, 4, None, 4, None, 1, 1, 4, 1e-8, None, None, None) == -1
    assert _lib.lpips_score_scratch(3, 225) == 3 * 4 and _lib.lpips_score_scratch(2, 64) == 2 and _lib.lpips_score_scratch(1, 65) == 2
    assert _lib.lpips_score_scratch(0, 5) == -1 and _lib.lpips_score_scratch(5, 0) == -1 and _lib.lpips_score_scratch(1 << 20, 1 << 20) == -1


def test_restatement_is_zero_on_identical_images_and_symmetric():
    fx = MU.fixture(2, 33, 46, False)
    sd = fx["sd"]
    for dtype in (torch.float64, torch.float32):
        same = MU.lpips(sd, fx["img0"], fx["img0"], False, dtype)
        assert same.dtype == dtype and bool((same == 0).all())
        ab, ba = MU.lpips(sd, fx["img0"], fx["img1"], False, dtype), MU.lpips(sd, fx["img1"], fx["img0"], False, dtype)
        assert torch.equal(ab, ba)
    # the fixture is not degenerate: a distance well inside (0, 1), different per sample, the fp32 run close to it
    ref = fx["ref64"]
    assert bool((ref > 1e-3).all()) and bool((ref < 1.0).all()) and float((ref[0] - ref[1]).abs()) > 1e-5
    assert float((fx["ref32"].double() - ref).abs().max()) <= 1e-4 * float(ref.max())
    # geometry: 33 x 46 -> 7 x 10 -> 3 x 4 -> 1 x 1 (x 3)
    shapes = [tuple(t.shape[1:]) for t in MU.taps(sd, fx["img0"], False, torch.float32)]
    assert shapes == [(64, 7, 10), (192, 3, 4), (384, 1, 1), (256, 1, 1), (256, 1, 1)]
    # normalize = True on [0, 1] images is normalize = False on 2 x - 1
    a = MU.lpips(sd, (fx["img0"] + 1) / 2, (fx["img1"] + 1) / 2, True, torch.float64)
    assert float((a - ref).abs().max()) <= 1e-6 * float(ref.max())
    # an all-zero pixel on both sides contributes 0, on one side a finite value
    z, o = torch.zeros(1, 8, 1, 1, dtype=torch.float64), torch.ones(1, 8, 1, 1, dtype=torch.float64)
    w = torch.full((8,), 0.125, dtype=torch.float64)
    assert float(MU.layer_score(z, z, w)) == 0.0 and abs(float(MU.layer_score(z, o, w)) - 0.125) <= 1e-8


def test_reconstruction_metrics_keeps_its_keys_without_lpips():
    from fourm.vq.metrics import ReconstructionMetrics
    r = ReconstructionMetrics('rgb')
    assert r.lpips is None
    assert list(r.compute('[Eval]', 224)) == ['[Eval] MSE@224', '[Eval] MAE@224', '[Eval] PSNR@224', '[Eval] MS-SSIM@224']
    assert list(ReconstructionMetrics('sam_mask').compute()) == ['[Eval] MSE@None', '[Eval] MAE@None', '[Eval] PSNR@None', '[Eval] IoU@None']
    with_lpips = ReconstructionMetrics('normal', lpips=_metric())
    keys = list(with_lpips.compute('[Eval]', 224))
    assert keys == ['[Eval] MSE@224', '[Eval] MAE@224', '[Eval] PSNR@224', '[Eval] MS-SSIM@224', '[Eval] LPIPS@224']
    with pytest.raises(ValueError, match="'rgb' and 'normal'"):
        ReconstructionMetrics('depth', lpips=_metric())
    with pytest.raises(TypeError, match="LearnedPerceptualImagePatchSimilarity"):
        ReconstructionMetrics('rgb', lpips=object())
