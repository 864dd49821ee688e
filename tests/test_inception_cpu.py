"""fourm.utils.inception without a GPU: the parameter table, the host side of prepare() (BatchNorm folding, weight packing), the refusals, and
the reference restatement's own geometry and fixture condition (tests/inception_util.py)."""
import os
import re

import numpy as np
import pytest
import torch

from tests import inception_util as IU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model():
    from fourm.utils.inception import FidInceptionV3
    return FidInceptionV3()


def test_state_dict_names_and_shapes_follow_the_table():
    want = IU.state_dict_shapes()
    got = {k: tuple(v.shape) for k, v in _model().state_dict().items()}
    assert set(got) == set(want), set(got) ^ set(want)
    assert got == dict(want)
    assert len(IU.unit_table()) == 94 and len(want) == 94 * 5 + 2


def test_unit_table_matches_the_restatement():
    from fourm.utils.inception import BN_EPS, UNITS
    assert BN_EPS == IU.BN_EPS == 1e-3
    assert list(UNITS) == list(IU.unit_table())
    for name, (cin, cout, kh, kw, s, ph, pw) in IU.unit_table().items():
        assert UNITS[name] == (cin, cout, (kh, kw), s, (ph, pw)), name


def test_load_round_trip_is_strict_but_tolerates_torchvision_extras():
    sd = IU.seeded_state_dict(3)
    extra = dict(sd)
    extra["Conv2d_1a_3x3.bn.num_batches_tracked"] = torch.tensor(5)
    extra["Mixed_7c.branch_pool.bn.num_batches_tracked"] = torch.tensor(5)
    extra["AuxLogits.conv0.conv.weight"] = torch.zeros(128, 768, 1, 1)
    extra["AuxLogits.fc.bias"] = torch.zeros(1008)
    m = _model()
    m.load_state_dict(extra)
    back = m.state_dict()
    assert set(back) == set(sd)
    for k, v in sd.items():
        assert torch.equal(back[k], v), k
    missing = dict(sd)
    del missing["Mixed_6c.branch7x7dbl_3.bn.running_var"]
    with pytest.raises(RuntimeError, match="running_var"):
        _model().load_state_dict(missing)
    unexpected = dict(sd)
    unexpected["Mixed_6c.branch7x7dbl_3.conv.bias"] = torch.zeros(160)
    with pytest.raises(RuntimeError, match="conv.bias"):
        _model().load_state_dict(unexpected)


def test_bn_folding_matches_float64_batch_norm():
    from fourm.utils.inception.model import fold_bn
    g = IU.gen(5)
    w = torch.randn(6, 4, 1, 7, generator=g)
    gamma, beta = 1.0 + 0.3 * torch.randn(6, generator=g), torch.randn(6, generator=g)
    mean, var = torch.randn(6, generator=g), 0.5 + torch.rand(6, generator=g)
    x = torch.randn(2, 4, 5, 9, generator=g).double()
    wf, bf = fold_bn(w, gamma, beta, mean, var)
    assert wf.dtype == bf.dtype == torch.float64
    got = torch.nn.functional.conv2d(x, wf, bf, padding=(0, 3))
    ref = torch.nn.functional.batch_norm(torch.nn.functional.conv2d(x, w.double(), None, padding=(0, 3)), mean.double(), var.double(), gamma.double(),
                                         beta.double(), False, 0.0, 1e-3)
    assert float((got - ref).abs().max()) <= 1e-13 * float(ref.abs().max())


def test_weight_packing_is_tap_major_channel_minor():
    from fourm.utils.inception.model import pack_weight
    cout, cin, kh, kw = 3, 5, 2, 7
    w = torch.arange(cout * cin * kh * kw, dtype=torch.float32).reshape(cout, cin, kh, kw)
    p = pack_weight(w)
    assert tuple(p.shape) == (cout, kh * kw * cin) and p.is_contiguous()
    for n in range(cout):
        for ky in range(kh):
            for kx in range(kw):
                for c in range(cin):
                    assert p[n, (ky * kw + kx) * cin + c] == w[n, c, ky, kx]


def test_refusals_without_a_gpu():
    from fourm.utils.inception import FrechetInceptionDistance, InceptionScore, fid_from_moments
    m = _model()
    imgs = torch.zeros(1, 3, 8, 8, dtype=torch.uint8)
    with pytest.raises(NotImplementedError, match="inference only"):
        m(imgs)                                                        # trainable parameters with gradients enabled
    m.requires_grad_(False)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(imgs)
    with torch.no_grad():
        with pytest.raises(TypeError):
            m(imgs.float())                                            # fp32 needs normalize=True
        with pytest.raises(TypeError):
            m(imgs, normalize=True)
        with pytest.raises(RuntimeError, match="no CPU path"):
            m.features(torch.zeros(299 * 299, 3))
    for f in (64, 192, 768):
        with pytest.raises(ValueError, match="not built"):
            FrechetInceptionDistance(feature=f)
    with pytest.raises(TypeError):
        FrechetInceptionDistance(no_such_keyword=1)
    fid = FrechetInceptionDistance(feature=2048, reset_real_features=True, normalize=False, sync_on_compute=True, compute_on_cpu=False)
    with pytest.raises(RuntimeError, match="no CPU path"):
        fid.update_features(torch.zeros(4, 16), real=True)
    with pytest.raises(TypeError):
        fid.update_features(torch.zeros(4, 16, dtype=torch.float64), real=True)
    with pytest.raises(RuntimeError, match="tower"):
        fid.update(imgs, real=True)
    with pytest.raises(RuntimeError, match="at least 2 samples"):
        fid.compute()
    s, o = torch.zeros(3, dtype=torch.float64), torch.zeros(3, 3, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="at least 2 samples"):
        fid_from_moments(s, o, 5, s, o, 1)
    with pytest.raises(RuntimeError, match="at least 2 samples"):
        fid_from_moments(s, o, 1, s, o, 5)
    isc = InceptionScore(feature="logits_unbiased", splits=10, normalize=False, sync_on_compute=True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        isc.update_features(torch.zeros(4, 1008))
    with pytest.raises(TypeError):
        isc.update_features(torch.zeros(4, 1008, dtype=torch.float16))
    with pytest.raises(ValueError, match="not built"):
        InceptionScore(feature=2048)
    with pytest.raises(RuntimeError):
        isc.compute()


def test_fid_from_moments_agrees_with_the_second_float64_route():
    """The host part of compute() against the restatement's two routes, on CPU tensors (no kernel involved)."""
    from fourm.utils.inception import fid_from_moments
    g = IU.gen(21)
    a = (torch.randn(200, 16, generator=g) * torch.linspace(0.5, 2.0, 16)).float()
    b = (0.3 + 1.2 * torch.randn(150, 16, generator=g)).float()
    m1, m2 = IU.moments(a), IU.moments(b)
    tol, spread = IU.fid_tol(m1, m2)
    got = float(fid_from_moments(torch.from_numpy(m1[0]), torch.from_numpy(m1[1]), m1[2], torch.from_numpy(m2[0]), torch.from_numpy(m2[1]), m2[2]))
    assert abs(got - IU.fid_eigh(m1, m2)) <= tol, (got, IU.fid_eigh(m1, m2), tol, spread)
    assert got > 0.1


def test_restatement_geometry_and_fixture_condition():
    fx = IU.fixture()
    sizes = []
    for _, _, h, w in fx["trace"]:
        assert h == w
        if not sizes or sizes[-1] != h:
            sizes.append(h)
    assert tuple(sizes) == IU.GEOMETRY == (299, 149, 147, 73, 71, 35, 17, 8)
    widths = {name: c for name, c, _, _ in fx["trace"]}
    assert tuple(widths[b] for b in ("Mixed_5b", "Mixed_5c", "Mixed_5d", "Mixed_6a", "Mixed_7a", "Mixed_7c")) == IU.WIDTHS == (256, 288, 288, 768, 1280, 2048)
    assert all(widths[b] == 768 for b in ("Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e")) and widths["Mixed_7b"] == 2048
    pool = fx["ref64"]["pool"]
    assert tuple(pool.shape) == (2, 2048) and tuple(fx["ref64"]["logits_unbiased"].shape) == (2, 1008)
    # a dead or exploding tower would let every comparison pass vacuously
    for b in range(pool.shape[0]):
        assert int((pool[b] != 0).sum()) >= 1024, int((pool[b] != 0).sum())
        assert 1e-2 <= float(pool[b].max()) <= 1e3, float(pool[b].max())
    assert not torch.equal(pool[0], pool[1])
    assert torch.equal(fx["ref64"]["logits"], fx["ref64"]["logits_unbiased"] + fx["sd"]["fc.bias"].double())


def test_resize_tables_of_the_package_match_the_restatement():
    from fourm.utils.inception import ops
    for n in (1, 48, 64, 299, 300, 448):
        i0, i1, w = ops.resize_axis(n)
        r0, r1, rw = IU.axis_table(n)
        assert np.array_equal(i0, r0.numpy()) and np.array_equal(i1, r1.numpy()) and np.array_equal(w.astype(np.float64), rw.numpy())
        assert i0.dtype == i1.dtype == np.int32 and w.dtype == np.float32 and i1.max() <= n - 1
    i0, _, w = ops.resize_axis(299)
    assert np.array_equal(i0, np.arange(299)) and not w.any()


def test_new_entry_points_are_declared_and_bound():
    import ctypes
    from fourm.hip import _lib
    header = open(os.path.join(ROOT, "include", "fourm_hip.h")).read()
    assert re.search(r"#define FM_ABI_VERSION 11\b", header) and _lib.ABI_VERSION == 11
    for sym in ("fm_conv2d_nhwc_f32", "fm_pool2d_nhwc_f32", "fm_inception_preprocess", "fm_feature_moments"):
        assert re.search(r"\bint %s\(" % sym, header) and sym in _lib.EXPORTS and hasattr(_lib.lib, sym)
    for name, val in dict(FM_CONV2D_MAX_K=_lib.CONV2D_MAX_K, FM_CONV2D_MAX_PAD=_lib.CONV2D_MAX_PAD, FM_INCEPTION_SIZE=_lib.INCEPTION_SIZE,
                          FM_MOMENTS_MAX_D=_lib.MOMENTS_MAX_D, FM_POOL_MAX_3X3_S2=_lib.POOL_MAX_3X3_S2, FM_POOL_MAX_3X3_S1P1=_lib.POOL_MAX_3X3_S1P1,
                          FM_POOL_AVG_3X3_S1P1=_lib.POOL_AVG_3X3_S1P1, FM_POOL_GLOBAL_AVG=_lib.POOL_GLOBAL_AVG).items():
        assert re.search(rf"#define {name} {val}\b", header), name
    assert ctypes.sizeof(_lib.Conv2dArgs) == 4 * 8 + 14 * 4
    # refusals of the C side need no GPU: nothing is launched
    a = _lib.Conv2dArgs()
    assert _lib.conv2d_nhwc_f32(ctypes.byref(a), None) == -1 and b"null pointer" in _lib.lib.fm_last_error()
    assert _lib.pool2d_nhwc_f32(None, 1, None, 1, 1, 3, 3, 1, 0, None) == -1
    assert _lib.feature_moments(None, 1, 1, 1, None, None, None, None) == -1
    assert _lib.inception_preprocess(None, 0, 1, 8, 8, None, None, None, None) == -1
