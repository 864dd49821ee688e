"""LpipsPerceptualLoss without a GPU: the restatement the GPU tests compare against is pinned to upstream's own forward (the fixture
tests/golden/lpips_small.npz, written by tests/golden/make_golden_lpips.py), and the module's surface - names, shapes, frozen state, refusals,
the dgrad weight image, the C ABI additions - is checked."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from tests import lpips_util as LU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["fm_lpips_stem", "fm_lpips_stem_bwd", "fm_maxpool2x2_nhwc", "fm_lpips_distance", "fm_lpips_tap_bwd"]


@pytest.fixture(scope="module")
def golden():
    return LU.load_golden()


def make(**kw):
    from fourm.vq.percept_losses import LpipsPerceptualLoss
    return LpipsPerceptualLoss(LU.seeded_state_dict(), **kw)


@pytest.mark.parametrize("case", sorted(LU.CASES))
def test_restatement_reproduces_upstreams_forward_in_float64(case, golden):
    loss, grad = LU.ref_run(case, torch.float64)
    assert loss.shape == (LU.CASES[case][0], 1, 1, 1)
    for name, got in (("loss", loss), ("grad", grad)):
        ref = torch.from_numpy(golden[f"{case}/{name}"])
        assert got.shape == ref.shape and LU.rel_max(got, ref) <= 1e-12, (case, name, LU.rel_max(got, ref))


def test_state_dict_keys_and_shapes_are_upstreams(golden):
    sd = make().state_dict()
    keys = [str(k) for k in golden["keys"]]
    assert list(sd) == keys
    for k in keys:
        assert tuple(sd[k].shape) == tuple(int(v) for v in golden["shape/" + k]), k
    assert len(keys) == 2 + 26 + 5


def test_load_state_dict_round_trips_strictly():
    from fourm.vq.percept_losses import LpipsPerceptualLoss
    a = make()
    b = LpipsPerceptualLoss()
    assert not torch.equal(a.state_dict()["net.slice3.12.weight"], b.state_dict()["net.slice3.12.weight"])       # seeded-random without a state dict
    assert torch.equal(b.state_dict()["lin2.model.1.weight"], LpipsPerceptualLoss().state_dict()["lin2.model.1.weight"])
    res = b.load_state_dict(a.state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for k, v in a.state_dict().items():
        assert torch.equal(v, b.state_dict()[k]), k
    for k, v in LU.seeded_state_dict().items():
        assert torch.equal(v, a.state_dict()[k]), k
    assert all(not p.requires_grad for p in b.parameters())
    # as upstream's load_from_pretrained: strict=False with a partial dict
    part = {k: v for k, v in a.state_dict().items() if k.startswith("lin")}
    assert not b.load_state_dict(part, strict=False).unexpected_keys


def test_everything_is_frozen_and_train_keeps_eval():
    m = make()
    assert list(m.parameters()) and all(not p.requires_grad for p in m.parameters())
    assert not m.training
    assert m.train() is m and not m.training and not any(c.training for c in m.modules())
    m.train(True)
    assert not m.training
    m.eval()
    assert not m.training
    assert m.compute_precision == "bf16" and make(compute_precision="fp32").compute_precision == "fp32"
    with pytest.raises(ValueError):
        make(compute_precision="fp16")


def test_percept_transform_is_the_identity():
    m = make()
    x = torch.randn(2, 3, 16, 16)
    assert m.percept_transform(x) is x


def test_refusals():
    m = make()
    x = torch.zeros(2, 3, 32, 32)
    with pytest.raises(NotImplementedError, match="multiples of 16"):
        m(torch.zeros(2, 3, 40, 32), torch.zeros(2, 3, 40, 32))
    with pytest.raises(NotImplementedError, match="multiples of 16"):
        m(torch.zeros(2, 3, 32, 24), torch.zeros(2, 3, 32, 24))
    with pytest.raises(ValueError):
        m(torch.zeros(2, 4, 32, 32), torch.zeros(2, 4, 32, 32))
    with pytest.raises(ValueError):
        m(x, torch.zeros(2, 3, 32, 48))
    with pytest.raises(ValueError):
        m(x, torch.zeros(3, 3, 32, 32))
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(x, x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(x.clone().requires_grad_(), x)


def test_dgrad_weight_image_is_the_input_gradient_of_the_convolution():
    from fourm.vq.percept_losses.lpips_loss import dgrad_weight_image
    g = torch.Generator().manual_seed(3)
    cin, cout = 64, 128
    w = torch.randn(cout, cin, 3, 3, generator=g, dtype=torch.float64)
    x = torch.randn(2, cin, 5, 7, generator=g, dtype=torch.float64).requires_grad_()
    dy = torch.randn(2, cout, 5, 7, generator=g, dtype=torch.float64)
    ref, = torch.autograd.grad(F.conv2d(x, w, padding=1), x, dy)
    wd = dgrad_weight_image(w)
    assert wd.shape == (cin, 9 * cout)
    assert wd[5, 7 * cout + 11] == w[11, 5, 2 - 7 // 3, 2 - 7 % 3]
    got = F.conv2d(dy, wd.reshape(cin, 3, 3, cout).permute(0, 3, 1, 2), padding=1)
    assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())


def test_new_symbols_are_declared_exported_and_bound():
    from fourm.hip import _lib
    header = open(os.path.join(ROOT, "include", "fourm_hip.h")).read()
    args_h = open(os.path.join(ROOT, "ml-4m_amd", "csrc", "gemm_args.h")).read()
    assert re.search(r"#define FM_ABI_VERSION 11\b", header) and _lib.ABI_VERSION == 11 and _lib.lib.fm_abi_version() == 11
    assert re.search(r"FM_EPI_RELU = 9\b", header) and re.search(r"FM_EPI_RELU_BWD = 10\b", header) and re.search(r"FM_EPI_QUICK_GELU = 8\b", header)
    assert "FM_EPI_RELU" in args_h and "FM_EPI_RELU_BWD" in args_h
    assert (_lib.EPI_RELU, _lib.EPI_RELU_BWD, _lib.EPI_QUICK_GELU) == (9, 10, 8)
    assert re.search(r"#define FM_LPIPS_CHUNK %d\b" % _lib.LPIPS_CHUNK, header)
    n_args = dict(fm_lpips_stem=12, fm_lpips_stem_bwd=11, fm_maxpool2x2_nhwc=10, fm_lpips_distance=14, fm_lpips_tap_bwd=16)
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib.EXPORTS and hasattr(_lib.lib, name), name
        fn = getattr(_lib.lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == n_args[name] and fn.argtypes[-1] is ctypes.c_void_p, name      # the stream comes last
    assert "lpips.hip" in open(os.path.join(ROOT, "ml-4m_amd", "build_ext.py")).read()


def test_package_exports_and_the_upstream_fallthrough_stay():
    """A fresh interpreter without an upstream checkout: the class imports, __all__ still starts with the CLIP loss, and upstream's own
    ``lpips`` module is still reported missing by name (no file of that name shadows it)."""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from fourm import _upstream\n"
            "assert _upstream.upstream_root() is None, _upstream.upstream_root()\n"
            "from fourm.vq.percept_losses import LpipsPerceptualLoss\n"
            "import fourm.vq.percept_losses as P\n"
            "assert LpipsPerceptualLoss.__module__ == 'fourm.vq.percept_losses.lpips_loss'\n"
            "assert P.__all__[0] == 'ClipPerceptualLoss' and P.__all__[-1] == 'LpipsPerceptualLoss'\n"
            "try:\n    import fourm.vq.percept_losses.lpips\nexcept ImportError as e:\n    print('missing:', e.name)\n") % os.path.join(ROOT, "ml-4m_amd")
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    env.pop("FOURM_UPSTREAM", None)
    run = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr
    assert "missing: fourm.vq.percept_losses.lpips" in run.stdout
