"""The CLIP perceptual loss without a GPU: the float64 yardstick of the GPU tests (tests/clip_percept_util.py) is pinned to the pinned
restatement of the tower, ``percept_transform`` is upstream's two Normalize steps, the constructor parses and refuses what it documents, and the
new C symbols are declared, exported and bound."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from tests import clip_percept_util as PU
from tests import clip_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["fm_feat_distance", "fm_quick_gelu_bwd", "fm_quick_gelu_bwd_f32", "fm_clip_embed_ln_bwd", "fm_tap_add"]


def tower(case="clip_a", **over):
    from fourm.utils.clip.model import VisionTransformer
    return VisionTransformer(**{**U.CASES[case], **over})


@pytest.mark.parametrize("case", list(U.CASES))
def test_vit_taps_is_the_pinned_restatement(case):
    """The stream after the last block, finished with ln_post and proj, is bit for bit vit_forward's 'return_all_final_tokens' in float64; the
    earlier taps are the same loop stopped earlier (the stream after block i does not depend on the blocks behind it)."""
    sd = U.seeded_state_dict(case)
    x = U.images(case, "native")
    layers = U.CASES[case]["layers"]
    taps = PU.vit_taps(sd, x, list(range(layers)), torch.float64)
    D = U.CASES[case]["width"]
    last = taps[layers - 1]
    done = F.layer_norm(last, (D,), sd["ln_post.weight"].double(), sd["ln_post.bias"].double(), U.LN_EPS) @ sd["proj"].double()
    assert torch.equal(done, U.vit_forward(sd, x, "return_all_final_tokens", torch.float64))
    assert last.shape == (x.shape[0], (x.shape[2] // U.CASES[case]["patch_size"]) ** 2 + 1, D)
    for i in range(layers - 1):
        assert torch.equal(PU.vit_taps(sd, x, [i], torch.float64)[i], taps[i]) and not torch.equal(taps[i], last)


def test_percept_ref_is_upstreams_arithmetic():
    """lines 89-109 on hand-made features: the per-tap terms, their sum, the division by the batch size."""
    g = torch.Generator().manual_seed(3)
    fp, ft = torch.randn(2, 5, 8, generator=g, dtype=torch.float64), torch.randn(2, 5, 8, generator=g, dtype=torch.float64)
    cos = (fp * ft).sum(-1) / (fp.norm(dim=-1) * ft.norm(dim=-1))
    assert torch.allclose(PU.feature_loss(fp, ft, "cosine"), 1 - cos.mean(-1), rtol=1e-14, atol=0)
    l1 = (fp / fp.norm(dim=-1, keepdim=True) - ft / ft.norm(dim=-1, keepdim=True)).abs().sum(-1).mean(-1)
    assert torch.allclose(PU.feature_loss(fp, ft, "mae"), l1, rtol=1e-14, atol=0)
    sd, x = U.seeded_state_dict("clip_a"), U.images("clip_a", "native")
    y = x + 0.3 * torch.randn(x.shape, generator=g)
    a, b = PU.vit_taps(sd, y, [0, 1]), PU.vit_taps(sd, x, [0, 1])
    want = (PU.feature_loss(a[0], b[0], "cos") + PU.feature_loss(a[1], b[1], "cos")) / 3
    assert torch.equal(PU.percept_ref(sd, y, x, [0, 1], "cos"), want) and want.shape == (3,)


def test_percept_transform_is_the_two_normalize_steps():
    from fourm.vq.percept_losses import OPENAI_CLIP_MEAN, OPENAI_CLIP_STD, ClipPerceptualLoss
    loss = ClipPerceptualLoss(tower(), "blocks.1")
    x = (torch.rand(2, 3, 32, 32, generator=torch.Generator().manual_seed(1), dtype=torch.float64) * 2 - 1)

    def normalize(t, mean, std):                                        # torchvision.transforms.Normalize
        return (t - torch.tensor(mean, dtype=t.dtype).view(1, 3, 1, 1)) / torch.tensor(std, dtype=t.dtype).view(1, 3, 1, 1)

    want = normalize(normalize(x, (-1.0, -1.0, -1.0), (2.0, 2.0, 2.0)), OPENAI_CLIP_MEAN, OPENAI_CLIP_STD)
    got = loss.percept_transform(x.float())
    assert got.dtype == torch.float32 and got.shape == x.shape
    # one fp32 rounding of an affine whose two coefficients are fp32 roundings: 3 x 2^-24 of the magnitudes involved (|x| <= 1, |shift| < 2)
    assert float((got.double() - want).abs().max()) <= 3 * 2.0 ** -24 * float(want.abs().max() + 2)
    other = ClipPerceptualLoss(tower(), "blocks.0", mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5))         # v -> 2 v - 1 undoes the first step
    assert torch.equal(other.percept_transform(x.float()), x.float())
    xr = x.float().requires_grad_()
    loss.percept_transform(xr).sum().backward()                         # differentiable: d / dx = 0.5 / std per channel
    assert torch.allclose(xr.grad[:, 1], torch.full((2, 32, 32), 0.5 / OPENAI_CLIP_STD[1]), rtol=1e-6, atol=0)
    assert callable(loss.percept_transform)


def test_feature_ids_and_feature_loss_parsing():
    from fourm.vq.percept_losses import ClipPerceptualLoss
    vis = tower()
    assert ClipPerceptualLoss(vis, "blocks.0-blocks.1").taps == [0, 1]
    assert ClipPerceptualLoss(vis, ["blocks.1"]).taps == [1] and ClipPerceptualLoss(vis, ["blocks.1"]).feature_ids == ["blocks.1"]
    for bad in ("blocks.2", "blocks.0-blocks.2", "blocks.-1", "block.0", "blocks.0.attn", "norm", "", ["blocks.x"]):
        with pytest.raises(ValueError, match="blocks.<i>"):
            ClipPerceptualLoss(vis, bad)
    with pytest.raises(ValueError, match="blocks.<i>"):                # the default taps of ViT-B/16 do not exist in a 2-block tower
        ClipPerceptualLoss(vis)
    for ok in ("cosine", "cos", "l1", "mae"):
        assert ClipPerceptualLoss(vis, "blocks.0", feature_loss=ok).feature_loss == ok
    with pytest.raises(ValueError, match="Unknown feature loss: mse"):
        ClipPerceptualLoss(vis, "blocks.0", feature_loss="mse")
    with pytest.raises(TypeError, match="VisionTransformer"):
        ClipPerceptualLoss(torch.nn.Linear(2, 2), "blocks.0")


def test_tower_is_frozen_and_stays_in_eval_mode():
    from fourm.vq.percept_losses import ClipPerceptualLoss
    vis = tower().train()
    assert all(p.requires_grad for p in vis.parameters())
    loss = ClipPerceptualLoss(vis, "blocks.0")
    assert loss.visual is vis and not any(p.requires_grad for p in vis.parameters()) and not vis.training
    loss.train()
    assert loss.training and not vis.training
    assert not [k for k in loss.state_dict() if not k.startswith("visual.")]           # the affine is derived, not stored


def test_wrong_size_and_shape_are_refused_before_the_device_is_touched():
    from fourm.vq.percept_losses import ClipPerceptualLoss
    loss = ClipPerceptualLoss(tower(), "blocks.0")
    x = torch.zeros(2, 3, 64, 64)
    with pytest.raises(NotImplementedError, match="resize"):
        loss(x, x)
    with pytest.raises(NotImplementedError, match="resize"):
        loss.percept_transform(x)
    with pytest.raises(ValueError, match="differ in shape"):
        loss(torch.zeros(2, 3, 32, 32), torch.zeros(3, 3, 32, 32))
    with pytest.raises(ValueError, match=r"\(B, 3, H, W\)"):
        loss(torch.zeros(2, 1, 32, 32), torch.zeros(2, 1, 32, 32))
    with pytest.raises(RuntimeError, match="MI355X"):                   # the right size on the host: there is no CPU path
        loss(torch.zeros(2, 3, 32, 32), torch.zeros(2, 3, 32, 32))


def test_trainable_tower_is_refused_by_the_differentiable_path():
    vis = tower()
    with pytest.raises(NotImplementedError, match="frozen"):
        vis.features(torch.zeros(1, 3, 32, 32), [0], True)
    vis.requires_grad_(False)
    with pytest.raises(ValueError, match="taps"):
        vis.features(torch.zeros(1, 3, 32, 32), [2], True)
    with pytest.raises(RuntimeError, match="most recent training forward"):
        vis.features_backward(None, {})


def test_new_symbols_are_declared_exported_and_bound():
    from fourm.hip import _lib
    header = open(os.path.join(ROOT, "include", "fourm_hip.h")).read()
    assert re.search(r"#define FM_ABI_VERSION 11\b", header) and _lib.ABI_VERSION == 11 and _lib.lib.fm_abi_version() == 11        # purely additive
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.EXPORTS and hasattr(_lib.lib, name), name
        fn = getattr(_lib.lib, name)
        assert fn.argtypes is not None and fn.restype is ctypes.c_int and fn.argtypes[-1] is ctypes.c_void_p, name
    assert [len(getattr(_lib.lib, n).argtypes) for n in NEW] == [12, 10, 9, 14, 11]
    assert len(_lib.quick_gelu_bwd.argtypes) == len(_lib.gelu_bwd.argtypes) and len(_lib.quick_gelu_bwd_f32.argtypes) == len(_lib.gelu_bwd_f32.argtypes)
    assert _lib.clip_embed_ln_bwd.argtypes[12] is ctypes.c_float
    assert re.search(r"FM_FEAT_COSINE = 0, FM_FEAT_L1 = 1\b", header) and (_lib.FEAT_COSINE, _lib.FEAT_L1) == (0, 1)


def test_package_imports_without_an_upstream_checkout():
    """A fresh interpreter with no checkout named or on the path: the package and its class import, and upstream-only siblings are reported
    as missing by name instead of breaking the import."""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from fourm import _upstream\n"
            "assert _upstream.upstream_root() is None, _upstream.upstream_root()\n"
            "import torch, fourm.vq.percept_losses as P\n"
            "assert P.ClipPerceptualLoss.__module__ == 'fourm.vq.percept_losses.clip_loss' and P.__all__[0] == 'ClipPerceptualLoss'\n"
            "try:\n    import fourm.vq.percept_losses.lpips\nexcept ImportError as e:\n    print('missing:', e.name)\n") % os.path.join(ROOT, "ml-4m_amd")
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    env.pop("FOURM_UPSTREAM", None)
    run = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr
    assert "missing: fourm.vq.percept_losses.lpips" in run.stdout
