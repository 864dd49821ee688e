"""CLIP's vision tower without a GPU: the float64 yardstick of the GPU tests (tests/clip_util.py::vit_forward) is pinned to upstream's class
through tests/golden/clip_vit_micro.npz, the module has upstream's parameter tree and loads its checkpoints strictly, ``build_visual`` reads
the sizes off a state dict, what the HIP path does not do is refused in Python, and the new C symbols are declared, exported and bound."""
import ctypes
import os
import re

import pytest
import torch

from tests import clip_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(case, **over):
    from fourm.utils.clip.model import VisionTransformer
    return VisionTransformer(**{**U.CASES[case], **over})


@pytest.fixture(scope="module")
def gold():
    return U.load_golden()


@pytest.mark.parametrize("case", list(U.CASES))
def test_restatement_reproduces_upstreams_fp32_outputs(case, gold):
    """vit_forward in float32 against upstream's own fp32 run: within 8 x the distance of that run from float64 (two fp32 evaluations of one
    function differ by about that distance; a wrong formula - eps, head split, QuickGELU constant, interpolation - is off by 1e-3 or more)."""
    sd = U.seeded_state_dict(case)
    for run, B, H, W in U.RUNS[case]:
        x = U.images(case, run)
        for flag in U.FLAGS:
            ref = torch.from_numpy(gold[f"{case}/{run}/{flag}/out32"])
            got = U.vit_forward(sd, x, flag, torch.float32)
            assert got.shape == ref.shape and got.dtype == torch.float32
            err, bound = U.rel_max(got, ref), 8 * float(gold[f"{case}/{run}/{flag}/err32"])
            assert err <= bound, (case, run, flag, err, bound)


def test_fixture_shapes_are_the_documented_ones(gold):
    assert gold["clip_a/native/return_all_final_tokens/out32"].shape == (3, 17, 64)
    assert gold["clip_a/interp/return_all_final_tokens/out32"].shape == (2, 65, 64)
    assert gold["clip_b/native/return_all_final_tokens/out32"].shape == (5, 10, 96)
    assert gold["clip_b/interp/return_all_final_tokens/out32"].shape == (2, 13, 96)
    assert gold["clip_b/interp/return_all_tokens/out32"].shape == (2, 12, 192) and gold["clip_a/native/default/out32"].shape == (3, 64)


@pytest.mark.parametrize("case", list(U.CASES))
def test_state_dict_layout_and_strict_load(case, gold):
    model = build(case)
    keys = [str(k) for k in gold[f"{case}/keys"]]
    sd = model.state_dict()
    assert list(sd.keys()) == keys == [k for k, _ in U.expected_shapes(case)]
    assert len(keys) == 8 + 12 * U.CASES[case]["layers"]
    assert [",".join(map(str, sd[k].shape)) for k in keys] == [str(s) for s in gold[f"{case}/shapes"]]
    filled = U.seeded_state_dict(case)
    model.load_state_dict(filled, strict=True)                                 # an upstream-keyed dict into this module ...
    assert all(torch.equal(model.state_dict()[k], filled[k]) for k in keys)
    other = build(case)
    other.load_state_dict(model.state_dict(), strict=True)                     # ... and this module's own dict back
    assert all(torch.equal(other.state_dict()[k], filled[k]) for k in keys)
    assert set(n for n, _ in model.named_parameters()) == set(keys)            # every entry is a parameter, as upstream


def test_initialisation_is_upstreams():
    """class / position embeddings and proj at scale width^-0.5, LayerNorms at (1, 0), in_proj_bias zero, eps 1e-5."""
    torch.manual_seed(0)
    m = build("clip_b")
    w = U.CASES["clip_b"]["width"]
    for p in (m.class_embedding, m.positional_embedding, m.proj):
        assert 0.6 * w ** -0.5 < float(p.detach().std()) < 1.4 * w ** -0.5
    for ln in (m.ln_pre, m.ln_post, m.transformer.resblocks[0].ln_1, m.transformer.resblocks[0].ln_2):
        assert ln.eps == 1e-5 and bool((ln.weight == 1).all()) and bool((ln.bias == 0).all())
    assert bool((m.transformer.resblocks[0].attn.in_proj_bias == 0).all()) and m.conv1.bias is None
    assert m.input_resolution == 48 and m.patch_size == 16 and m.output_dim == 96 and m.width == 192 and m.heads == 3


@pytest.mark.parametrize("prefix", ["visual.", ""])
def test_build_visual_recovers_the_sizes(prefix):
    from fourm.utils.clip.model import build_visual
    for case, cfg in U.CASES.items():
        sd = {prefix + k: v.half() for k, v in U.seeded_state_dict(case).items()}
        if prefix:                                                             # a full CLIP dict carries the text tower too
            sd.update({"text_projection": torch.zeros(8, 8), "transformer.resblocks.0.attn.in_proj_weight": torch.zeros(24, 8), "input_resolution": torch.tensor(1)})
        m = build_visual(sd)
        assert (m.input_resolution, m.patch_size, m.width, m.heads, m.output_dim, len(m.transformer.resblocks)) == \
            (cfg["input_resolution"], cfg["patch_size"], cfg["width"], cfg["heads"], cfg["output_dim"], cfg["layers"])
        assert not m.training and all(p.dtype == torch.float32 and not p.requires_grad for p in m.parameters())
        assert torch.equal(m.proj, sd[prefix + "proj"].float())
    with pytest.raises(NotImplementedError, match="ViT"):
        build_visual({"visual.layer1.0.conv1.weight": torch.zeros(4, 4, 1, 1)})


def test_from_upstream_adopts_a_module_with_upstreams_attributes():
    from fourm.utils.clip.model import VisionTransformer
    src = build("clip_a")
    src.load_state_dict(U.seeded_state_dict("clip_a"))
    got = VisionTransformer.from_upstream(src)
    assert got is not src and not got.training
    assert all(torch.equal(a, b) for a, b in zip(got.state_dict().values(), src.state_dict().values()))


def test_refusals():
    from fourm.utils.clip.model import VisionTransformer
    with pytest.raises(NotImplementedError, match="head_dim"):
        VisionTransformer(32, 8, 128, 1, 4, 64)                                # head_dim 32
    with pytest.raises(NotImplementedError, match="head_dim"):
        VisionTransformer(32, 8, 96, 1, 1, 64)                                 # head_dim 96
    m = build("clip_a")
    assert m.compute_precision == "bf16"
    m.compute_precision = "fp32"
    assert m.compute_precision == "fp32"
    with pytest.raises(ValueError, match="compute_precision"):
        m.compute_precision = "fp16"
    assert m.compute_precision == "fp32"
    x = torch.zeros(2, 3, 32, 32)
    with pytest.raises(NotImplementedError, match="inference only"):           # gradients enabled, trainable parameters
        m(x)
    m.requires_grad_(False)
    with pytest.raises(ValueError, match="divisible"):
        m(torch.zeros(2, 3, 36, 32))
    with pytest.raises(ValueError, match="expected images"):
        m(torch.zeros(2, 1, 32, 32))
    with pytest.raises(RuntimeError, match="GPU"):                             # a CPU model says where it computes: no torch fall-back
        m(x)
    with torch.no_grad(), pytest.raises(RuntimeError, match="GPU"):
        build("clip_a")(x)


def test_position_table_follows_upstreams_interpolation(gold):
    """The host-side table the device kernel adds: the parameter itself whenever the token count matches, else the bicubic resize."""
    m = build("clip_b").requires_grad_(False)
    m.load_state_dict(U.seeded_state_dict("clip_b"))
    pe = m.positional_embedding.detach()
    assert torch.equal(m._pos_table(3, 3, pe.device), pe)
    assert torch.equal(m._pos_table(9, 1, pe.device), pe)                       # 9 patches in another arrangement: upstream adds the native table
    t = m._pos_table(4, 3, pe.device)
    assert t.shape == (13, 192) and torch.equal(t, U.position_table(pe, 4, 3)) and torch.equal(t[0], pe[0])
    assert m._pos_table(4, 3, pe.device) is t                                    # cached
    assert m.interpolate_pos_encoding(torch.zeros(1, 13, 192), 64, 48).shape == (1, 13, 192)


def test_new_symbols_are_declared_exported_and_bound():
    from fourm.hip import _lib
    header = open(os.path.join(ROOT, "include", "fourm_hip.h")).read()
    args_h = open(os.path.join(ROOT, "ml-4m_amd", "csrc", "gemm_args.h")).read()
    assert re.search(r"#define FM_ABI_VERSION 11\b", header) and _lib.ABI_VERSION == 11 and _lib.lib.fm_abi_version() == 11
    assert re.search(r"FM_EPI_QUICK_GELU = 8\b", header) and "FM_EPI_QUICK_GELU" in args_h and _lib.EPI_QUICK_GELU == 8
    assert (_lib.EPI_BF16, _lib.EPI_GELU, _lib.EPI_RESIDUAL, _lib.EPI_SWIGLU, _lib.EPI_F32, _lib.EPI_TANH, _lib.EPI_SWIGLU_BWD, _lib.EPI_GELU_BWD) == tuple(range(8))
    assert re.search(r"\bint fm_clip_embed_ln\(", header) and "fm_clip_embed_ln" in _lib.EXPORTS
    fn = _lib.lib.fm_clip_embed_ln                                              # resolves: the library exports it
    assert fn is _lib.clip_embed_ln or fn.argtypes == _lib.clip_embed_ln.argtypes
    assert len(fn.argtypes) == 14 and fn.restype is ctypes.c_int and fn.argtypes[12] is ctypes.c_float
    assert "clip.hip" in open(os.path.join(ROOT, "ml-4m_amd", "build_ext.py")).read()


def test_package_layout():
    import fourm
    from fourm.utils import clip
    from fourm.utils.clip import model
    assert os.path.dirname(os.path.abspath(model.__file__)) == os.path.join(os.path.dirname(os.path.abspath(fourm.__file__)), "utils", "clip")
    assert clip.VisionTransformer is model.VisionTransformer and clip.build_visual is model.build_visual
    assert callable(getattr(model.VisionTransformer, "from_upstream"))
