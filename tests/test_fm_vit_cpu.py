"""FourMViT without a GPU: the module is this package's own, its parameter tree is upstream's (tests/golden/fm_vit_micro.npz, written by
the unmodified upstream class), checkpoints load, the factories resolve, and everything the HIP path does not implement is refused in
Python before the kernel library is touched."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import fm_vit_util as U

GOLD = os.path.join(os.path.dirname(__file__), "golden", "fm_vit_micro.npz")
FACTORIES = ["fm_vit_tiny_6e_gelu", "fm_vit_small_8e_gelu", "fm_vit_base_12e_gelu", "fm_vit_large_24e_gelu", "fm_vit_xlarge_24e_gelu",
             "fm_vit_tiny_6e_swiglu_nobias", "fm_vit_small_8e_swiglu_nobias", "fm_vit_base_12e_swiglu_nobias", "fm_vit_large_24e_swiglu_nobias",
             "fm_vit_xlarge_24e_swiglu_nobias", "fm_vit_base_12e_swiglu_qknorm_nobias", "fm_vit_large_24e_swiglu_qknorm_nobias",
             "fm_vit_xlarge_24e_swiglu_qknorm_nobias"]


def build(name, **extra):
    from fourm.models import fm_vit
    from fourm.models.fm_utils import LayerNorm
    return fm_vit.FourMViT(**{**U.model_kwargs(name, LayerNorm), **extra})


def test_module_is_this_packages_own_and_has_upstreams_public_names():
    import fourm
    from fourm.models import fm_vit
    assert os.path.dirname(os.path.abspath(fm_vit.__file__)) == os.path.join(os.path.dirname(os.path.abspath(fourm.__file__)), "models")
    for n in ["FourMViT", "FMViT"] + FACTORIES:
        assert n in vars(fm_vit), n
    assert sorted(fm_vit.__all__) == sorted(FACTORIES)
    for n in ("init_weights", "get_num_layers", "get_num_layers_encoder", "no_weight_decay", "freeze_encoder", "unfreeze_encoder", "forward"):
        assert callable(getattr(fm_vit.FourMViT, n)), n


@pytest.mark.parametrize("name", list(U.CASES))
def test_state_dict_layout_and_strict_load(name):
    g = np.load(GOLD)
    model = build(name)
    sd = model.state_dict()
    assert list(sd.keys()) == g[f"{name}/keys"].tolist()
    assert [",".join(map(str, v.shape)) for v in sd.values()] == g[f"{name}/shapes"].tolist()
    assert [k for k, _ in model.named_parameters()] == g[f"{name}/param_keys"].tolist()
    assert sorted(model.no_weight_decay()) == g[f"{name}/no_weight_decay"].tolist()
    assert [model.get_num_layers(), model.get_num_layers_encoder()] == g[f"{name}/num_layers"].tolist()
    seeded = U.seeded_state_dict(model, torch.from_numpy(g["pos_emb"]))
    assert abs(sum(float(v.double().abs().sum()) for v in seeded.values()) - float(g[f"{name}/weight_checksum"])) < 1e-6 * float(g[f"{name}/weight_checksum"])
    res = model.load_state_dict(seeded, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    # this package's sin-cos table is upstream's
    assert float((sd[f"encoder_embeddings.rgb@{U.IMG}.pos_emb"] - torch.from_numpy(g["pos_emb"])).abs().max()) < 1e-6


def test_fourm_checkpoint_loads_non_strict():
    from tests.golden.cases import build_case
    case = build_case("micro_swiglu")
    model = build("swiglu")
    res = model.load_state_dict(case["sd"], strict=False)
    assert res.missing_keys == []          # (output_head is an Identity: nothing of the ViT is left uninitialised)
    own = ("encoder_embeddings.rgb@32.", "encoder.", "encoder_norm.")
    assert sorted(res.unexpected_keys) == sorted(k for k in case["sd"] if not k.startswith(own))
    for k in res.unexpected_keys:
        assert k.startswith(("decoder", "encoder_embeddings.", "mask_token")), k
    assert torch.equal(model.encoder[1].mlp.fc3.weight, case["sd"]["encoder.1.mlp.fc3.weight"])
    with_head = build("swiglu", output_head=nn.Linear(U.DIM, U.CLASSES))
    res = with_head.load_state_dict(case["sd"], strict=False)
    assert sorted(res.missing_keys) == ["output_head.bias", "output_head.weight"]


def test_factories_resolve_through_create_model():
    from fourm.utils import create_model
    from fourm.utils.registry import is_model
    m = create_model("fm_vit_tiny_6e_swiglu_nobias", img_size=32, patch_size=8)
    assert type(m).__name__ == "FourMViT" and m.get_num_layers() == 6 and m.dim == 384 and m.num_patches == 16
    assert m.encoder[0].mlp.fc3.weight.shape[0] == int(2 * 4 * 384 / 3) and m.encoder[0].attn.qkv.bias is None
    m = create_model("fm_vit_tiny_6e_gelu", img_size=32, patch_size=8)
    assert isinstance(m.encoder_norm, nn.LayerNorm) and m.encoder[0].attn.qkv.bias is not None and not hasattr(m.encoder[0].mlp, "fc3")
    assert all(is_model(n) for n in FACTORIES)
    from fourm.utils import list_models
    assert sorted(list_models("fm_vit_*", include_unlisted=True)) == sorted(FACTORIES)


def test_output_head_hook_identity_norm_and_fmvit_config():
    from fourm.models import fm_vit

    class Head(nn.Module):
        def init(self, dim):
            self.fc = nn.Linear(dim, 7)
    m = build("swiglu", output_head=Head(), encoder_norm=False)
    assert isinstance(m.encoder_norm, nn.Identity) and m.output_head.fc.in_features == U.DIM
    assert not any(k.startswith("encoder_norm") for k in m.state_dict())
    assert isinstance(build("swiglu").output_head, nn.Identity)
    cfg = dict(image_size=224, patch_size=16, norm_bias=False, act_layer="SiLU", dim=128, encoder_depth=1, decoder_depth=3, num_heads=2,
               gated_mlp=True, qkv_bias=False, proj_bias=False, mlp_bias=False, domains_in=["rgb@224"], domains_out=[], share_modality_embeddings=True)
    fm = fm_vit.FMViT(cfg)
    assert list(fm.encoder_embeddings) == ["rgb@224"] and fm.num_patches == 196 and len(fm.encoder) == 1
    assert not isinstance(fm.encoder_norm.bias, nn.Parameter)


def test_freeze_and_unfreeze_flags():
    m = build("gelu", output_head=nn.Linear(U.DIM, U.CLASSES))
    emb = [p for p in m.encoder_embeddings.parameters()]
    trunk = list(m.encoder.parameters()) + list(m.encoder_norm.parameters())
    m.freeze_encoder(freeze_embeddings=False)
    assert not any(p.requires_grad for p in trunk) and all(p.requires_grad for p in emb)
    m.freeze_encoder()
    assert not any(p.requires_grad for p in trunk + emb) and all(p.requires_grad for p in m.output_head.parameters())
    m.unfreeze_encoder(unfreeze_embeddings=False)
    assert all(p.requires_grad for p in trunk) and not any(p.requires_grad for p in emb)
    m.unfreeze_encoder()
    assert all(p.requires_grad for p in m.parameters())


def test_refusals_happen_in_python(monkeypatch):
    from fourm.hip import _lib
    from fourm.models import fm_vit

    def boom(*a, **k):
        raise AssertionError("the kernel library was called")
    for fn in ("vit_patch_rows", "vit_emb_rows", "gemm_nt", "layernorm_fwd"):
        monkeypatch.setattr(_lib, fn, boom)
    with pytest.raises(NotImplementedError, match="dropout"):
        build("swiglu", drop_rate=0.1)
    with pytest.raises(NotImplementedError, match="dropout"):
        build("swiglu", attn_drop_rate=0.1)
    with pytest.raises(NotImplementedError, match="head_dim 64"):
        build("swiglu", num_heads=4)
    with pytest.raises(NotImplementedError, match="SiLU|GELU"):
        build("gelu", act_layer=nn.ReLU)
    with pytest.raises(NotImplementedError, match="GELU"):
        build("gelu", act_layer=partial_tanh_gelu())
    with pytest.raises(NotImplementedError, match="SwiGLU"):
        build("swiglu", act_layer=nn.GELU)
    m = build("swiglu")
    for shape in ((2, 3, 40, 32), (2, 3, 32, 24), (2, 3, 64, 64)):
        with pytest.raises(ValueError, match="32 x 32"):
            m(torch.zeros(shape))
    with pytest.raises(RuntimeError, match="GPU"):         # a CPU model says where it computes instead of falling back to torch
        m(torch.zeros(2, 3, 32, 32))
    assert isinstance(fm_vit.FourMViT.engine, property)


def partial_tanh_gelu():
    from functools import partial
    return partial(nn.GELU, approximate="tanh")


def test_vit_patch_rows_is_exported_with_argtypes():
    import ctypes
    from fourm.hip import _lib
    assert "fm_vit_patch_rows" in _lib.EXPORTS and "fm_vit_emb_rows" in _lib.EXPORTS
    fn = _lib.lib.fm_vit_patch_rows
    assert fn is not None and len(fn.argtypes) == 10 and fn.restype is ctypes.c_int
    assert fn.argtypes[0] is ctypes.c_void_p and fn.argtypes[-1] is ctypes.c_void_p and all(t is ctypes.c_int32 for t in fn.argtypes[2:9])
    assert _lib.ABI_VERSION == 11
