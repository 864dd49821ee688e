"""The DINOv2 tower without a GPU: state-dict contract, position tables, refusals, ABI additions and the feature tasks' refusals.
(The `facebookresearch/dinov2` package is not available here: the definition in INTEGRATION.md is the contract, parity with the package is
unpinned.)"""
import os
import re

import pytest
import torch
import torch.nn.functional as F

from tests import dinov2_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HUB = {      # constructor -> (width, heads, depth, ffn)
    "vit_small": (384, 6, 12, "mlp"), "vit_base": (768, 12, 12, "mlp"), "vit_large": (1024, 16, 24, "mlp"), "vit_giant2": (1536, 24, 40, "swiglufused"),
}


def _cfg(name, reg4=False, depth=None):
    D, H, L, ffn = HUB[name]
    return dict(img_size=518, patch_size=14, embed_dim=D, depth=depth or L, num_heads=H, ffn_layer=ffn, num_register_tokens=4 if reg4 else 0,
                interpolate_antialias=reg4, interpolate_offset=0.0 if reg4 else 0.1)


@pytest.mark.parametrize("reg4", [False, True], ids=["plain", "reg4"])
@pytest.mark.parametrize("name", sorted(HUB))
def test_hub_constructor_state_dict_contract(name, reg4):
    """Key and shape lists of every hub configuration (depth cut to 2 blocks to keep the test small; the full depth is checked by its count)."""
    from fourm.utils import dinov2
    ctor = getattr(dinov2, name + ("_reg4" if reg4 else ""))
    with torch.device("meta"):
        full = ctor()
    D, H, L, ffn = HUB[name]
    assert (full.embed_dim, full.num_heads, full.n_blocks, full.ffn_layer, len(full.blocks)) == (D, H, L, ffn, L)
    assert (full.num_register_tokens, full.interpolate_antialias, full.interpolate_offset) == ((4, True, 0.0) if reg4 else (0, False, 0.1))
    want = U.expected_shapes(_cfg(name, reg4))
    got = {k: tuple(v.shape) for k, v in full.state_dict().items()}
    assert got == dict(want) and len(got) == len(want)
    if ffn == "swiglufused":
        assert got["blocks.0.mlp.w12.weight"] == (2 * 4096, 1536) and got["blocks.0.mlp.w3.weight"] == (1536, 4096)


@pytest.mark.parametrize("case", sorted(U.CASES))
def test_micro_state_dict_strict_and_build_round_trip(case):
    from fourm.utils.dinov2 import DinoVisionTransformer, build_dinov2
    gold = U.load_golden()
    cfg, sd = U.CASES[case], U.seeded_state_dict(case)
    m = DinoVisionTransformer(**cfg)
    assert sorted(gold[f"{case}/keys"].tolist()) == sorted(m.state_dict())
    for k, s in zip(gold[f"{case}/keys"].tolist(), gold[f"{case}/shapes"].tolist()):
        assert tuple(m.state_dict()[k].shape) == tuple(int(v) for v in s.split(","))
    m.load_state_dict(sd, strict=True)
    with pytest.raises(RuntimeError, match="Missing key|Unexpected key"):
        m.load_state_dict({k: v for k, v in sd.items() if k != "blocks.0.ls1.gamma"}, strict=True)
    built = build_dinov2({k: v.half() for k, v in sd.items()})
    for key in ("img_size", "patch_size", "embed_dim", "n_blocks", "num_heads", "ffn_layer", "num_register_tokens", "interpolate_antialias", "interpolate_offset"):
        assert getattr(built, key) == getattr(m, key), key
    assert all(v.dtype == torch.float32 and torch.equal(v, sd[k].half().float()) for k, v in built.state_dict().items())
    assert not built.training and not any(p.requires_grad for p in built.parameters())
    again = build_dinov2(built.state_dict(), interpolate_antialias=True, interpolate_offset=0.25)
    assert again.interpolate_antialias is True and again.interpolate_offset == 0.25
    adopted = DinoVisionTransformer.from_upstream(m)
    assert adopted is not m and all(torch.equal(v, m.state_dict()[k]) for k, v in adopted.state_dict().items())
    with pytest.raises(NotImplementedError, match="not a DINOv2 state dict"):
        build_dinov2({"conv1.weight": torch.zeros(1)})


@pytest.mark.parametrize("case,gh,gw", [("dino_a", 4, 6), ("dino_a", 7, 7), ("dino_a", 5, 5), ("dino_a", 3, 2), ("dino_b", 2, 2), ("dino_b", 4, 5),
                                        ("dino_b", 3, 3), ("dino_b", 1, 4)])
def test_position_table_against_float64_interpolate(case, gh, gw):
    """Both offset modes (dino_a: scale factors with offset 0.1; dino_b: size, antialiased), non-square grids and the native shortcut."""
    from fourm.utils.dinov2 import DinoVisionTransformer, position_table
    cfg = U.CASES[case]
    pe = U.seeded_state_dict(case)["pos_embed"]
    M, D, off, aa = cfg["img_size"] // 14, cfg["embed_dim"], cfg["interpolate_offset"], cfg["interpolate_antialias"]
    got = position_table(pe, gh, gw, aa, off)
    assert got.dtype == torch.float64 and got.shape == (1 + gh * gw, D)
    assert torch.equal(got[0], pe[0, 0].double())                      # the class row is never resampled
    grid = pe[0, 1:].double().reshape(1, M, M, D).permute(0, 3, 1, 2)
    if gh == gw == M:
        assert torch.equal(got, pe[0].double())
        return
    kw = dict(scale_factor=((gh + off) / M, (gw + off) / M)) if off else dict(size=(gh, gw))
    want = F.interpolate(grid, mode="bicubic", antialias=aa, **kw)[0].permute(1, 2, 0).reshape(gh * gw, D)
    assert float((got[1:] - want).abs().max()) <= 1e-12
    if not aa:      # the rule written out: A = -0.75, clamped borders, source coordinate (i + 0.5) M / (g + off) - 0.5
        rule = U.bicubic_rule(grid[0], gh, gw, off).permute(1, 2, 0).reshape(gh * gw, D)
        assert float((got[1:] - rule).abs().max()) <= 1e-12
    m = DinoVisionTransformer(**cfg)
    m.load_state_dict(U.seeded_state_dict(case))
    t = m._pos_table(gh, gw, torch.device("cpu"))
    assert t.dtype == torch.float32 and torch.equal(t, got.float()) and m._pos_table(gh, gw, torch.device("cpu")) is t      # rounded once, cached


def test_refusals():
    from fourm.utils.dinov2 import DinoVisionTransformer
    with pytest.raises(NotImplementedError, match="head_dim 64"):
        DinoVisionTransformer(img_size=70, embed_dim=128, depth=1, num_heads=4)
    with pytest.raises(NotImplementedError, match="ffn_layer"):
        DinoVisionTransformer(img_size=70, embed_dim=128, depth=1, num_heads=2, ffn_layer="swiglu")
    m = DinoVisionTransformer(**U.CASES["dino_a"])
    x = torch.zeros(1, 3, 70, 70)
    with pytest.raises(NotImplementedError, match="inference only"):          # trainable parameters with autograd on
        m(x)
    m.requires_grad_(False)
    with pytest.raises(NotImplementedError, match="masks"):
        m(x, masks=torch.zeros(1, 25, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.get_intermediate_layers(x, n=1)
    with pytest.raises(ValueError, match="divisible by the patch size"):
        m(torch.zeros(1, 3, 64, 70))
    with pytest.raises(ValueError, match="compute_precision"):
        m.compute_precision = "tf32"


def test_abi_additions_are_declared_everywhere():
    from fourm.hip import _lib
    header = open(os.path.join(ROOT, "include", "fourm_hip.h")).read()
    assert "#define FM_ABI_VERSION 11" in header or re.search(r"FM_ABI_VERSION\s+11\b", header)
    assert _lib.ABI_VERSION == 11
    for name, nargs in (("fm_layernorm_fwd_res_ls", 19), ("fm_layerscale_add", 11), ("fm_cls_pos_embed", 13)):
        proto = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, header)
        assert proto is not None and len(proto.group(1).split(",")) == nargs, name
        fn = getattr(_lib.lib, name)
        assert len(fn.argtypes) == nargs and name in _lib.EXPORTS
    import importlib.util
    spec = importlib.util.spec_from_file_location("build_ext_probe", os.path.join(ROOT, "ml-4m_amd", "build_ext.py"))
    be = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(be)
    for src in ("layerscale.hip", "dinov2.hip"):
        assert src in be.SOURCES and os.path.exists(os.path.join(be.CSRC, src))
        assert src not in be.EXTRA_FLAGS          # the unfused LayerScale sum is scoped in the source, the norm behind it compiles as layernorm.hip does
    assert "#pragma clang fp contract(off)" in open(os.path.join(be.CSRC, "layerscale.hip")).read()


def test_feature_tasks_refuse_before_anything_is_loaded(monkeypatch, tmp_path):
    import importlib.util
    spec = importlib.util.spec_from_file_location("save_vq_tokens_probe", os.path.join(ROOT, "ml-4m_amd", "save_vq_tokens.py"))
    S = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(S)
    import fourm.data.crops as crops
    import fourm.data.features as feats
    import fourm.vq as vq

    def boom(*a, **k):
        raise AssertionError("reached past the refusal")
    for mod, name in ((crops, "crop_resize"), (vq, "get_image_tokenizer"), (vq, "tokenize_sub_batches"), (S, "find_samples"), (S, "load_tokenizer"),
                      (feats, "load_feature_extractor"), (feats, "feature_maps")):
        monkeypatch.setattr(mod, name, boom)
    assert feats.FEATURE_TASKS == S.FEATURE_TASKS == ("CLIP-B16", "DINOv2-B14", "DINOv2-B14-global")
    monkeypatch.delenv(feats.CKPT_ENV, raising=False)
    for task in feats.FEATURE_TASKS:
        with pytest.raises(NotImplementedError, match="feature extractor.*FOURM_FEATURE_EXTRACTOR_CKPT"):
            S.main(S.get_args(["--task", task]))
    monkeypatch.setenv(feats.CKPT_ENV, str(tmp_path / "absent.pth"))
    for task in feats.FEATURE_TASKS:
        with pytest.raises(FileNotFoundError, match="FOURM_FEATURE_EXTRACTOR_CKPT"):
            S.main(S.get_args(["--task", task]))
    for task in ("ImageBind-H14", "ImageBind-H14-global", "CLIP-L14", "DINOv2-G14"):          # still refused, variable set or not
        with pytest.raises(NotImplementedError, match="feature extractor"):
            S.main(S.get_args(["--task", task]))
    # a present file passes the check and selects rgb's crops and normalisation
    (tmp_path / "w.pth").write_bytes(b"")
    monkeypatch.setenv(feats.CKPT_ENV, str(tmp_path / "w.pth"))
    cfg = S.task_config(S.get_args(["--task", "DINOv2-B14-global", "--resample_mode", "bilinear"]))
    assert cfg == ("RGB", (0.5, 0.5, 0.5), (0.5, 0.5, 0.5), (), "float32", "bilinear", 0)
    with pytest.raises(NotImplementedError, match="feature extractor tasks"):
        feats.checkpoint_path("rgb")


def test_feature_extractor_loads_from_a_local_state_dict(tmp_path):
    """Both towers from files written here: a full CLIP dict (visual.* keys) and a DINOv2 dict; weights_only loading refuses pickled objects."""
    from tests import clip_util as CU
    from fourm.data.features import load_feature_extractor
    from fourm.utils.clip.model import VisionTransformer
    from fourm.utils.dinov2 import DinoVisionTransformer
    sd = {"visual." + k: v for k, v in CU.seeded_state_dict("clip_a").items()}
    sd["logit_scale"] = torch.zeros(())
    torch.save(sd, tmp_path / "clip.pth")
    v = load_feature_extractor("CLIP-B16", str(tmp_path / "clip.pth"))
    assert isinstance(v, VisionTransformer) and v.width == 128 and torch.equal(v.proj, sd["visual.proj"])
    torch.save(U.seeded_state_dict("dino_b"), tmp_path / "dino.pth")
    for task in ("DINOv2-B14", "DINOv2-B14-global"):
        d = load_feature_extractor(task, str(tmp_path / "dino.pth"))
        assert isinstance(d, DinoVisionTransformer) and d.num_register_tokens == 4 and d.ffn_layer == "swiglufused"
    torch.save({"model": DinoVisionTransformer(**U.CASES["dino_a"])}, tmp_path / "pickled.pth")
    with pytest.raises(Exception, match="(?i)weights_only|unsupported|state dict"):
        load_feature_extractor("DINOv2-B14", str(tmp_path / "pickled.pth"))
