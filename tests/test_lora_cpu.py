"""fourm.models.lora_utils without a GPU: the module tree, state-dict layout (against the upstream fixture), initialisation, fusing and
the refusals.  The low-rank kernels themselves are tested in test_lora_kernels_gpu.py, the engine in test_lora_gpu.py."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests.golden.cases import build_case
from tests.lora_util import LORA_CASES, RANK, SCALE, seed_adapters
from tests.util_model import build_hip_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "lora_micro.npz"))


def injected(name, rank=RANK, scale=SCALE):
    from fourm.models import lora_utils as LU
    case = build_case(name)
    model = build_hip_model(case["cfg"], case["share_embedding"], case["norm_bias"], case["learned_pos"])
    model.load_state_dict(case["sd"], strict=True)
    LU.inject_trainable_LoRA(model, rank=rank, scale=scale, target_replace_modules=LU.get_LoRA_module_names("attn"))
    return case, model


def test_module_is_this_packages_own():
    from fourm.models import lora_utils as LU
    assert os.path.abspath(LU.__file__).startswith(os.path.join(ROOT, "ml-4m_amd"))
    for n in ("LoRAWrapper", "get_LoRA_module_names", "inject_trainable_LoRA", "fuse_LoRA_into_linear", "unfreeze_all_LoRA_layers",
              "ATTENTION_MODULES", "SELF_ATTENTION_MODULES", "CROSS_ATTENTION_MODULES", "MLP_MODULES", "TRANSFORMER_MODULES"):
        assert n in vars(LU), n
    assert LU.get_LoRA_module_names("Attn") == LU.ATTENTION_MODULES == {"Attention", "NormAttention", "CrossAttention", "NormCrossAttention"}
    assert LU.get_LoRA_module_names("self_attention") == LU.SELF_ATTENTION_MODULES
    assert LU.get_LoRA_module_names("crossattn") == LU.CROSS_ATTENTION_MODULES
    with pytest.raises(ValueError):
        LU.get_LoRA_module_names("conv")


@pytest.mark.parametrize("name", LORA_CASES)
def test_state_dict_layout_is_upstreams(name):
    """Keys (in order) and shapes equal those of upstream's injected model; a state dict in upstream's names loads strict."""
    case, model = injected(name)
    sd = model.state_dict()
    assert list(sd.keys()) == GOLD[f"{name}/keys"].tolist()
    assert [",".join(map(str, v.shape)) for v in sd.values()] == GOLD[f"{name}/shapes"].tolist()
    gen = torch.Generator().manual_seed(0)
    other = {k: torch.randn(tuple(int(x) for x in s.split(",") if x), generator=gen)
             for k, s in zip(GOLD[f"{name}/keys"].tolist(), GOLD[f"{name}/shapes"].tolist())}
    res = model.load_state_dict(other, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert torch.equal(model.encoder[0].attn.qkv.lora_up.weight, other["encoder.0.attn.qkv.lora_up.weight"])
    assert torch.equal(model.decoder[1].cross_attn.kv.linear.weight, other["decoder.1.cross_attn.kv.linear.weight"])


def test_packed_ranks_and_forwarded_attributes():
    from fourm.models.lora_utils import LoRAWrapper
    _, model = injected("micro_swiglu", rank=3)
    D = model.dim
    blk = model.decoder[0]
    want = {blk.self_attn.qkv: (9, 3 * D), blk.self_attn.proj: (3, D), blk.cross_attn.q: (3, D), blk.cross_attn.kv: (6, 2 * D), blk.cross_attn.proj: (3, D),
            model.encoder[1].attn.qkv: (9, 3 * D), model.encoder[1].attn.proj: (3, D)}
    for w, (width, out_f) in want.items():
        assert isinstance(w, LoRAWrapper)
        assert tuple(w.lora_down.weight.shape) == (width, D) and tuple(w.lora_up.weight.shape) == (out_f, width)
        assert w.lora_down.bias is None and w.lora_up.bias is None
        assert w.weight is w.linear.weight and w.bias is w.linear.bias and (w.in_features, w.out_features) == (D, out_f)
        assert w.rank == 3 and w.scale == SCALE
    # nothing outside the attention modules is wrapped
    for n, m in model.named_modules():
        if isinstance(m, LoRAWrapper):
            assert re.search(r"\.(attn|self_attn|cross_attn)\.(qkv|proj|q|kv)$", n), n
    assert isinstance(model.encoder[0].mlp.fc1, nn.Linear) and isinstance(model.decoder_proj_context, nn.Linear)
    # a second injection finds no plain Linear left below the attention modules
    from fourm.models import lora_utils as LU
    before = [n for n, _ in model.named_parameters()]
    LU.inject_trainable_LoRA(model, rank=3)
    assert [n for n, _ in model.named_parameters()] == before


def test_defaults_and_initialisation_statistics():
    from fourm.models.lora_utils import LoRAWrapper
    torch.manual_seed(0)
    w = LoRAWrapper(nn.Linear(512, 1536), num_packed_linear=3)
    assert w.rank == 4 and w.scale == 1.0 and tuple(w.lora_down.weight.shape) == (12, 512)
    assert float(w.lora_up.weight.abs().max()) == 0.0
    d = w.lora_down.weight.detach()
    n = d.numel()                                              # 6144 samples of N(0, (1 / 4)^2)
    assert abs(float(d.mean())) < 5 * 0.25 / n ** 0.5          # five standard errors of the mean
    assert abs(float(d.std()) - 0.25) < 5 * 0.25 / (2 * n) ** 0.5
    w8 = LoRAWrapper(nn.Linear(512, 512), rank=8)
    assert abs(float(w8.lora_down.weight.std()) - 0.125) < 5 * 0.125 / (2 * 4096) ** 0.5
    with pytest.raises(ValueError):
        LoRAWrapper(nn.Linear(8, 8), rank=4, num_packed_linear=3)


def test_fuse_returns_plain_linears_with_the_low_rank_product():
    from fourm.models import lora_utils as LU
    _, model = injected("micro_qknorm")
    seed_adapters(model)
    with torch.no_grad():
        model.encoder[0].attn.proj.linear.bias = nn.Parameter(torch.randn(model.dim))
    want = {}
    for n, m in model.named_modules():
        if isinstance(m, LU.LoRAWrapper):
            mag = m.linear.weight.double().abs() + SCALE * (m.lora_up.weight.double().abs() @ m.lora_down.weight.double().abs())
            want[n] = (m.linear.weight.double() + SCALE * (m.lora_up.weight.double() @ m.lora_down.weight.double()),
                       None if m.linear.bias is None else m.linear.bias.detach().clone(), mag, m.lora_down.weight.shape[0])
    assert len(want) == 2 * 2 + 2 * 5
    model_base = {n: model.get_submodule(n).linear.weight.detach().double().clone() for n in want}
    LU.fuse_LoRA_into_linear(model)
    assert not any(isinstance(m, LU.LoRAWrapper) for m in model.modules())
    assert not any("lora" in k or ".linear." in k for k in model.state_dict())
    for n, (w64, b, mag, r) in want.items():
        lin = model.get_submodule(n)
        assert type(lin) is nn.Linear
        # fp32 arithmetic in any order: an r-term product chain, the scale, the sum -> |err| <= (r + 3) 2^-24 (|W| + s |up| |down|), entry by entry
        err = (lin.weight.double() - w64).abs()
        assert bool((err <= (r + 3) * 2.0 ** -24 * mag).all()), (n, float((err / mag).max()))
        assert float((lin.weight.double() - model_base[n]).abs().max()) > 1e-3      # (the product is really in there)
        assert (lin.bias is None) == (b is None) and (b is None or torch.equal(lin.bias, b))


def test_unfreeze_touches_adapters_only():
    from fourm.models import lora_utils as LU
    _, model = injected("micro_swiglu")
    for p in model.parameters():
        p.requires_grad = False
    LU.unfreeze_all_LoRA_layers(model)
    for n, p in model.named_parameters():
        assert p.requires_grad == ("lora_" in n), n


def test_refusals_raise_before_any_engine_exists():
    from fourm.models import lora_utils as LU
    case = build_case("micro_swiglu")
    model = build_hip_model(case["cfg"], case["share_embedding"], case["norm_bias"], case["learned_pos"])
    for bad in ("mlp", "all", "transformer", "MLP"):
        with pytest.raises(NotImplementedError, match="SwiGLU"):
            LU.get_LoRA_module_names(bad)
    for target in (LU.MLP_MODULES, LU.TRANSFORMER_MODULES, {"Attention", "GatedMlp"}):
        with pytest.raises(NotImplementedError, match="SwiGLU"):
            LU.inject_trainable_LoRA(model, target_replace_modules=target)
    with pytest.raises(ValueError, match="64"):
        LU.inject_trainable_LoRA(model, rank=22)               # 22 x 3 packed in qkv = 66
    assert not any(isinstance(m, LU.LoRAWrapper) for m in model.modules()) and model._engine is None
    LU.inject_trainable_LoRA(model, rank=21)                   # 63: allowed
    assert model.encoder[0].attn.qkv.lora_down.weight.shape[0] == 63


def test_engine_refuses_wrappers_it_does_not_run():
    from fourm.hip.engine import check_lora_targets
    from fourm.models.lora_utils import LoRAWrapper
    case = build_case("micro_swiglu")
    for where in ("decoder_proj_context", "encoder.0.mlp.fc2", "decoder_embeddings.cap.to_logits"):
        model = build_hip_model(case["cfg"], case["share_embedding"], case["norm_bias"], case["learned_pos"])
        parent, _, leaf = where.rpartition(".")
        holder = model.get_submodule(parent) if parent else model
        holder._modules[leaf] = LoRAWrapper(getattr(holder, leaf), rank=2)
        with pytest.raises(NotImplementedError, match=where.replace(".", r"\.")):
            check_lora_targets(model)
    _, model = injected("micro_swiglu")
    check_lora_targets(model)


def test_inject_and_fuse_drop_the_cached_engine_and_bump_the_epoch():
    from fourm.hip import engine as E
    from fourm.models import lora_utils as LU
    case = build_case("micro_swiglu")
    model = build_hip_model(case["cfg"], case["share_embedding"], case["norm_bias"], case["learned_pos"])
    model._engine = object()
    e0 = E._WEIGHT_EPOCH
    LU.inject_trainable_LoRA(model)
    assert model._engine is None and E._WEIGHT_EPOCH == e0 + 1
    model._engine = object()
    LU.fuse_LoRA_into_linear(model)
    assert model._engine is None and E._WEIGHT_EPOCH == e0 + 2


def test_new_entry_points_are_declared_exported_and_bound():
    from fourm.hip import _lib
    header = open(os.path.join(ROOT, "include", "fourm_hip.h")).read()
    for sym in ("fm_lora_apply", "fm_lora_grad"):
        assert re.search(r"\bint\s+%s\s*\(" % sym, header), sym
        assert sym in _lib.EXPORTS and hasattr(_lib.lib, sym)
    assert _lib.ABI_VERSION == 11 and _lib.lib.fm_abi_version() == 11
    assert len(_lib.lora_apply.argtypes) == 19 and len(_lib.lora_grad.argtypes) == 13
