"""LoRA fine-tuning on the HIP engine (attention adapters) on a real MI355X: an injected model against the same model with the adapters
fused into plain Linears, against upstream's own LoRA run (tests/golden/lora_micro.npz), and the training plumbing around it (frozen
base, flat gradient store, activation checkpointing, FusedAdamW, eval and K/V-cache generation).

Bounds are the existing ones: fp32 verification mode 2e-6 (loss) / 1e-5 (logits) / 5e-5 (gradient tensors), relative Frobenius, as
tests/test_model_gpu.py::test_fp32_verification_mode; bf16 gradients 4.8e-2 as test_loss_and_gradients; upstream's recorded
fp32-vs-float64 error times 8 as tests/test_memcodes_gpu.py; K/V-cache logits 8e-3."""
import copy
import os
import random

import numpy as np
import pytest
import torch

from tests.golden.cases import build_case
from tests.lora_util import LORA_CASES, RANK, SCALE, freeze_base, lora_names, seed_adapters
from tests.util_model import build_hip_model, to_device

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden", "lora_micro.npz")


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def setup(name, precision="bf16", frozen=True, ckpt=False):
    from fourm.models import lora_utils as LU
    case = build_case(name)
    model = build_hip_model(case["cfg"], case["share_embedding"], case["norm_bias"], case["learned_pos"])
    model.load_state_dict(case["sd"], strict=True)
    model.compute_precision = precision
    model.use_act_checkpoint = ckpt
    LU.inject_trainable_LoRA(model, rank=RANK, scale=SCALE, target_replace_modules=LU.get_LoRA_module_names("attn"))
    seed_adapters(model)
    if frozen:
        freeze_base(model)
    return case, model.cuda().train()


def fused_copy(model):
    from fourm.models import lora_utils as LU
    m = copy.deepcopy(model)
    LU.fuse_LoRA_into_linear(m)
    for p in m.parameters():
        p.requires_grad = True
    return m.cuda().train()


def step(model, case, md=None):
    random.seed(case["order_seed"])
    loss, _ = model(md if md is not None else to_device(case["mod_dict"]), case["N"], case["M"], loss_type=case["loss_type"])
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach()


def logits_of(model, case):
    model.eval()
    random.seed(case["order_seed"])
    with torch.no_grad():
        out = model(to_device(case["mod_dict"]), case["N"], case["M"], return_logits=True)
    model.train()
    return out


def wrappers(model):
    from fourm.models.lora_utils import LoRAWrapper
    return {n: m for n, m in model.named_modules() if isinstance(m, LoRAWrapper)}


@pytest.mark.parametrize("name", LORA_CASES)
def test_injected_equals_fused_fp32(name):
    """fp32 verification mode: loss and logits of the injected model equal the fused model's, and every adapter gradient equals the
    chain rule through the fused model's full dW: d(up) = s dW down^T, d(down) = s up^T dW."""
    case, model = setup(name, "fp32", frozen=False)
    fused = fused_copy(model)
    fused.compute_precision = "fp32"
    l1, l2 = step(model, case), step(fused, case)
    assert model.engine.fp32 and fused.engine.fp32
    e_loss = abs(float(l1) - float(l2)) / abs(float(l2))
    lg1, lg2 = logits_of(model, case), logits_of(fused, case)
    e_logits = max(rel(lg1[k], lg2[k]) for k in lg2)
    worst = []
    for n, w in wrappers(model).items():
        dW = fused.get_submodule(n).weight.grad.double()
        worst.append((rel(w.lora_up.weight.grad, SCALE * dW @ w.lora_down.weight.double().t()), n + ".lora_up"))
        worst.append((rel(w.lora_down.weight.grad, SCALE * w.lora_up.weight.double().t() @ dW), n + ".lora_down"))
    # with the base unfrozen, every base gradient equals the fused model's
    for n, p in model.named_parameters():
        if "lora_" in n:
            continue
        q = fused.get_parameter(n.replace(".linear.", "."))
        if q.grad is None or float(q.grad.norm()) < 1e-9:
            continue
        worst.append((rel(p.grad, q.grad), n))
    worst.sort(reverse=True)
    print(f"{name}: loss {e_loss:.2e} logits {e_logits:.2e} worst gradients {worst[:3]}")
    assert e_loss < 2e-6, e_loss
    assert e_logits < 1e-5, e_logits
    assert worst[0][0] < 5e-5, worst[:6]


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("name", LORA_CASES)
def test_adapter_gradients_match_upstream(name, precision):
    """Against upstream's injected model (unmodified FourM + lora_utils): the state-dict layout, loss, logits and every adapter gradient.
    fp32 mode: each gradient tensor within 8 x upstream's own fp32-vs-float64 error of the float64 gradient; bf16: within the bf16
    gradient bound of the end-to-end tests.  The decoder's cross_attn.kv is wrapped: the engine runs the per-block context norms."""
    g = np.load(GOLD)
    case, model = setup(name, precision)
    assert list(model.state_dict().keys()) == g[f"{name}/keys"].tolist()
    loss = step(model, case)
    assert model.engine.hoist_ctx is False
    e_loss = abs(float(loss) - float(g[f"{name}/loss"])) / abs(float(g[f"{name}/loss"]))
    lg = logits_of(model, case)
    e_logits = max(rel(v, torch.from_numpy(g[f"{name}/logits/{k}"])) for k, v in lg.items())
    worst = []
    for n in lora_names(model):
        got = model.get_parameter(n).grad
        g32 = torch.from_numpy(g[f"{name}/grad/{n}"])
        g64 = g32.double() + torch.from_numpy(g[f"{name}/grad64_lo/{n}"]).double()
        own = float(g[f"{name}/grad_rel/{n}"])
        worst.append((rel(got, g64) / own if precision == "fp32" else rel(got, g32), n, own))
    worst.sort(reverse=True)
    print(f"{name} {precision}: loss {e_loss:.2e} logits {e_logits:.2e} worst adapter gradient {worst[0]}")
    if precision == "fp32":
        assert e_loss < 2e-6 and e_logits < 1e-5, (e_loss, e_logits)
        assert worst[0][0] <= 8, worst[:6]
    else:
        assert e_loss < 2e-2, e_loss
        assert worst[0][0] < 4.8e-2, worst[:6]


def test_frozen_base_leaves_no_base_gradient():
    case, model = setup("micro_swiglu")
    step(model, case)
    eng = model.engine
    live = torch.zeros_like(eng.flat_grads, dtype=torch.bool)
    for n, p in model.named_parameters():
        if "lora_" in n:
            assert p.grad is not None and float(p.grad.abs().max()) > 0, n
            o, k = eng._slices[id(p)]
            live[o:o + k] = True
        else:
            assert p.grad is None, n
    assert float(eng.flat_grads[~live].abs().max()) == 0.0
    assert len(lora_names(model)) == 2 * 14


@pytest.mark.parametrize("name", LORA_CASES)
def test_activation_checkpointing_is_bit_identical(name):
    res = []
    for ckpt in (False, True):
        case, model = setup(name, ckpt=ckpt)
        loss = step(model, case)
        res.append((float(loss), {n: model.get_parameter(n).grad.clone() for n in lora_names(model)}))
    assert res[0][0] == res[1][0]
    for n, gr in res[0][1].items():       # (the adapters' gradients meet in fp32 atomics: equal up to their summation order)
        assert rel(res[1][1][n], gr) < 2e-5, n


def test_fused_adamw_moves_adapters_only_and_the_next_forward_sees_them():
    from fourm.utils.optim_factory import FusedAdamW
    case, model = setup("micro_swiglu", "fp32")
    md = to_device(case["mod_dict"])
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    opt = FusedAdamW([{"params": [p for p in model.parameters() if p.requires_grad], "weight_decay": 0.05}], lr=1e-2, betas=(0.9, 0.95))
    l0 = step(model, case, md)
    opt.step()
    opt.zero_grad()
    for n, p in model.named_parameters():
        moved = float((p.detach() - before[n]).abs().max())
        assert (moved > 0) == ("lora_" in n), (n, moved)
    random.seed(case["order_seed"])
    with torch.no_grad():
        l1, _ = model(md, case["N"], case["M"], loss_type=case["loss_type"])
    fused = fused_copy(model)
    fused.compute_precision = "fp32"
    random.seed(case["order_seed"])
    with torch.no_grad():
        l2, _ = fused(md, case["N"], case["M"], loss_type=case["loss_type"])
    print(f"loss before the step {float(l0):.6f}, after {float(l1):.6f}, fused model with the updated adapters {float(l2):.6f}")
    assert float(l1) != float(l0)
    assert abs(float(l1) - float(l2)) < 2e-6 * abs(float(l2))


def test_eval_and_kv_cache_generation_follow_the_fused_model():
    from fourm.models.generate import GenerationSampler
    from oracle import fourm_oracle as O
    case, model = setup("micro_swiglu")
    model.eval()
    fused = fused_copy(model).eval()
    # eval forward: both within the bf16-vs-fp32 logit bound tests/test_model_gpu.py holds micro_swiglu to (1.5e-2), against upstream's fp32 logits
    g = np.load(GOLD)
    for m in (model, fused):
        lg = logits_of(m, case)
        assert max(rel(v, torch.from_numpy(g[f"micro_swiglu/logits/{k}"])) for k, v in lg.items()) < 1.5e-2
    model.eval(); fused.eval()
    cfg = case["cfg"]
    target = next(m.name for m in cfg.mods if m.kind == "seq" and m.in_dec)
    B, n_prompt = 3, 2
    md = O.synthetic_mod_dict(cfg, B, 30, 0, seed=11, no_target=tuple(m.name for m in cfg.mods))
    for d in md.values():
        d["target_mask"][:] = True
    t = md[target]
    t["tensor"] = torch.randint(5, cfg.mod(target).vocab, t["tensor"].shape, generator=torch.Generator().manual_seed(12), dtype=t["tensor"].dtype)
    t["input_mask"][:] = True; t["input_mask"][:, :n_prompt] = False
    t["target_mask"][:] = True; t["target_mask"][:, n_prompt:n_prompt + 1] = False          # one position to generate: one decode step
    u = torch.rand(1, B, generator=torch.Generator().manual_seed(13)).cuda()
    got = []
    for m in (model, fused):
        smp = GenerationSampler(m)
        out = smp.autoregressive_generate({k: {a: b.cuda() for a, b in v.items()} for k, v in md.items()}, target, temperature=0.9, top_k=40,
                                          top_p=0.0, use_eos=False, uniforms=u, keep_logits=True)
        assert tuple(out.shape) == (B, 2)
        got.append(smp.last_ar["logits"][0].float().cpu())
    e = rel(got[0], got[1])
    print(f"K/V-cache decode step, injected vs fused: {e:.2e}")
    assert e < 8e-3, e
