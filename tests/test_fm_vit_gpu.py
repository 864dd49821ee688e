"""FourMViT on a real MI355X against the unmodified upstream class (tests/golden/fm_vit_micro.npz, CPU): output and parameter gradients
in both precisions, the autograd bridge under a torch head, freezing, FusedAdamW, LoRA, eval.

Bounds, fixed before anything was measured:
  fp32 verification mode: max |x - float64| of the output and of every gradient tensor (on the elements the fixture keeps) at most
      8 x upstream's own fp32-vs-float64 maximum on the same elements - the factor tests/test_memcodes_gpu.py, test_sam_instance_gpu.py
      and test_lora_gpu.py use for this construction;
  bf16: relative Frobenius error against float64 at most 2 x that of upstream's own torch.autocast(bfloat16) run - the factor by which
      LOGIT_BOUNDS of tests/test_model_gpu.py sit above upstream's autocast gap (1.5e-2 / 7.6e-3, 1.9e-2 / 9.6e-3);
  FusedAdamW against torch.optim.AdamW on the same gradients: 2e-6 absolute, as test_fused_adamw_step_matches_torch.
Measured ratios are printed by every test."""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import fm_vit_util as U

pytestmark = pytest.mark.gpu
_G = {}
FP32_FACTOR, BF16_FACTOR = 8.0, 2.0


def gold():
    if "g" not in _G:
        _G["g"] = np.load(os.path.join(os.path.dirname(__file__), "golden", "fm_vit_micro.npz"))
    return _G["g"]


class MeanHead(nn.Module):
    def __init__(self):
        super().__init__()
        self.fc = nn.Linear(U.DIM, U.CLASSES)

    def forward(self, x):
        return self.fc(x.mean(1))


def build(name, precision, head=None, **extra):
    from fourm.models.fm_utils import LayerNorm
    from fourm.models.fm_vit import FourMViT
    model = FourMViT(output_head=head, **{**U.model_kwargs(name, LayerNorm), **extra})
    sd = U.seeded_state_dict(model, torch.from_numpy(gold()["pos_emb"]))
    if head is not None:
        hs, _ = U.head_state()
        sd.update({"output_head.fc.weight": hs["weight"], "output_head.fc.bias": hs["bias"]})
    model.load_state_dict(sd, strict=True)
    model.compute_precision = precision
    return model.cuda().train()


def ref64(prefix, k):
    g = gold()
    return torch.from_numpy(g[f"{prefix}/g32/{k}"]).double() + torch.from_numpy(g[f"{prefix}/g64_lo/{k}"]).double()


def sampled(t, k, n=U.SAMPLE):
    return t.detach().reshape(-1).cpu()[torch.from_numpy(U.sample_index(k, t.numel(), n))].double()


def step(model, batch=0, cot=None):
    out = model(U.images(batch).cuda())
    cot = U.cotangent() if cot is None else cot
    (out * cot.cuda()).sum().backward()
    torch.cuda.synchronize()
    return out.detach()


def grad_ratios(model, prefix, n=U.SAMPLE, skip=()):
    """(max |got - float64| / upstream's own maximum, name) per parameter, on the elements the fixture keeps."""
    g, res = gold(), []
    for k, p in model.named_parameters():
        if k.startswith(skip):
            continue
        assert p.grad is not None, k
        err = float((sampled(p.grad, k, n) - ref64(prefix, k)).abs().max())
        res.append((0.0 if err == 0 else err / float(g[f"{prefix}/g_err/{k}"]), k))          # (an exact tensor meets any bound)
    return sorted(res, reverse=True)


@pytest.mark.parametrize("name", list(U.CASES))
def test_fp32_mode_against_float64(name):
    g = gold()
    model = build(name, "fp32")
    out = step(model)
    assert model.engine.fp32 and out.dtype == torch.float32 and tuple(out.shape) == (U.BATCH, U.NP, U.DIM)
    o64 = torch.from_numpy(g[f"{name}/out32"]).double() + torch.from_numpy(g[f"{name}/out64_lo"]).double()
    r_out = float((out.cpu().double() - o64).abs().max()) / float(g[f"{name}/out_err"])
    ratios = grad_ratios(model, name)
    print(f"{name} fp32: output max-abs error / upstream's own {r_out:.3g}; gradients worst {ratios[0][0]:.3g} ({ratios[0][1]}), "
          f"median {np.median([r[0] for r in ratios]):.3g} (bound {FP32_FACTOR:g})")
    assert r_out <= FP32_FACTOR, r_out
    assert ratios[0][0] <= FP32_FACTOR, ratios[:6]


@pytest.mark.parametrize("name", list(U.CASES))
def test_bf16_mode_no_worse_than_upstream_autocast(name):
    g = gold()
    model = build(name, "bf16")
    out = step(model)
    assert not model.engine.fp32 and out.dtype == torch.float32
    o64 = torch.from_numpy(g[f"{name}/out32"]).double() + torch.from_numpy(g[f"{name}/out64_lo"]).double()
    r_out = float((out.cpu().double() - o64).norm() / o64.norm()) / float(g[f"{name}/out_ac_rel"])
    res = []
    for k, p in model.named_parameters():
        r64 = ref64(name, k)
        res.append((float((sampled(p.grad, k) - r64).norm() / r64.norm()) / float(g[f"{name}/ac_rel/{k}"]), k))
    res.sort(reverse=True)
    print(f"{name} bf16: output rel error / upstream autocast's {r_out:.3g}; gradients worst {res[0][0]:.3g} ({res[0][1]}), "
          f"median {np.median([r[0] for r in res]):.3g} (bound {BF16_FACTOR:g})")
    assert r_out <= BF16_FACTOR, r_out
    assert res[0][0] <= BF16_FACTOR, res[:6]


def test_dense_front_end_equals_the_selected_patch_path():
    """The encoder weights of a FourM micro model in a FourMViT: bit for bit (fp32 mode) what the same engine family gives for that
    FourM's encoder on an all-visible RGB input, embedded by fm_select_embed."""
    from tests.golden.cases import build_case
    from tests.util_model import build_hip_model
    case = build_case("micro_swiglu")
    fm = build_hip_model(case["cfg"], case["share_embedding"], case["norm_bias"], case["learned_pos"])
    fm.load_state_dict(case["sd"], strict=True)
    fm.compute_precision = "fp32"
    fm = fm.cuda().eval()
    vit = build("swiglu", "fp32")
    vit.load_state_dict(case["sd"], strict=False)
    vit = vit.cuda().eval()
    x = U.images(0).cuda()
    with torch.no_grad():
        got = vit(x)
        eng = fm.engine
        eng.prepare()
        md = {"rgb@32": {"tensor": x, "input_mask": torch.zeros(U.BATCH, U.NP, dtype=torch.bool, device="cuda")}}
        s = eng.select(md, U.NP, False, ["rgb@32"], "xcheck.")
        x0 = s["x0"][:U.BATCH * U.NP].view(U.BATCH, U.NP, U.DIM).clone()
        ref = fm.forward_encoder(x0, None)
    torch.cuda.synchronize()
    assert torch.equal(s["patch_rows"][:U.BATCH * U.NP].cpu(), vit.engine.ws.get("vit.patch_rows", tuple(s["patch_rows"].shape), torch.float32)[:U.BATCH * U.NP].cpu())
    print(f"dense vs selected front end: max abs difference {float((got - ref).abs().max()):.3g}")
    assert torch.equal(got, ref)


def test_autograd_bridge_with_a_torch_head_accumulates():
    g = gold()
    _, hcot = U.head_state()
    model = build("swiglu", "fp32", head=MeanHead())
    for b in (0, 1):
        step(model, b, hcot)
        ratios = grad_ratios(model, f"head{b}", U.HEAD_SAMPLE)
        print(f"head composition after batch {b}: worst gradient ratio {ratios[0][0]:.3g} ({ratios[0][1]}) (bound {FP32_FACTOR:g})")
        assert ratios[0][0] <= FP32_FACTOR, ratios[:6]
        assert any(k.startswith("output_head") for _, k in ratios)
    eng = model.engine
    assert model.output_head.fc.weight.grad.data_ptr() != eng.flat_grads.data_ptr() and id(model.output_head.fc.weight) not in eng._slices
    assert model.encoder[0].attn.qkv.weight.grad.data_ptr() == eng.grad_view(model.encoder[0].attn.qkv.weight).data_ptr()
    model.zero_grad(set_to_none=True)          # a cleared window starts from zero again
    step(model, 0, hcot)
    assert grad_ratios(model, "head0", U.HEAD_SAMPLE)[0][0] <= FP32_FACTOR


def test_frozen_encoder_keeps_nothing_and_embeddings_can_stay_trainable():
    model = build("swiglu", "bf16", head=MeanHead())
    x = U.images(0).cuda()
    full = model(x)
    (full * U.head_state()[1].cuda()).sum().backward()
    model.zero_grad(set_to_none=True)
    model.freeze_encoder()
    out = model(x)
    assert model.engine._ctx is None and out.grad_fn is not None          # (the head's graph only)
    assert torch.equal(out.detach(), full.detach())
    (out * U.head_state()[1].cuda()).sum().backward()
    assert all(p.grad is None for _, p in model.engine_parameters()) and model.output_head.fc.weight.grad is not None
    model.zero_grad(set_to_none=True)
    model.freeze_encoder(freeze_embeddings=False)
    for p in model.encoder_embeddings.parameters():
        p.requires_grad = True
    out = model(x)
    assert model.engine._ctx is not None and torch.equal(out.detach(), full.detach())
    (out * U.head_state()[1].cuda()).sum().backward()
    torch.cuda.synchronize()
    assert model.engine._ctx is None
    for k, p in model.engine_parameters():
        if k.startswith("encoder_embeddings"):
            assert p.grad is not None and float(p.grad.abs().max()) > 0, k
        else:
            assert p.grad is None, k


def test_fused_adamw_step_matches_torch():
    from fourm.utils.optim_factory import FusedAdamW
    model = build("gelu", "bf16", head=MeanHead())
    named = list(model.engine_parameters())          # (the head would take a torch optimizer of its own)
    ref = {n: p.detach().clone().requires_grad_(True) for n, p in named}
    groups = lambda named: [{"params": [p for n, p in named if p.dim() > 1], "weight_decay": 0.05},
                            {"params": [p for n, p in named if p.dim() <= 1], "weight_decay": 0.0}]
    opt = FusedAdamW(groups(named), lr=1e-3, betas=(0.9, 0.95))
    ropt = torch.optim.AdamW(groups(list(ref.items())), lr=1e-3, betas=(0.9, 0.95))
    before = model(U.images(1).cuda()).detach()
    for b in (0, 1):
        step(model, b, U.head_state()[1])
        for n, p in named:
            ref[n].grad = p.grad.clone()
        opt.step(); ropt.step()
        opt.zero_grad(); ropt.zero_grad()
        model.output_head.zero_grad()
    worst = max((float((p - ref[n]).abs().max()), n) for n, p in named)
    print(f"FusedAdamW vs torch.optim.AdamW after two steps: worst {worst}")
    assert worst[0] < 2e-6, worst
    assert not torch.equal(model(U.images(1).cuda()).detach(), before)          # the next forward runs on the updated weight shadows


def test_lora_adapters_train_on_a_frozen_base_and_fuse():
    from fourm.models import lora_utils as LU
    from tests.lora_util import freeze_base, seed_adapters
    g = gold()
    model = build("swiglu", "fp32")
    LU.inject_trainable_LoRA(model, rank=4, scale=0.5)
    seed_adapters(model)
    freeze_base(model)
    model = model.cuda().train()
    out = step(model)
    n_adapters = 0
    for k, p in model.named_parameters():
        if "lora_" in k:
            assert p.grad is not None and float(p.grad.abs().max()) > 0, k
            n_adapters += 1
        else:
            assert p.grad is None, k
    assert n_adapters == 2 * 2 * U.DEPTH
    fused = build("swiglu", "fp32")
    LU.inject_trainable_LoRA(fused, rank=4, scale=0.5)
    seed_adapters(fused)
    LU.fuse_LoRA_into_linear(fused)
    fused = fused.cuda().eval()
    with torch.no_grad():
        ref = fused(U.images(0).cuda())
    r = float((out - ref).abs().max()) / float(g["swiglu/out_err"])
    print(f"LoRA injected vs fused (fp32 mode): max abs difference / upstream's fp32-vs-float64 output error {r:.3g} (bound {FP32_FACTOR:g})")
    assert r <= FP32_FACTOR, r
    assert float((out - torch.from_numpy(g["swiglu/out32"]).cuda()).abs().max()) > 1e-3          # the adapters do change the output


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_eval_and_no_grad_return_the_training_bits(precision):
    model = build("qknorm", precision)
    x = U.images(0).cuda()
    train_out = model(x)
    assert train_out.grad_fn is not None and model.engine._ctx is not None
    with torch.no_grad():
        ng = model(x)
    assert model.engine._ctx is None and ng.grad_fn is None
    ev = model.eval()(x)
    assert ev.grad_fn is None and model.engine._ctx is None
    assert torch.equal(train_out.detach(), ng) and torch.equal(ng, ev)


def test_drop_path_runs_in_training_only():
    model = build("swiglu", "bf16", drop_path_rate=0.5)
    x = U.images(0).cuda()
    torch.manual_seed(0)
    a = step(model)
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for _, p in model.engine_parameters())
    ref = build("swiglu", "bf16").eval()
    with torch.no_grad():
        assert torch.equal(model.eval()(x), ref(x)) and not torch.equal(a, ref(x))
