"""K/V-cache decoding of the trunk variants that run on fm_attn_decode: qk_norm models (NormAttention / NormCrossAttention) and the fp32
verification mode.  Same structure as tests/test_generate_gpu.py::test_autoregressive_kv_cache: B = 3, a 2-token prompt, 9 generated
tokens, fixed uniforms; every step's logits against the oracle's NON-cached recompute of the whole prefix under a causal mask."""
import copy

import numpy as np
import pytest
import torch

from oracle import fourm_oracle as O
from oracle import sample_oracle as S
from tests.golden.cases import build_case
from tests.lora_util import RANK, SCALE, seed_adapters
from tests.parity_log import record
from tests.test_generate_gpu import sampler
from tests.util_model import build_hip_model, tie

pytestmark = pytest.mark.gpu
B, N_PROMPT, N_GEN = 3, 2, 9
TEMP, TOP_K = 0.9, 40


def setup(case_name, precision):
    case = build_case(case_name)
    cfg = case["cfg"]
    target = next(m.name for m in cfg.mods if m.kind == "seq" and m.in_dec)
    model = build_hip_model(cfg, case["share_embedding"], case["norm_bias"], case["learned_pos"])
    model.load_state_dict(case["sd"], strict=True)
    model.compute_precision = precision
    model = model.cuda().eval()
    md = O.synthetic_mod_dict(cfg, B, 30, 0, seed=11, no_target=tuple(m.name for m in cfg.mods))
    for d in md.values():
        d["target_mask"][:] = True
    t = md[target]
    t["tensor"] = torch.randint(5, cfg.mod(target).vocab, t["tensor"].shape, generator=torch.Generator().manual_seed(12), dtype=t["tensor"].dtype)
    t["input_mask"][:] = True; t["input_mask"][:, :N_PROMPT] = False          # a short visible prompt ...
    t["target_mask"][:] = True; t["target_mask"][:, N_PROMPT:N_PROMPT + N_GEN] = False      # ... then the positions to generate
    u = torch.rand(N_GEN, B, generator=torch.Generator().manual_seed(13))
    return case, model, md, target, u


def fresh(md):
    return {k: {a: b.cuda() for a, b in v.items()} for k, v in md.items()}


def decode(smp, md, target, u, **kw):
    """-> (ids (B, 1 + steps), [logits of every step, on the host])"""
    out = smp.autoregressive_generate(fresh(md), target, TEMP, TOP_K, 0.0, use_eos=False, uniforms=u.cuda(), keep_logits=True, **kw)
    return out, [l.cpu() for l in smp.last_ar["logits"]]


def worst_vs_oracle(P, case, md, target, out, got, emulate_bf16):
    """Worst relative distance (Frobenius, per step) between the cached logits ``got`` and the oracle's recompute of every prefix of ``out``."""
    cfg, spec, num = case["cfg"], case["cfg"].mod(target), O._Num(emulate_bf16)
    with torch.no_grad():
        n_enc = max(int(sum((~md[m.name]["input_mask"].reshape(B, -1)[b]).sum() for m in cfg.mods if m.in_enc)) for b in range(B))
        enc = O.select_encoder(P, cfg, md, n_enc, num)
        x = O.encoder_forward(P, cfg, enc["tokens"] + enc["emb"], enc["mask"], num)
        ctx = num.linear(x, P["decoder_proj_context.weight"], P["decoder_proj_context.bias"]) + enc["emb"]
        _, e, _ = O.embed_decoder_modality(P, spec, md[target])
        y_emb = e.float()[:, N_PROMPT:N_PROMPT + N_GEN]
        table = P[f"decoder_embeddings.{target}.token_emb.weight"]
        worst = 0.0
        for i in range(len(got)):
            cur = i + 1
            y = table[out[:, :cur].cpu()] + y_emb[:, :cur]
            causal = torch.ones(cur, cur, dtype=torch.bool).triu(1)[None].expand(B, -1, -1)
            yd = O.decoder_forward(P, cfg, y, ctx, enc["mask"], causal, num)
            want = num.linear(yd[:, -1], P[f"decoder_embeddings.{target}.to_logits.weight"], None)
            worst = max(worst, float((got[i].double() - want.double()).norm() / want.double().norm()))
    return worst


def check_sampling(out, got, u):
    assert tuple(out.shape) == (B, 1 + N_GEN)
    for i in range(N_GEN):
        ids, _ = S.sample_tokens(got[i].float().numpy().copy(), TEMP, TOP_K, 0.0, u[i].numpy())
        assert np.array_equal(out[:, i + 1].cpu().numpy(), ids), i


def test_qknorm_bf16_kv_cache_decoding():
    """micro_qknorm in bf16: the cache holds normalised keys (written by fm_attn_decode), the context keys are normalised once.  The
    bound is the 1.2e-2 relative of the bf16 test without qk_norm."""
    case, model, md, target, u = setup("micro_qknorm", "bf16")
    cfg = case["cfg"]
    assert model.engine.qk_norm and not model.engine.fp32
    P = tie({k: v.clone() for k, v in case["sd"].items()}, cfg, case["share_embedding"])
    smp = sampler(model)
    out, got = decode(smp, md, target, u)
    assert got[0].dtype == torch.float32
    check_sampling(out, got, u)                                                   # ids bit-exact from the kernel's own logits
    worst = worst_vs_oracle(P, case, md, target, out, got, True)
    record("generate.autoregressive_logits_qknorm", case="micro_qknorm", worst_rel=worst, steps=N_GEN)
    print(f"micro_qknorm bf16 cached vs recomputed logits: worst rel {worst:.3e}")
    assert worst < 1.2e-2, worst
    # ---- several start tokens: the prefix fills the cache (and normalises its keys) before the first sampled token ----
    smp.autoregressive_generate(fresh(md), target, TEMP, TOP_K, 0.0, use_eos=False, uniforms=u.cuda(), keep_logits=True, start_tokens=out[:, :3])
    assert torch.equal(smp.last_ar["logits"][0].cpu(), got[2])
    # ---- end of sequence: a batch of one stops as soon as it has produced the token ----
    eos = int(out[0, 3])
    one = {k: {a: b[:1].cuda() for a, b in v.items()} for k, v in md.items()}
    out2 = smp.autoregressive_generate(one, target, TEMP, TOP_K, 0.0, use_eos=True, eos_token=eos, uniforms=u[:, :1].cuda())
    first = int((out[0] == eos).nonzero()[0])
    assert out2.shape[1] == first + 1 and torch.equal(out2[0], out[0, :first + 1])
    # ---- classifier-free guidance: two decoder states, the first-step logits are the fp32 combination of the two unguided runs ----
    cond_mod = next(m.name for m in cfg.mods if m.in_enc and m.name != target and m.kind == "tok" and bool((~md[m.name]["input_mask"]).any()))
    smp.autoregressive_generate(smp.unconditional_dict(fresh(md), [cond_mod]), target, TEMP, TOP_K, 0.0, use_eos=False, uniforms=u.cuda(), keep_logits=True)
    lu0 = smp.last_ar["logits"][0].cpu().numpy()
    lc0 = got[0].numpy()
    assert float(np.abs(lc0 - lu0).max()) > 1e-3
    outg, gotg = decode(smp, md, target, u, conditioning=[cond_mod], guidance_scale=3.0)
    assert np.array_equal(gotg[0].numpy(), S.cfg_logits(lc0, lu0, 3.0))
    check_sampling(outg, gotg, u)
    # ---- hipGraph replay of the per-position launch sequences: bit-identical to eager, twice (the second call reuses the graphs) ----
    for rep in range(2):
        outr, gotr = decode(smp, md, target, u, use_graphs=True)
        assert torch.equal(outr, out), rep
        for i in range(N_GEN):
            assert torch.equal(gotr[i], got[i]), (rep, i)
    assert len(smp._ar_graphs) == N_GEN
    outg2 = smp.autoregressive_generate(fresh(md), target, TEMP, TOP_K, 0.0, use_eos=False, uniforms=u.cuda(), conditioning=[cond_mod],
                                        guidance_scale=3.0, use_graphs=True)
    assert torch.equal(outg2, outg)
    # ---- LoRA on the attention Linears: the cached path follows the oracle on the FUSED weights.  Tolerance: the 1.5e-2 that
    # tests/test_lora_gpu.py holds the bf16 eval forward of the injected and the fused model to ----
    from fourm.models import lora_utils as LU
    LU.inject_trainable_LoRA(model, rank=RANK, scale=SCALE, target_replace_modules=LU.get_LoRA_module_names("attn"))
    seed_adapters(model)
    model = model.cuda().eval()
    fused = copy.deepcopy(model)
    LU.fuse_LoRA_into_linear(fused)
    Pf = tie({k: v.detach().cpu().clone() for k, v in fused.state_dict().items()}, cfg, case["share_embedding"])
    assert set(Pf) == set(P) and any(not torch.equal(Pf[k], P[k]) for k in P)
    outl, gotl = decode(sampler(model), md, target, u)
    check_sampling(outl, gotl, u)
    worst_l = worst_vs_oracle(Pf, case, md, target, outl, gotl, True)
    record("generate.autoregressive_logits_qknorm_lora", case="micro_qknorm", worst_rel=worst_l, steps=N_GEN)
    print(f"micro_qknorm bf16 + LoRA cached vs recomputed (fused weights) logits: worst rel {worst_l:.3e}")
    assert worst_l < 1.5e-2, worst_l


@pytest.mark.parametrize("case_name", ["micro_swiglu", "micro_qknorm"])
def test_fp32_mode_kv_cache_decoding(case_name):
    """compute_precision = "fp32": fp32 cache, fp32 logits.  The cached and the recomputed path differ in summation order only, so the
    bound is the 1e-5 that tests/test_model_gpu.py::test_fp32_verification_mode holds the logits of these fixtures to."""
    case, model, md, target, u = setup(case_name, "fp32")
    cfg = case["cfg"]
    P = tie({k: v.clone() for k, v in case["sd"].items()}, cfg, case["share_embedding"])
    smp = sampler(model)
    out, got = decode(smp, md, target, u)
    assert model.engine.fp32 and model.engine.adt == torch.float32 and model.engine.qk_norm == (case_name == "micro_qknorm")
    check_sampling(out, got, u)
    worst = worst_vs_oracle(P, case, md, target, out, got, False)
    record("generate.autoregressive_logits_fp32", case=case_name, worst_rel=worst, steps=N_GEN)
    print(f"{case_name} fp32 cached vs recomputed logits: worst rel {worst:.3e}")
    assert worst < 1e-5, worst
    # captured replay is bit-identical to eager in this mode too
    outr, gotr = decode(smp, md, target, u, use_graphs=True)
    assert torch.equal(outr, out) and all(torch.equal(a, b) for a, b in zip(gotr, got))
