"""compute_precision = "fp32" of the diffusion detokenizer on the GPU: the conditional UNet on csrc/unet_f32.hip + fm_gemm_f32 and the sampling
pipeline against a float64 run of the same arithmetic (tests/divae_f64_util.py).

The rule (as in tests/test_fm_vit_gpu.py, test_memcodes_gpu.py, test_sam_instance_gpu.py): max |HIP fp32 - float64| must be at most 8 x
max |upstream's fp32 fixture - float64| on the same tensor, both computed here at run time.  The factor 8 covers what legitimately differs
between two correct fp32 evaluations: the summation order of every reduction and the device's expf / sqrt against the host's."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ml-4m_amd"))
from oracle import divae_oracle as DO  # noqa: E402
from tests import divae_f64_util as F64  # noqa: E402
from tests.parity_log import record  # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = os.path.join(ROOT, "tests", "golden", "divae_small.npz")
SMALL = dict(image_size=32, in_channels=3, out_channels=3, cond_channels=8, patch_size=4, model_channels=64, num_res_blocks=1,
             attention_resolutions=(2,), channel_mult=(1, 2))        # = tests/test_divae.py SMALL
EVALS = (("unet", False, False), ("unet_masked", True, False), ("unet_t250", False, True))      # (fixture key, conditioning mask, integer timestep)
LOOPS = (("ddim", 4), ("ddpm", 3))
FACTOR = 8.0


@functools.lru_cache(maxsize=None)
def yardstick():
    """The float64 run of every tensor the tests compare (computed once, shared, never modified) and upstream's fp32 fixture."""
    fx = np.load(GOLD)
    cfg = DO.UNetCfg(**SMALL)
    P = F64.cast_state(DO.seeded_unet_state_dict(cfg, seed=3), torch.float64)
    x, cond, ts, mask = (torch.from_numpy(fx[k]) for k in ("x", "cond", "ts", "mask"))
    ref = {}
    for name, masked, integer in EVALS:
        ref[name] = F64.unet_forward(P, cfg, x, 250 if integer else ts, cond, mask if masked else None)
    for kind, n in LOOPS:
        gen = torch.Generator().manual_seed(5)
        noise0 = torch.randn(3, 3, 32, 32, generator=gen)
        step_noise = [torch.randn(3, 3, 32, 32, generator=gen) for _ in range(n)] if kind == "ddpm" else None
        ref[f"loop_{kind}"], _ = F64.sample_loop(P, cfg, DO.SchedCfg(kind=kind), cond, noise0, n, "trailing", step_noise)
    return fx, ref


def small_net():
    from fourm.vq.models.unet import PatchedUNetCondCat
    net = PatchedUNetCondCat(**SMALL)
    net.load_state_dict(DO.seeded_unet_state_dict(DO.UNetCfg(**SMALL), seed=3), strict=True)
    return net.cuda().eval()


def under_the_rule(case, name, got):
    fx, ref = yardstick()
    assert got.dtype == torch.float32 and tuple(got.shape) == tuple(ref[name].shape)
    err = float((got.double().cpu() - ref[name]).abs().max())
    own = float((torch.from_numpy(fx[name]).double() - ref[name]).abs().max())
    print(f"{case} {name}: HIP fp32 vs float64 {err:.3e}, upstream's fp32 vs float64 {own:.3e}, ratio {err / own:.3g} (bound {FACTOR:g})")
    record("divae.fp32", case=case, tensor=name, err_vs_float64=err, upstream_err_vs_float64=own, ratio=err / own)
    assert err <= FACTOR * own, (case, name, err, own)


def inputs():
    fx, _ = yardstick()
    return tuple(torch.from_numpy(fx[k]).cuda() for k in ("x", "cond", "ts", "mask"))


def test_fp32_unet_evaluation_against_float64():
    """One evaluation with per-sample timesteps, with the conditioning mask, with an integer timestep; the same call twice gives the same bits."""
    net = small_net()
    net.compute_precision = "fp32"
    x, cond, ts, mask = inputs()
    for name, masked, integer in EVALS:
        under_the_rule("evaluation", name, net(x, 250 if integer else ts, cond, cond_mask=mask if masked else None))
    assert torch.equal(net(x, ts, cond, cond_mask=mask), net(x, ts, cond, cond_mask=mask))
    eng = net._engine
    assert eng.precision == "fp32" and all(b.dtype == torch.float32 for b in eng._buf.values())
    assert all(t.dtype == torch.float32 for hit in eng._w.values() for t in hit[1:])


def test_fp32_sampling_loop_against_float64():
    """PipelineCond for 4 DDIM / 3 DDPM steps from the CPU generator of tests/test_divae.py::test_hip_sampling_loop_matches_upstream_fixture."""
    from fourm.vq.scheduling import DDIMScheduler, DDPMScheduler, PipelineCond
    net = small_net()
    net.compute_precision = "fp32"
    cond = inputs()[1]
    for (kind, n), cls in zip(LOOPS, (DDIMScheduler, DDPMScheduler)):
        sch = cls(num_train_timesteps=1000, thresholding=True, clip_sample=False, beta_schedule="squaredcos_cap_v2", prediction_type="v_prediction", zero_terminal_snr=True)
        img = PipelineCond(model=net, scheduler=sch)(cond, generator=torch.Generator().manual_seed(5), timesteps=n, verbose=False, scheduler_timesteps_mode="trailing")
        under_the_rule(f"loop {n} steps", f"loop_{kind}", img)


def test_flipping_the_precision_on_a_live_module():
    """bf16 -> fp32 -> bf16 -> fp32 -> bf16 on one module: every fp32 evaluation is under the rule, every bf16 evaluation - eager, warm-up, capture
    and graph replays - is bit-identical to the first one; a graph of one precision is never replayed for the other."""
    import fourm.vq.models.unet.unet as U
    net = small_net()
    x, cond, ts, mask = inputs()
    saved = U.UNET_GRAPH
    try:
        U.UNET_GRAPH = False
        first = net(x, ts, cond).clone()
        assert net._engine.precision == "bf16" and any(b.dtype == torch.bfloat16 for b in net._engine._buf.values())
        for flip in range(2):
            net.compute_precision = "fp32"
            U.UNET_GRAPH = True                                        # (ignored in fp32 mode)
            for i in range(4):
                got = net(x, ts, cond)
            under_the_rule(f"flip {flip}", "unet", got)
            assert not getattr(net._engine, "_graphs", None)
            net.compute_precision = "bf16"
            for i in range(5):                                         # two eager warm-ups, the capture, two replays
                assert torch.equal(net(x, ts, cond), first), (flip, i)
            assert len(net._engine._graphs) == 1 and all(k[0] == "bf16" for k in net._engine._graphs)
        net.compute_precision = "fp16"
        with pytest.raises(ValueError, match="'bf16' or 'fp32'"):
            net(x, ts, cond)
    finally:
        U.UNET_GRAPH = saved


def test_full_size_fp32_evaluation_against_float64():
    """unet_patched at 224 x 224 (56 x 56 grid, 14 x 14 conditioning, 196 M parameters), one fp32 evaluation.  There is no upstream fixture at this
    size: the fp32 side of the rule is the CPU oracle (pinned to upstream's fixture at < 2e-6, tests/test_divae.py) on the same seeded weights."""
    from fourm.vq.models.unet import unet_patched
    ucfg = DO.unet_patched_cfg(cond_channels=32, image_size=224)
    sd = DO.seeded_unet_state_dict(ucfg, seed=1)
    net = unet_patched(in_channels=3, out_channels=3, cond_channels=32, image_size=224)
    net.load_state_dict(sd, strict=True)
    net = net.cuda().eval()
    net.compute_precision = "fp32"
    g = torch.Generator().manual_seed(2)
    quant, noised = torch.randn(1, 32, 14, 14, generator=g), torch.randn(1, 3, 224, 224, generator=g)
    got = net(noised.cuda(), 601, quant.cuda())
    ref = F64.unet_forward(F64.cast_state(sd, torch.float64), ucfg, noised, 601, quant)
    err = float((got.double().cpu() - ref).abs().max())
    own = float((DO.unet_forward(sd, ucfg, noised, 601, quant).double() - ref).abs().max())
    print(f"full size: HIP fp32 vs float64 {err:.3e}, the fp32 oracle vs float64 {own:.3e}, ratio {err / own:.3g} (bound {FACTOR:g}); output magnitude {float(ref.abs().max()):.3f}")
    record("divae.fp32", case="full size", tensor="unet_patched_t601", err_vs_float64=err, upstream_err_vs_float64=own, ratio=err / own)
    assert got.dtype == torch.float32 and err <= FACTOR * own, (err, own)
    assert all(b.dtype == torch.float32 for b in net._engine._buf.values())


def test_divae_end_to_end_in_fp32():
    """DiVAE.compute_precision = "fp32" at the configuration of test_unet_evaluation_replayed_from_a_graph_is_bit_identical: autoencode and
    decode_tokens run, give finite f32 images, and neither the tokenizer nor the decoder keeps a single bf16 buffer (= no bf16 kernel ran)."""
    from fourm.vq import DiVAE, decode_token_batches
    torch.manual_seed(0)
    m = DiVAE(image_size=64, n_channels=3, enc_type="vit_s_enc", patch_size=16, codebook_size=256, latent_dim=16, post_mlp=True, norm_codes=True,
              scheduler="ddim", prediction_type="sample", beta_schedule="linear", sync_codebook=False)
    for p in m.decoder.parameters():
        if float(p.detach().abs().max()) == 0:
            torch.nn.init.normal_(p, std=0.02)
    m = m.cuda().eval()
    m.compute_precision = "fp32"
    assert (m.compute_precision, m.encoder.compute_precision, m.decoder.compute_precision) == ("fp32",) * 3
    x = torch.rand(3, 3, 64, 64, device="cuda") * 2 - 1
    img = m.autoencode(x, timesteps=4, generator=torch.Generator().manual_seed(1), verbose=False)
    assert img.dtype == torch.float32 and tuple(img.shape) == (3, 3, 64, 64) and bool(torch.isfinite(img).all())
    tokens = m.tokenize(x)
    dec = m.decode_tokens(tokens, timesteps=4, generator=torch.Generator().manual_seed(1), verbose=False)
    assert dec.dtype == torch.float32 and bool(torch.isfinite(dec).all())
    assert torch.equal(dec, img)                                      # autoencode = tokenize + decode_tokens, bit for bit
    out, code_loss = m(x, torch.randn_like(x), torch.tensor([601, 20, 999], device="cuda"))
    assert out.dtype == torch.float32 and bool(torch.isfinite(out).all())
    ue, ve = m.decoder._engine, m.encoder._hip_engine
    assert ue.precision == "fp32" and ue._buf and all(b.dtype == torch.float32 for b in ue._buf.values())
    assert all(t.dtype == torch.float32 for hit in ue._w.values() for t in hit[1:])
    assert ve.fp32 and ve.adt == torch.float32 and not ve.shadows        # (shadows = the bf16 weight images of the trunk engine)
    assert all(t.dtype != torch.bfloat16 for t in ve.ws.bufs.values())
    # two decodes in flight on two streams, still fp32, still the same bits
    toks = [tokens, tokens[:2].contiguous(), tokens[1:].contiguous()]
    want = [m.decode_tokens(t, timesteps=2, generator=torch.Generator().manual_seed(7 + i), verbose=False).clone() for i, t in enumerate(toks)]
    got = decode_token_batches(m, toks, n_streams=2, timesteps=2, generator=[torch.Generator().manual_seed(7 + i) for i in range(3)], verbose=False)
    torch.cuda.synchronize()
    assert all(torch.equal(g, w) for g, w in zip(got, want))
    m.train()
    with torch.no_grad(), pytest.raises(NotImplementedError, match="inference only"):
        m.encode(x)                                                   # (training mode would move the codebook: not built in fp32)
