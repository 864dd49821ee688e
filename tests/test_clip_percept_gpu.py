"""The CLIP perceptual loss on a real MI355X: loss (B,) and d loss.sum() / d preds against float64 autograd of
tests/clip_percept_util.py::percept_ref (upstream's arithmetic on the float64 restatement of the tower, pinned by tests/test_clip_percept_cpu.py).

fp32 mode: max |a - ref| / max |ref| <= 8 x max(the same distance of percept_ref evaluated in float32 on the CPU, 2^-24) per tensor - the
           project's fp32 rule.
bf16 mode: the same distance <= 2 x that of percept_ref run on the CPU under torch.autocast("cpu", torch.bfloat16), forward and backward.
           The engine rounds where autocast does not (bf16 LayerNorm outputs, attention probabilities, the bf16 copy of the stream gradient)
           and keeps fp32 where autocast rounds (the residual stream): errors of one size, not equal - the margin of the tower's forward test.
           Every ratio goes to the parity log.
Measured on an MI355X (this file's run): see INTEGRATION.md, "CLIP perceptual loss"."""
import pytest
import torch
import torch.nn.functional as F

from tests import clip_percept_util as PU
from tests import clip_util as U
from tests.parity_log import record

pytestmark = pytest.mark.gpu

DEV = "cuda"
CASES = [("clip_a", "blocks.0-blocks.1"), ("clip_a", "blocks.1"), ("clip_b", "blocks.0")]
MODES = ["cosine", "l1"]
IDS = [(c, f, m) for c, f in CASES for m in MODES]


def taps_of(feature_ids):
    return [int(s.split(".")[1]) for s in feature_ids.split("-")]


def inputs(case):
    """targets: the tower tests' images at the native resolution; preds = targets + 0.3 randn (seeded)."""
    targets = U.images(case, "native")
    g = torch.Generator().manual_seed(4000 + sorted(U.CASES).index(case))
    return targets + 0.3 * torch.randn(targets.shape, generator=g), targets


def make_loss(case, feature_ids, mode, precision="bf16"):
    from fourm.utils.clip.model import VisionTransformer
    from fourm.vq.percept_losses import ClipPerceptualLoss
    vis = VisionTransformer(**U.CASES[case])
    vis.load_state_dict(U.seeded_state_dict(case), strict=True)
    vis.compute_precision = precision
    return ClipPerceptualLoss(vis, feature_ids, feature_loss=mode).to(DEV)


def ref_run(case, feature_ids, mode, dtype, autocast=False, weights=None):
    sd = U.seeded_state_dict(case)
    preds, targets = inputs(case)
    p = preds.to(dtype).requires_grad_()
    with torch.autocast("cpu", torch.bfloat16, enabled=autocast):
        loss = PU.percept_ref(sd, p, targets.to(dtype), taps_of(feature_ids), mode, dtype)
        total = loss.sum() if weights is None else (loss * weights.to(loss.dtype)).sum()
    grad, = torch.autograd.grad(total, p)
    return loss.detach(), grad


@pytest.fixture(scope="module")
def refs():
    """Per case: float64 (the reference), float32 and CPU-autocast (the yardsticks) loss and pixel gradient; computed once, never modified."""
    out = {}
    for case, fid, mode in IDS:
        out[case, fid, mode] = dict(f64=ref_run(case, fid, mode, torch.float64), f32=ref_run(case, fid, mode, torch.float32),
                                    ac=ref_run(case, fid, mode, torch.float32, autocast=True))
    return out


def hip_run(loss_mod, case, weights=None, **kw):
    preds, targets = inputs(case)
    p = preds.to(DEV).requires_grad_()
    loss = loss_mod(p, targets.to(DEV), **kw)
    (loss.sum() if weights is None else (loss * weights.to(DEV)).sum()).backward()
    return loss.detach(), p.grad


@pytest.mark.parametrize("case,fid,mode", IDS)
def test_fp32_mode_against_float64(case, fid, mode, refs):
    loss, grad = hip_run(make_loss(case, fid, mode, "fp32"), case)
    r = refs[case, fid, mode]
    assert loss.dtype == torch.float32 and loss.shape == r["f64"][0].shape and grad.shape == r["f64"][1].shape
    for name, got, k in (("loss", loss, 0), ("grad", grad, 1)):
        err, own = U.rel_max(got, r["f64"][k]), U.rel_max(r["f32"][k], r["f64"][k])
        bound = 8 * max(own, 2.0 ** -24)
        print(f"percept fp32 {case}/{fid}/{mode} {name}: {err:.3e} vs float64 (torch fp32 {own:.3e}, ratio {err / max(own, 2.0 ** -24):.2f}, bound {bound:.3e})")
        record("clip.percept.fp32", case=case, taps=fid, mode=mode, tensor=name, err=err, torch_fp32_err=own, ratio=err / max(own, 2.0 ** -24))
        assert err <= bound, (case, fid, mode, name, err, bound)


@pytest.mark.parametrize("case,fid,mode", IDS)
def test_bf16_mode_against_float64(case, fid, mode, refs):
    mod = make_loss(case, fid, mode)
    assert mod.visual.compute_precision == "bf16"
    loss, grad = hip_run(mod, case)
    r = refs[case, fid, mode]
    assert loss.dtype == torch.float32 and grad.dtype == torch.float32
    for name, got, k in (("loss", loss, 0), ("grad", grad, 1)):
        err, own = U.rel_max(got, r["f64"][k]), U.rel_max(r["ac"][k], r["f64"][k])
        print(f"percept bf16 {case}/{fid}/{mode} {name}: {err:.3e} vs float64 (CPU autocast {own:.3e}, ratio {err / own:.2f}, bound 2)")
        record("clip.percept.bf16", case=case, taps=fid, mode=mode, tensor=name, err=err, cpu_autocast_err=own, ratio=err / own)
        assert err <= 2 * own, (case, fid, mode, name, err, own)


@pytest.mark.parametrize("mode", MODES)
def test_non_uniform_incoming_gradient_scales_per_sample(mode):
    """(loss * w).sum() with a random w: sample b's pixel gradient is w[b] times its gradient under loss.sum() - checked against float64 in
    fp32 mode by the rule above."""
    case, fid = "clip_a", "blocks.0-blocks.1"
    w = torch.randn(3, generator=torch.Generator().manual_seed(9)).abs() + 0.25
    w[1] = -w[1]
    _, grad = hip_run(make_loss(case, fid, mode, "fp32"), case, weights=w)
    ref = ref_run(case, fid, mode, torch.float64, weights=w)[1]
    own = ref_run(case, fid, mode, torch.float32, weights=w)[1]
    err, bound = U.rel_max(grad, ref), 8 * max(U.rel_max(own, ref), 2.0 ** -24)
    assert err <= bound, (err, bound)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_preprocess_inputs_equals_the_transform_applied_outside(precision):
    """The affine folded into the patch gather (and its scale applied on the way out of the backward) against percept_transform in front of
    the loss: the same loss bits; in fp32 mode the same pixel-gradient bits after autograd's chain rule."""
    case = "clip_a"
    mod = make_loss(case, "blocks.0-blocks.1", "cosine", precision)
    preds, targets = inputs(case)
    preds, targets = (0.4 * preds).to(DEV), (0.4 * targets).to(DEV)
    a = preds.clone().requires_grad_()
    la = mod(a, targets, preprocess_inputs=True)
    la.sum().backward()
    b = preds.clone().requires_grad_()
    lb = mod(mod.percept_transform(b), mod.percept_transform(targets))
    lb.sum().backward()
    assert torch.equal(la, lb) and not torch.equal(la, mod(preds, targets))
    assert torch.equal(a.grad, b.grad)                       # (both modes: the same launches on the same rows, one rounding of grad * scale)


def test_targets_get_no_gradient_and_no_grad_saves_nothing():
    case = "clip_b"
    mod = make_loss(case, "blocks.0", "cosine")
    preds, targets = inputs(case)
    p, t = preds.to(DEV).requires_grad_(), targets.to(DEV).requires_grad_()
    loss = mod(p, t)
    assert loss.grad_fn is not None and loss.shape == (5,)
    loss.sum().backward()
    assert t.grad is None and p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0
    with torch.no_grad():
        quiet = mod(p, t)
    assert quiet.grad_fn is None and not quiet.requires_grad and torch.equal(quiet, loss.detach())
    assert mod.visual.__dict__.get("_feat_saved") is None
    plain = mod(preds.to(DEV), t)                                       # preds that ask for no gradient: no graph either
    assert plain.grad_fn is None and torch.equal(plain, loss.detach())
    assert not any(q.grad is not None for q in mod.visual.parameters())


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_two_identical_runs_give_identical_bits(precision):
    mod = make_loss("clip_a", "blocks.0-blocks.1", "l1", precision)
    l1, g1 = hip_run(mod, "clip_a")
    l2, g2 = hip_run(mod, "clip_a")
    assert torch.equal(l1, l2) and torch.equal(g1, g2)


def test_backward_after_a_newer_forward_raises():
    mod = make_loss("clip_a", "blocks.1", "cosine")
    preds, targets = inputs("clip_a")
    p, t = preds.to(DEV).requires_grad_(), targets.to(DEV)
    first = mod(p, t)
    second = mod(p, t)
    with pytest.raises(RuntimeError, match="most recent training forward only"):
        first.sum().backward()
    second.sum().backward()                                             # the newer one is intact
    assert p.grad is not None and bool(torch.isfinite(p.grad).all())
    with torch.no_grad():                                               # a pass that keeps no state does not disturb one that does
        third = mod(p, t)
        mod.visual(t)
    p.grad = None
    fourth = mod(p, t)
    with torch.no_grad():
        mod(p, t)
        mod.visual(t)
    fourth.sum().backward()
    assert torch.equal(third, fourth.detach()) and bool(torch.isfinite(p.grad).all())


@pytest.fixture(scope="module")
def vqvae_steps():
    """One micro VQ-VAE (the configuration of tests/test_vqvae.py's optimizer test: image 32, vit_s encoder / decoder, patch 8) with the clip_a
    tower behind it.  Route "one": (mse + 0.5 percept.mean()).backward().  Route "two": d / d dec of the same scalar with dec detached as a
    leaf, then dec.backward(gradient=...).  "again": route two a second time.  Parameter gradients of each, the gradient that reached dec."""
    from fourm.vq import VQVAE
    torch.manual_seed(0)
    m = VQVAE(dec_type="vit_s_dec", image_size=32, enc_type="vit_s_enc", patch_size=8, post_mlp=True, codebook_size=64, latent_dim=32,
              norm_codes=True, sync_codebook=False, threshold_ema_dead_code=0).cuda().train()
    m.quantize.eval()                                                   # keep the codebook fixed: identical steps
    percept = make_loss("clip_a", "blocks.0-blocks.1", "cosine")
    x = torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(1)).clamp(-1, 1).cuda()

    def objective(dec):
        return F.mse_loss(dec, x) + 0.5 * percept(dec, x, preprocess_inputs=True).mean()

    def grads():
        missing = [k for k, p in m.named_parameters() if p.requires_grad and p.grad is None]
        out = {k: p.grad.clone() for k, p in m.named_parameters() if p.requires_grad and p.grad is not None}
        m.zero_grad(set_to_none=True)
        return out, missing

    res = {}
    dec, _ = m(x)
    dec.register_hook(lambda g: res.__setitem__("g_dec_one", g.clone()))
    objective(dec).backward()
    res["one"], res["missing"] = grads()
    for name in ("two", "again"):
        dec, _ = m(x)
        leaf = dec.detach().requires_grad_()
        objective(leaf).backward()
        res["g_dec_" + name] = leaf.grad.clone()
        res["g_mse"] = torch.autograd.grad(F.mse_loss(leaf, x), leaf)[0]
        dec.backward(gradient=leaf.grad)
        res[name], _ = grads()
    return res


def test_vqvae_training_step_with_the_perceptual_term(vqvae_steps):
    """(mse + 0.5 percept(dec, x, preprocess_inputs=True).mean()).backward() through the VQ-VAE's own hand-written backward fills every trainable
    gradient with finite, non-zero values, and the gradient that reaches ``dec`` is bit for bit the one computed with ``dec`` detached as a
    leaf: the chain through the new Function adds nothing of its own."""
    r = vqvae_steps
    assert not r["missing"] and r["one"]
    bad = [k for k, g in r["one"].items() if not (bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0)]
    assert not bad, bad
    assert torch.equal(r["g_dec_one"], r["g_dec_two"]) and torch.equal(r["g_dec_two"], r["g_dec_again"])
    assert not torch.equal(r["g_dec_two"], r["g_mse"])                  # the perceptual term is in it
    assert sorted(r["one"]) == sorted(r["two"])


def test_vqvae_parameter_gradients_equal_the_two_stage_bits(vqvae_steps):
    """Every trainable VQ-VAE gradient of the one-call route is torch.equal to the one of the two-stage route (same d / d dec bits, see the test
    above, fed to the same backward).  Bit equality needs the VQ-VAE's own backward to repeat itself: the column sums of its fp32 tail
    (fm_colsum_f32, the dw / db of fm_layernorm_bwd_f32) add the rows in a fixed order, and at this size (32 token rows) every other
    reduction of the step is the work of one workgroup.  Two runs of one route are compared and printed next to the comparison of the routes."""
    r = vqvae_steps
    differ = {k: float((r["one"][k] - r["two"][k]).abs().max() / r["two"][k].abs().max()) for k in r["one"] if not torch.equal(r["one"][k], r["two"][k])}
    rerun = {k: float((r["again"][k] - r["two"][k]).abs().max() / r["two"][k].abs().max()) for k in r["two"] if not torch.equal(r["again"][k], r["two"][k])}
    print(f"vqvae + percept: {len(differ)} of {len(r['one'])} gradients differ between the routes (worst rel {max(differ.values(), default=0):.2e}): {sorted(differ)}")
    print(f"vqvae + percept: {len(rerun)} differ between two runs of the SAME route (worst rel {max(rerun.values(), default=0):.2e}): {sorted(rerun)}")
    for k in r["one"]:
        assert torch.equal(r["one"][k], r["two"][k]), k
