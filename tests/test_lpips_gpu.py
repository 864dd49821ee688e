"""The LPIPS perceptual loss on a real MI355X: loss (B, 1, 1, 1) and d loss.sum() / d preds at the full VGG16 widths against float64 autograd of
tests/lpips_util.py::lpips_ref (upstream's forward, pinned to upstream's own code by tests/test_lpips_cpu.py), at the two fixture cases
(B = 3, 32 x 32 and B = 2, 16 x 48: the last feature maps are 2 x 2 and 1 x 3, so every border and pooling rule is exercised).

fp32 mode: max |a - ref| / max |ref| <= 8 x max(the same distance of lpips_ref evaluated in float32 on the CPU, 2^-24) per tensor - the
           project's fp32 rule (tests/test_clip_percept_gpu.py).  Condition on the inputs, asserted: the float32 CPU run itself stays within
           1e-5 of float64 on the gradient (no ReLU or pool selection flips in the reference's own arithmetic).
bf16 mode: yardstick = lpips_ref on the CPU under torch.autocast("cpu", torch.bfloat16), forward and backward.  Loss: max-norm distance
           <= 2 x the yardstick's.  Gradient: relative L2 distance <= 2 x the yardstick's - a bf16 network with ReLU and max-pool routes
           single gradient entries through other positions than float64 does, so a max-norm bound would be decided by one flipped
           selection.  The factor 2 is the CLIP loss's margin: the engine rounds at other points than autocast, errors of one size, not equal.
           Every ratio, the max-norm one included, goes to the parity log.
Measured on an MI355X: see INTEGRATION.md, "LPIPS perceptual loss"."""
import pytest
import torch
import torch.nn.functional as F

from tests import lpips_util as LU
from tests.parity_log import record

pytestmark = pytest.mark.gpu

DEV = "cuda"
CASES = sorted(LU.CASES)


def make_loss(precision="bf16"):
    from fourm.vq.percept_losses import LpipsPerceptualLoss
    return LpipsPerceptualLoss(LU.seeded_state_dict(), compute_precision=precision).to(DEV)


@pytest.fixture(scope="module")
def refs():
    """Per case: float64 (the reference), float32 and CPU-autocast (the yardsticks) loss and pixel gradient; computed once, never modified."""
    return {case: dict(f64=LU.ref_run(case, torch.float64), f32=LU.ref_run(case, torch.float32), ac=LU.ref_run(case, torch.float32, autocast=True))
            for case in CASES}


@pytest.fixture(scope="module")
def losses():
    return {p: make_loss(p) for p in ("fp32", "bf16")}


def hip_run(loss_mod, case, weights=None, dtype=torch.float32):
    preds, targets = LU.inputs(case)
    p = preds.to(DEV, dtype).requires_grad_()
    loss = loss_mod(p, targets.to(DEV, dtype))
    (loss.sum() if weights is None else (loss.reshape(-1) * weights.to(DEV)).sum()).backward()
    return loss.detach(), p.grad


@pytest.mark.parametrize("case", CASES)
def test_fp32_mode_against_float64(case, refs, losses):
    loss, grad = hip_run(losses["fp32"], case)
    r = refs[case]
    assert loss.dtype == torch.float32 and loss.shape == r["f64"][0].shape == (LU.CASES[case][0], 1, 1, 1) and grad.shape == r["f64"][1].shape
    assert LU.rel_max(r["f32"][1], r["f64"][1]) <= 1e-5          # the yardstick is a rounding-error yardstick: no selection flipped in it
    for name, got, k in (("loss", loss, 0), ("grad", grad, 1)):
        err, own = LU.rel_max(got, r["f64"][k]), LU.rel_max(r["f32"][k], r["f64"][k])
        bound = 8 * max(own, 2.0 ** -24)
        print(f"lpips fp32 {case} {name}: {err:.3e} vs float64 (torch fp32 {own:.3e}, ratio {err / max(own, 2.0 ** -24):.2f}, bound {bound:.3e})")
        record("lpips.fp32", case=case, tensor=name, err=err, torch_fp32_err=own, ratio=err / max(own, 2.0 ** -24))
        assert err <= bound, (case, name, err, bound)


@pytest.mark.parametrize("case", CASES)
def test_bf16_mode_against_float64(case, refs, losses):
    mod = losses["bf16"]
    assert mod.compute_precision == "bf16"
    loss, grad = hip_run(mod, case)
    r = refs[case]
    assert loss.dtype == torch.float32 and grad.dtype == torch.float32 and bool(torch.isfinite(grad).all())
    l_err, l_own = LU.rel_max(loss, r["f64"][0]), LU.rel_max(r["ac"][0], r["f64"][0])
    g_err, g_own = LU.rel_l2(grad, r["f64"][1]), LU.rel_l2(r["ac"][1], r["f64"][1])
    m_err, m_own = LU.rel_max(grad, r["f64"][1]), LU.rel_max(r["ac"][1], r["f64"][1])
    print(f"lpips bf16 {case}: loss {l_err:.3e} (CPU autocast {l_own:.3e}, ratio {l_err / l_own:.2f}); grad L2 {g_err:.3e} (autocast {g_own:.3e}, ratio "
          f"{g_err / g_own:.2f}); grad max-norm {m_err:.3e} (autocast {m_own:.3e}, ratio {m_err / m_own:.2f}); bound 2")
    record("lpips.bf16", case=case, loss_err=l_err, loss_autocast_err=l_own, loss_ratio=l_err / l_own, grad_l2_err=g_err, grad_l2_autocast_err=g_own,
           grad_l2_ratio=g_err / g_own, grad_max_err=m_err, grad_max_autocast_err=m_own, grad_max_ratio=m_err / m_own)
    assert l_err <= 2 * l_own, (case, "loss", l_err, l_own)
    assert g_err <= 2 * g_own, (case, "grad", g_err, g_own)


def test_non_uniform_incoming_gradient_scales_per_sample(losses):
    """(loss * w).sum() with a random w that contains a negative entry: sample b's pixel gradient is w[b] times its gradient under
    loss.sum() - checked against float64 in fp32 mode by the rule above."""
    case = "b3_32x32"
    w = torch.randn(3, generator=torch.Generator().manual_seed(9)).abs() + 0.25
    w[1] = -w[1]
    _, grad = hip_run(losses["fp32"], case, weights=w)
    ref = LU.ref_run(case, torch.float64, weights=w)[1]
    own = LU.ref_run(case, torch.float32, weights=w)[1]
    err, bound = LU.rel_max(grad, ref), 8 * max(LU.rel_max(own, ref), 2.0 ** -24)
    assert err <= bound, (err, bound)


def test_targets_get_no_gradient_and_no_grad_saves_nothing(losses):
    mod = losses["bf16"]
    preds, targets = LU.inputs("b2_16x48")
    p, t = preds.to(DEV).requires_grad_(), targets.to(DEV).requires_grad_()
    loss = mod(p, t)
    assert loss.grad_fn is not None and loss.shape == (2, 1, 1, 1)
    loss.sum().backward()
    assert t.grad is None and p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0
    gen_before = mod._gen
    with torch.no_grad():
        quiet = mod(p, t)
    assert quiet.grad_fn is None and not quiet.requires_grad and torch.equal(quiet, loss.detach())
    plain = mod(preds.to(DEV), t)                                       # preds that ask for no gradient: no graph either
    assert plain.grad_fn is None and torch.equal(plain, loss.detach())
    assert mod._gen == gen_before                                       # neither pass registered a state awaiting a backward
    assert not any(q.grad is not None for q in mod.parameters())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_half_precision_inputs_are_accepted(dtype, losses):
    loss, grad = hip_run(losses["bf16"], "b2_16x48", dtype=dtype)
    assert loss.dtype == torch.float32 and grad.dtype == dtype and bool(torch.isfinite(loss).all()) and bool(torch.isfinite(grad.float()).all())
    preds, targets = LU.inputs("b2_16x48")
    same = losses["bf16"](preds.to(DEV, dtype).float(), targets.to(DEV, dtype).float())          # the cast to fp32 in front is all that differs
    assert torch.equal(loss, same)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_two_identical_runs_give_identical_bits(precision, losses):
    l1, g1 = hip_run(losses[precision], "b3_32x32")
    l2, g2 = hip_run(losses[precision], "b3_32x32")
    assert torch.equal(l1, l2) and torch.equal(g1, g2)


def test_backward_after_a_newer_forward_raises(losses):
    mod = losses["bf16"]
    preds, targets = LU.inputs("b2_16x48")
    p, t = preds.to(DEV).requires_grad_(), targets.to(DEV)
    first = mod(p, t)
    second = mod(p, t)
    with pytest.raises(RuntimeError, match="most recent training forward only"):
        first.sum().backward()
    second.sum().backward()                                             # the newer one is intact
    assert p.grad is not None and bool(torch.isfinite(p.grad).all())
    ref_grad = p.grad.clone()
    p.grad = None
    third = mod(p, t)
    with torch.no_grad():                                               # a pass that keeps no state does not disturb one that does
        mod(p * 0.5, t)
    third.sum().backward()
    assert torch.equal(third, second) and torch.equal(p.grad, ref_grad)


@pytest.fixture(scope="module")
def vqvae_steps(losses):
    """The micro VQ-VAE of tests/test_clip_percept_gpu.py::vqvae_steps (image 32, patch 8) with the LPIPS loss behind it.  Route "one":
    (mse + 0.5 lpips.mean()).backward().  Route "two": the same scalar with dec detached as a leaf."""
    from fourm.vq import VQVAE
    torch.manual_seed(0)
    m = VQVAE(dec_type="vit_s_dec", image_size=32, enc_type="vit_s_enc", patch_size=8, post_mlp=True, codebook_size=64, latent_dim=32,
              norm_codes=True, sync_codebook=False, threshold_ema_dead_code=0).cuda().train()
    m.quantize.eval()
    percept = losses["bf16"]
    x = torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(1)).clamp(-1, 1).cuda()

    def objective(dec):
        return F.mse_loss(dec, x) + 0.5 * percept(dec, x).mean()

    res = {}
    dec, _ = m(x)
    dec.register_hook(lambda g: res.__setitem__("g_dec_one", g.clone()))
    objective(dec).backward()
    res["missing"] = [k for k, p in m.named_parameters() if p.requires_grad and p.grad is None]
    res["one"] = {k: p.grad.clone() for k, p in m.named_parameters() if p.requires_grad and p.grad is not None}
    m.zero_grad(set_to_none=True)
    dec, _ = m(x)
    leaf = dec.detach().requires_grad_()
    objective(leaf).backward()
    res["g_dec_two"] = leaf.grad.clone()
    res["g_mse"] = torch.autograd.grad(F.mse_loss(leaf, x), leaf)[0]
    return res


def test_vqvae_training_step_with_the_lpips_term(vqvae_steps):
    """(mse + 0.5 lpips(dec, x).mean()).backward() through the VQ-VAE's own hand-written backward fills every trainable gradient with finite,
    non-zero values, and the gradient that reaches ``dec`` is bit for bit the one computed with ``dec`` detached as a leaf."""
    r = vqvae_steps
    assert not r["missing"] and r["one"]
    bad = [k for k, g in r["one"].items() if not (bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0)]
    assert not bad, bad
    assert torch.equal(r["g_dec_one"], r["g_dec_two"])
    assert not torch.equal(r["g_dec_two"], r["g_mse"])                  # the perceptual term is in it
