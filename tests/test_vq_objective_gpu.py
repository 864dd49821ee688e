"""The tokenizer training objective on a real MI355X (fourm.vq.training, fourm.vq.vq_utils, csrc/train_objective.hip): the seven
reconstruction losses and every gradient element against float64 torch on the CPU within bounds derived from the formats
(tests/vq_objective_util.py), the bit-exact pieces (mask_out_samples, ModelEma.update, diffusion_training_pair) with torch.equal against the
torch expressions evaluated on the CPU, compute_codebook_usage against the host count, and one end-to-end training step of the smallest VQVAE."""
import math

import numpy as np
import pytest
import torch
from torch import nn

from tests import vq_objective_util as R
from tests.parity_log import record

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = 7.0


def _T():
    from fourm.vq import training
    return training


def run_public(loss_fn, x, t, scale=None):
    """compute_reconst_loss through autograd on the device -> (loss, d / d model_output) as device tensors."""
    xd = x.to(DEV).requires_grad_(True)
    loss = _T().compute_reconst_loss(xd, t.to(DEV), loss_fn)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.requires_grad
    (loss if scale is None else loss * scale).backward()
    return loss.detach(), xd.grad


def run_padded(loss_fn, x, t, offset):
    """fm_reconst_loss writing its gradient into the middle of a sentinel buffer (offset 32: 16-byte aligned, 33: the scalar accesses)."""
    from fourm.hip import _lib as L, ops
    mode = {"mse": L.LOSS_MSE, "l1": L.LOSS_L1, "smooth_l1": L.LOSS_SMOOTH_L1, "cross_entropy": L.LOSS_CE_INDEX, "binary_cross_entropy": L.LOSS_BCE,
            "cosine": L.LOSS_COSINE, "cosine_1d": L.LOSS_COSINE_1D}[loss_fn]
    n = x.numel()
    buf = torch.full((n + 96,), SENT, device=DEV)
    grad = buf[offset:offset + n].view(x.shape)
    loss = ops.reconst_loss(x.to(DEV), t.to(DEV), mode, grad)
    assert bool((buf[:offset] == SENT).all()) and bool((buf[offset + n:] == SENT).all()), f"{loss_fn}: wrote outside its gradient"
    return loss.reshape(()), grad


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("loss_fn", R.LOSS_FNS)
def test_reconst_loss_and_gradient_against_float64(loss_fn, shape):
    """Loss value and every gradient element of a mode against upstream's expression in float64 (torch's F.* functions and autograd on the CPU,
    same fp32 inputs).  Bounds (tests/vq_objective_util.py::bounds, all from float64 quantities, doubled for second-order terms; D = the depth
    of the fixed-order sum, 40 + workgroups / 256):
      mse        term 3 U d^2 (d = x - t rounds once, the square once);        gradient 4 U |g|
      l1         term U |d|;                                                   gradient 2 U / n, exactly 0 where x == t
      smooth_l1  term 3 U (term + |d|);                                        gradient 4 U |g| + U / n (rounding may move |d| across 1)
      loss = sum / n: mean term error + D U mean |term| + 3 U |loss|
      cross_entropy  the bound of tests/test_fp32_kernels_gpu.py::test_cross_entropy_f32 with K sequential terms: E_lse = 2 (sum e (|t| + 3) U /
                 sum e + (K + 10) U + 2 U |log S| + 2 U |lse|); pixel loss E_lse + U |loss|; gradient (p (E_lse + (|x - lse| + 3) U) + U |p - 1hot|)
                 / count + 4 U |g| + 2^-126
      binary_cross_entropy  sigmoid and 1 - sigmoid to 6 U absolute; exp of them to 9 U relative; E_lse = (9 + 2 C) U + 3 U |lse|; pixel loss
                 C E_lse + E_A + 2 U (C |lse| + |A|); gradient chained through p_k = exp(z_k - lse), C p_k - q_k, both occurrences of s, s (1 - s)
      cosine / cosine_1d  E_cos = (L + 8) U (sum |x t| / (|x| |t|) + |cos|) + 6 U |cos| over a reduced axis of length L; the gradient
                 (b x - a t) / R from it.  One row of model_output is all zero: its loss term is checked (cos = 0), its gradient is not;
                 gradients are compared on rows of norm >= 1e-3 (all others here).
    Also: a second call returns the same bits; a non-unit incoming gradient scales the gradient by exactly that fp32 factor; the sentinels
    around a gradient written into the middle of a larger buffer are intact, on the 16-byte and on the scalar access path, same bits."""
    x, t = R.make_inputs(loss_fn, shape, seed=100 + len(loss_fn) + shape[1])
    ref_loss, ref_grad = R.reference(x, t, loss_fn)
    loss_tol, grad_tol, live = R.bounds(x, t, loss_fn)
    loss, grad = run_public(loss_fn, x, t)
    err = abs(float(loss.double().cpu()) - float(ref_loss))
    worst_g = R.within(f"{loss_fn} gradient", grad, ref_grad, grad_tol, live)
    record(f"vq_objective.reconst_loss.{loss_fn}", shape=list(shape), loss=float(loss), loss_err=err, loss_tol=float(loss_tol), grad_worst_err_over_tol=worst_g)
    assert err <= float(loss_tol), (loss_fn, float(loss), float(ref_loss), err, float(loss_tol))
    assert bool(torch.isfinite(grad).all())
    if loss_fn in ("l1", "smooth_l1"):
        same = (x == t).to(DEV)
        assert int(same.sum()) > 0 and bool((grad[same] == 0).all())
    # determinism
    loss2, grad2 = run_public(loss_fn, x, t)
    assert torch.equal(loss, loss2) and torch.equal(grad, grad2)
    # a non-unit incoming gradient
    s = 0.37
    loss3, grad3 = run_public(loss_fn, x, t, scale=s)
    assert torch.equal(loss3, loss) and torch.equal(grad3, grad * torch.tensor(s, dtype=torch.float32, device=DEV))
    # sentinels, both access paths
    for off in (32, 33):
        lp, gp = run_padded(loss_fn, x, t, off)
        assert torch.equal(lp, loss) and torch.equal(gp, grad), (loss_fn, off)


def test_cross_entropy_ignored_and_out_of_range_labels():
    """Index cross-entropy, K = 37: pixels labelled -100 drop out of the mean and get a zero gradient (float64 reference, the bound of the
    test above); an all-ignored input gives nan as torch does; a label outside [0, K) gives a NaN loss and is never used as an index."""
    T = _T()
    K, shape = 37, (2, 37, 7, 9)
    x, t = R.make_inputs("cross_entropy", shape, seed=7)
    g = R.gen(8)
    t[torch.rand(t.shape, generator=g) < 0.3] = -100
    assert 0 < int((t == -100).sum()) < t.numel()
    ref_loss, ref_grad = R.reference(x, t, "cross_entropy")
    loss_tol, grad_tol, _ = R.bounds(x, t, "cross_entropy")
    loss, grad = run_public("cross_entropy", x, t)
    assert abs(float(loss) - float(ref_loss)) <= float(loss_tol)
    R.within("ce gradient with ignored pixels", grad, ref_grad, grad_tol)
    ign = (t == -100).unsqueeze(1).expand(shape).to(DEV)
    assert bool((grad[ign] == 0).all())
    # all ignored
    ta = torch.full_like(t, -100)
    assert math.isnan(float(R.reference(x, ta, "cross_entropy")[0]))
    la, ga = run_public("cross_entropy", x, ta)
    assert math.isnan(float(la)) and bool((ga == 0).all())
    # one label out of range (K and a large one): NaN, and the device is still healthy afterwards
    for bad in (K, 2 ** 40, -5):
        tb = t.clone()
        tb[1, 3, 4] = bad
        lb = T.compute_reconst_loss(x.to(DEV), tb.to(DEV), "cross_entropy")
        torch.cuda.synchronize()
        assert math.isnan(float(lb))
    assert float(run_public("cross_entropy", x, t)[0]) == float(loss)


@pytest.mark.parametrize("C", [1, 3])
def test_binary_cross_entropy_gradient_carries_sum_q(C):
    """upstream's binary_cross_entropy applies a softmax to the 2 C probabilities [s, 1 - s] with targets [t, 1 - t] that add up to C, not 1:
    d / d z_k = (C p_k - q_k) / N.  torch's autograd reference equals that closed form (sum_q = C) and, for C = 3, is far from the sum_q = 1
    form; the kernel agrees with the former within the bound of the test above."""
    shape = (2, C, 8, 8)
    x, t = R.make_inputs("binary_cross_entropy", shape, seed=40 + C)
    ref_loss, ref_grad = R.reference(x, t, "binary_cross_entropy")
    closed = R.bce_closed_form(x, t, sum_q=C)
    assert float((ref_grad - closed).abs().max()) <= 1e-14
    loss_tol, grad_tol, _ = R.bounds(x, t, "binary_cross_entropy")
    if C > 1:
        naive = R.bce_closed_form(x, t, sum_q=1)
        assert float(((naive - closed).abs() > 100 * grad_tol).double().mean()) > 0.9          # the bound tells the two apart almost everywhere
    loss, grad = run_public("binary_cross_entropy", x, t)
    assert abs(float(loss) - float(ref_loss)) <= float(loss_tol)
    R.within(f"bce gradient C={C}", grad, closed, grad_tol)


# ---- bit-exact pieces -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 3, 8, 8), (3, 5, 7, 9), (2, 1, 33, 31)], ids=lambda s: "x".join(map(str, s)))
def test_mask_out_samples_bit_exact(shape):
    T = _T()
    g = R.gen(5)
    B, C, H, W = shape
    clean = torch.randn(shape, generator=g)
    valid = torch.rand(B, 1, H, W, generator=g) > 0.4
    value = -0.3
    want_clean = clean.clone()
    want_clean[~valid.expand(B, C, H, W)] = value                                        # upstream's indexing assignment, on the CPU
    want = torch.cat([want_clean, valid.float() * 2 - 1], dim=1)
    dev_clean = clean.to(DEV)
    out = T.mask_out_samples(dev_clean, valid, mask_value=value)                          # (the mask may arrive on the CPU, as the loaders deliver it)
    assert out.shape == (B, C + 1, H, W) and torch.equal(out.cpu(), want)
    assert torch.equal(dev_clean.cpu(), want_clean)                                       # overwritten in place
    untouched = clean.to(DEV)
    assert T.mask_out_samples(untouched, valid.to(DEV), None) is untouched and torch.equal(untouched.cpu(), clean)
    # a non-contiguous input is still overwritten in place
    wide = torch.randn(B, C, H, W + 3, generator=g).to(DEV)
    view = wide[..., :W]
    ref_view = view.cpu().clone()
    ref_view[~valid.expand(B, C, H, W)] = value
    out2 = T.mask_out_samples(view, valid.to(DEV), value)
    assert torch.equal(view.cpu(), ref_view) and torch.equal(out2[:, :C].cpu(), ref_view)


class _Mixed(nn.Module):
    """A state dict of mixed sizes: 1, 3, 4097 and 315 000 fp32 elements, an fp32 buffer and an int64 buffer."""

    def __init__(self):
        super().__init__()
        g = R.gen(11)
        self.one = nn.Parameter(torch.randn(1, generator=g))
        self.three = nn.Parameter(torch.randn(3, generator=g))
        self.odd = nn.Parameter(torch.randn(4097, generator=g))
        self.big = nn.Parameter(torch.randn(700, 450, generator=g))
        self.register_buffer("stat", torch.randn(17, generator=g))
        self.register_buffer("steps", torch.tensor(5, dtype=torch.int64))


@pytest.mark.parametrize("decay", [0.9999, 0.8, 0.999])
def test_model_ema_update_bit_exact(decay):
    """ModelEma.update on the device against upstream's expression ema * decay + (1 - decay) * model evaluated by torch on the CPU, entry by
    entry, over two consecutive updates; the int64 buffer follows upstream's expression too (torch's path)."""
    T = _T()
    from fourm.hip import engine as hip_engine
    model = _Mixed().to(DEV)
    ema = T.ModelEma(model, decay=decay)
    g = R.gen(12)
    for step in range(2):
        with torch.no_grad():
            for p in model.parameters():
                p.add_(torch.randn(p.shape, generator=g).to(DEV))
            model.stat.mul_(1.5)
            model.steps.add_(4)
        cpu_ema = {k: v.cpu().clone() for k, v in ema.ema.state_dict().items()}
        cpu_model = {k: v.cpu() for k, v in model.state_dict().items()}
        want = {k: (v * decay + (1. - decay) * cpu_model[k]).to(v.dtype) for k, v in cpu_ema.items()}
        epoch, table = hip_engine._WEIGHT_EPOCH, ema._jobs
        ema.update(model)
        assert hip_engine._WEIGHT_EPOCH == epoch + 1
        assert step == 0 or ema._jobs is table                                             # the job list is built once
        for k, v in ema.ema.state_dict().items():
            assert v.dtype == want[k].dtype and torch.equal(v.cpu(), want[k]), (k, step, decay)
        for k, v in model.state_dict().items():
            assert torch.equal(v.cpu(), cpu_model[k]), k                                   # the model is only read
    assert ema._jobs[2] == 5                                                               # the five fp32 entries in one launch; the int64 buffer on torch
    # a parameter re-allocated (a new data pointer): the job list is rebuilt
    model.three.data = model.three.data.clone()
    want = (ema.ema.three.cpu() * decay + (1. - decay) * model.three.detach().cpu())
    ema.update(model)
    assert ema._jobs is not table and torch.equal(ema.ema.three.cpu(), want)


@pytest.mark.parametrize("shape", [(4, 3, 8, 8), (5, 3, 7, 9)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("sched", ["ddpm", "ddim"])
def test_diffusion_training_pair_bit_exact(sched, shape):
    """(noisy, target) against scheduler.add_noise / get_velocity evaluated on the CPU (and on the device) for per-sample timesteps including 0
    and the last; 'sample' and 'epsilon' hand back clean / noise themselves."""
    T = _T()
    from fourm.vq.scheduling import DDIMScheduler, DDPMScheduler
    s = (DDPMScheduler if sched == "ddpm" else DDIMScheduler)(num_train_timesteps=1000, beta_schedule="squaredcos_cap_v2", prediction_type="v_prediction")
    g = R.gen(21)
    clean, noise = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    ts = torch.tensor([0, 999, 500, 1, 37][:shape[0]])
    want_noisy, want_v = s.add_noise(clean, noise, ts), s.get_velocity(clean, noise, ts)
    c, z = clean.to(DEV), noise.to(DEV)
    noisy, target = T.diffusion_training_pair(s, c, z, ts, "v_prediction")
    assert torch.equal(noisy.cpu(), want_noisy) and torch.equal(target.cpu(), want_v)
    assert torch.equal(noisy, s.add_noise(c, z, ts.to(DEV))) and torch.equal(target, s.get_velocity(c, z, ts.to(DEV)))
    n2, t2 = T.diffusion_training_pair(s, c, z, ts.to(DEV), "sample")
    assert torch.equal(n2, noisy) and t2 is c
    for pt in ("epsilon", "v_prediction-epsilon_loss"):
        n3, t3 = T.diffusion_training_pair(s, c, z, ts, pt)
        assert torch.equal(n3, noisy) and t3 is z
    # a timestep outside the schedule is not used as an index
    n4, _ = T.diffusion_training_pair(s, c, z, torch.tensor([0, 1000, 5, -1, 2][:shape[0]]), "epsilon")
    torch.cuda.synchronize()
    assert bool(torch.isnan(n4[1]).all()) and torch.equal(n4[0], noisy[0])


# ---- codebook usage -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,window", [(64, 100), (16384, 20000)])
@pytest.mark.parametrize("dtype", [torch.int64, torch.int32, torch.int16])
def test_codebook_usage_on_device(dtype, K, window):
    """Several windows plus a ragged tail that is dropped; one window uses every code, one a single code; equal to the host count of the same
    function and to numpy.unique; a token outside [0, K) raises."""
    from fourm.vq.vq_utils import compute_codebook_usage
    g = R.gen(31)
    every = torch.arange(window) % K
    tokens = torch.cat([torch.randint(0, K, (window,), generator=g), every[torch.randperm(window, generator=g)], torch.full((window,), K - 1),
                        torch.randint(0, max(K // 9, 2), (window,), generator=g), torch.randint(0, K, (window // 3,), generator=g)]).to(dtype)
    a = tokens.numpy()
    per_window = [len(np.unique(a[i * window:(i + 1) * window])) for i in range(4)]
    assert per_window[1] == K and per_window[2] == 1
    want = float(np.mean([c / K for c in per_window]))
    got = compute_codebook_usage(tokens.to(DEV), codebook_size=K, window_size=window)
    assert isinstance(got, float) and got == want == compute_codebook_usage(tokens, codebook_size=K, window_size=window)
    assert got == compute_codebook_usage(tokens.to(DEV), codebook_size=K, window_size=window)
    assert math.isnan(compute_codebook_usage(tokens[:window - 1].to(DEV), codebook_size=K, window_size=window))
    for bad in (K, -1):
        tb = tokens.clone()
        tb[window + 5] = bad
        with pytest.raises(ValueError, match="outside"):
            compute_codebook_usage(tb.to(DEV), codebook_size=K, window_size=window)
    assert compute_codebook_usage(tokens.to(DEV), codebook_size=K, window_size=window) == want        # the flag is cleared by the next call


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------
def test_training_step_with_ema_end_to_end():
    """One tokenizer training step on the smallest VQVAE tests/test_vqvae.py trains: (compute_reconst_loss(dec, x, 'mse') + code_loss).backward()
    leaves finite gradients on every trainable parameter, bit-identical across two runs; the gradient that reaches ``dec`` is the stand-alone
    loss's; after FusedAdamW.step() and ema.update(model) the EMA copy evaluates exactly as a fresh model loaded from its state_dict (its
    cached weight images were refreshed) and the model's own output is untouched."""
    T = _T()
    from fourm.utils.optim_factory import FusedAdamW
    from tests.test_vqvae import build, case
    c, cfg, sd, x, _ = case("vqvae_small")
    xg = x.to(DEV)

    def step():
        m = build(c, cfg)
        m.load_state_dict(sd, strict=True)
        m = m.to(DEV).train()
        dec, code_loss = m(xg)
        dec.retain_grad()
        (T.compute_reconst_loss(dec, xg, "mse") + code_loss).backward()
        return m, dec

    m, dec = step()
    m2, _ = step()
    trainable = [(k, p) for k, p in m.named_parameters() if p.requires_grad]
    assert len(trainable) > 10
    for (k, p), (_, p2) in zip(trainable, [(k, p) for k, p in m2.named_parameters() if p.requires_grad]):
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
        assert torch.equal(p.grad, p2.grad), k
    alone = dec.detach().clone().requires_grad_(True)
    T.compute_reconst_loss(alone, xg, "mse").backward()
    assert torch.equal(dec.grad, alone.grad)
    ref_loss, ref_grad = R.reference(dec.detach().cpu(), x, "mse")
    R.within("d loss / d dec", dec.grad, ref_grad, R.bounds(dec.detach().cpu(), x, "mse")[1])

    ema = T.ModelEma(m, decay=0.5)
    import copy
    assert m.encoder.__dict__.get("_hip_engine") is not None and m.decoder.__dict__.get("_hip_engine") is not None
    for twin in (ema.ema, copy.deepcopy(m)):                                              # a copy does not inherit the model's engine state
        assert twin.encoder.__dict__.get("_hip_engine") is None and twin.decoder.__dict__.get("_hip_engine") is None
    with torch.no_grad():
        before = ema.ema(xg)[0].clone()                                                   # fills the copy's cached weight images
    opt = FusedAdamW([p for _, p in trainable], lr=1e-2)
    opt.step()
    m.eval()
    with torch.no_grad():
        own = m(xg)[0].clone()
    ema.update(m)
    with torch.no_grad():
        own_after = m(xg)[0]
        got = ema.ema(xg)[0]
    assert torch.equal(own, own_after)
    fresh = build(c, cfg)
    fresh.load_state_dict({k: v.cpu() for k, v in ema.ema.state_dict().items()}, strict=True)
    fresh = fresh.to(DEV).eval()
    with torch.no_grad():
        want = fresh(xg)[0]
    assert torch.equal(got, want)
    assert not torch.equal(got, before)
    for k, v in ema.ema.state_dict().items():
        if v.dtype == torch.float32 and k in dict(trainable):
            assert torch.equal(v, (sd[k].to(DEV) * 0.5 + (1. - 0.5) * m.state_dict()[k])), k


def test_model_ema_update_time_on_vit_b_tokenizer():
    """Reported, not asserted: wall time of ModelEma.update (one launch) on a ViT-B / ViT-B VQVAE against upstream's per-tensor loop (four small
    torch kernels per state-dict entry) on the same tensors in the same process.  Asserted: both leave the same bits."""
    import time
    T = _T()
    from fourm.vq import VQVAE
    model = VQVAE(dec_type="vit_b_dec", image_size=224, enc_type="vit_b_enc", patch_size=16, codebook_size=4096, latent_dim=32, sync_codebook=False).to(DEV)
    ema = T.ModelEma(model, decay=0.9999)
    loop_ema = {k: v.clone() for k, v in ema.ema.state_dict().items()}
    msd = {k: v.detach() for k, v in model.state_dict().items()}

    def loop():
        with torch.no_grad():
            for k, ema_v in loop_ema.items():
                ema_v.copy_(ema_v * 0.9999 + (1. - 0.9999) * msd[k])

    def timed(fn, windows=3, calls=10):
        """seconds per call: the best of ``windows`` host-clock windows of ``calls`` back-to-back calls, each ended by a device synchronise"""
        best = float("inf")
        for _ in range(windows):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
            best = min(best, (time.perf_counter() - t0) / calls)
        return best

    ema.update(model)
    loop()                                                                                 # (both once: job list built, allocator warm)
    for k, v in ema.ema.state_dict().items():
        assert torch.equal(v, loop_ema[k]), k
    t_fused, t_loop = timed(lambda: ema.update(model)), timed(loop)
    from fourm.hip import ops
    _, table, n_jobs, chunks, _ = ema._jobs
    t_launch = timed(lambda: ops.ema_update(table, n_jobs, chunks, 0.9999))                 # the launch alone, without walking the two state dicts
    n = sum(v.numel() for v in loop_ema.values())
    record("vq_objective.model_ema_update_time", entries=len(loop_ema), elements=n, fused_ms=1e3 * t_fused, per_tensor_loop_ms=1e3 * t_loop,
           launch_only_ms=1e3 * t_launch, fused_jobs=n_jobs, device=torch.cuda.get_device_name())
