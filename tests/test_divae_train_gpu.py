"""Training the DiVAE decoder on a frozen encoder (compute_precision = "fp32") on a real MI355X: every parameter gradient of the conditional
UNet against float64 autograd of tests/divae_f64_util.unet_forward under the rule of tests/divae_train_util.py, torch's .grad semantics, two
live graphs, and DiVAE.forward with freeze_enc=True."""
import os
import sys
import time

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ml-4m_amd"))
from tests import divae_train_util as TU  # noqa: E402
from tests.parity_log import record  # noqa: E402

pytestmark = pytest.mark.gpu


def make_net(cfg_name):
    from fourm.vq.models.unet import PatchedUNetCondCat
    net = PatchedUNetCondCat(**TU.CONFIGS[cfg_name][0])
    net.load_state_dict(TU.state_dict(cfg_name), strict=True)
    net = net.cuda().train()
    net.compute_precision = "fp32"
    return net


def loss_of(net, evals):
    """sum of F.mse_loss(net(...), target) over the evaluations: every graph is alive until the one backward"""
    return sum(F.mse_loss(net(x.cuda(), t.cuda(), c.cuda(), cond_mask=None if m is None else m.cuda()), tgt.cuda()) for x, t, c, m, tgt in evals)


def grads_of(net):
    return {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in net.named_parameters()}


@pytest.mark.parametrize("name", ["small", "small_masked"])
def test_small_gradients_against_float64(name):
    """The configuration, seed-3 weights and inputs of tests/golden/divae_small.npz (B = 3, per-sample timesteps), with and without the
    conditioning mask: all 128 parameter gradients under the rule; the train-mode forward is the eval-mode fp32 forward, bit for bit."""
    cfg_name, evals = TU.case(name)
    net = make_net(cfg_name)
    x, t, c, m, tgt = evals[0]
    args = (x.cuda(), t.cuda(), c.cuda())
    mask = None if m is None else m.cuda()
    out = net(*args, cond_mask=mask)
    assert out.requires_grad and out.grad_fn is not None and out.dtype == torch.float32
    F.mse_loss(out, tgt.cuda()).backward()                         # (warm-up: kernels loaded, scratch sized)
    net.zero_grad()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = net(*args, cond_mask=mask)
    F.mse_loss(out, tgt.cuda()).backward()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    print(f"{name}: one forward + backward {ms:.1f} ms wall (reported, not asserted)")
    record("divae.fp32.grad", case=name, tensor="(wall time of one forward + backward, ms)", ms=ms)
    got = grads_of(net)
    assert len(got) == 128 and all(g is not None for g in got.values())
    TU.under_the_rule(name, got)
    net.eval()
    with torch.no_grad():
        ev = net(*args, cond_mask=mask)
    assert ev.grad_fn is None and torch.equal(ev, out.detach())
    net.train()
    with torch.no_grad():
        assert net(*args, cond_mask=mask).grad_fn is None          # training mode without gradients: the plain evaluation
    with pytest.raises(NotImplementedError, match="frozen-encoder scope"):
        net(args[0].clone().requires_grad_(True), args[1], args[2])
    with pytest.raises(NotImplementedError, match="frozen-encoder scope"):
        net(args[0], args[1], args[2].clone().requires_grad_(True))


def test_mid_gradients_against_float64():
    """Three Downs and three Ups, attention on 16 and on 4 tokens in both halves, two blocks per level on the skip stack: all 334 under the rule."""
    cfg_name, evals = TU.case("mid")
    net = make_net(cfg_name)
    loss_of(net, evals).backward()
    got = grads_of(net)
    assert len(got) == 334 and all(g is not None for g in got.values())
    TU.under_the_rule("mid", got)


def test_torch_semantics_of_the_gradients():
    """A second backward without zero_grad doubles .grad; after zero_grad the first value comes back bit for bit; frozen parameters get None
    and leave every other gradient unchanged, bit for bit."""
    cfg_name, evals = TU.case("small")
    net = make_net(cfg_name)
    loss_of(net, evals).backward()
    first = grads_of(net)
    loss_of(net, evals).backward()
    assert all(torch.equal(g, 2 * first[k]) for k, g in grads_of(net).items())
    net.zero_grad()
    loss_of(net, evals).backward()
    assert all(torch.equal(g, first[k]) for k, g in grads_of(net).items())
    for k, p in net.named_parameters():
        assert p.grad.shape == p.shape and p.grad.is_contiguous() and p.grad.dtype == p.dtype, k
    frozen = [k for k, _ in net.named_parameters() if k.startswith("time_embed.") or k.startswith("input_blocks.1.0.in_layers.2.")]
    assert len(frozen) == 6
    for k, p in net.named_parameters():
        p.requires_grad_(k not in frozen)
    net.zero_grad()
    loss_of(net, evals).backward()
    for k, g in grads_of(net).items():
        assert (g is None) if k in frozen else torch.equal(g, first[k]), k
    # both optimizers of the project step on these gradients
    from fourm.utils.optim_factory import FusedAdamW
    for opt in (torch.optim.AdamW([p for p in net.parameters() if p.requires_grad], lr=1e-3), FusedAdamW([p for p in net.parameters() if p.requires_grad], lr=1e-3)):
        before = {k: p.detach().clone() for k, p in net.named_parameters()}
        opt.step()
        for k, p in net.named_parameters():
            assert torch.equal(p, before[k]) == (k in frozen), k
    net.zero_grad()
    loss_of(net, evals).backward()                                # the weight images follow the stepped parameters
    assert all(bool(torch.isfinite(g).all()) for g in grads_of(net).values() if g is not None)


def test_two_live_graphs():
    """loss(net(x1)) + loss(net(x2)) with one backward: the sum of the two separate gradients, under the rule against float64."""
    cfg_name, evals = TU.case("small_two")
    net = make_net(cfg_name)
    loss_of(net, evals).backward()
    both = grads_of(net)
    TU.under_the_rule("small_two", both)
    net.zero_grad()
    for e in evals:                                               # and the same as one graph at a time (the order of the additions may differ)
        loss_of(net, [e]).backward()
    apart = grads_of(net)
    TU.under_the_rule("small_two (one at a time)", apart, ref_case="small_two")


def make_divae(**kw):
    from fourm.vq import DiVAE
    torch.manual_seed(0)
    m = DiVAE(image_size=64, n_channels=3, enc_type="vit_s_enc", patch_size=16, codebook_size=256, latent_dim=16, post_mlp=True, norm_codes=True,
              scheduler="ddim", prediction_type="sample", beta_schedule="linear", sync_codebook=False, **kw)
    for p in m.decoder.parameters():
        if float(p.detach().abs().max()) == 0:
            torch.nn.init.normal_(p, std=0.02)
    return m.cuda()


def test_divae_trains_its_decoder_on_a_frozen_encoder():
    m = make_divae(freeze_enc=True).train()
    m.compute_precision = "fp32"
    g = torch.Generator().manual_seed(1)
    x = (torch.rand(3, 3, 64, 64, generator=g) * 2 - 1).cuda()
    noised, target = torch.randn(3, 3, 64, 64, generator=g).cuda(), torch.randn(3, 3, 64, 64, generator=g).cuda()
    ts = torch.tensor([601, 20, 999], device="cuda")
    buffers = {k: b.detach().clone() for k, b in m.named_buffers()}
    params = {k: p.detach().clone() for k, p in m.named_parameters()}
    dec, code_loss = m(x, noised, ts)
    assert dec.requires_grad and dec.dtype == torch.float32 and float(code_loss) == 0.0
    F.mse_loss(dec, target).backward()
    for k, p in m.named_parameters():
        assert (p.grad is not None) == k.startswith("decoder."), k
    assert all(torch.equal(b, buffers[k]) for k, b in m.named_buffers())          # no EMA update: the codebook keeps its bits
    via_model = {k: p.grad.clone() for k, p in m.decoder.named_parameters()}
    with torch.no_grad():
        m.eval()
        quant = m.encode(x)[0]
        m.train()
    m.zero_grad()
    F.mse_loss(m.decoder(noised, ts, quant), target).backward()
    assert all(torch.equal(p.grad, via_model[k]) for k, p in m.decoder.named_parameters())
    torch.optim.AdamW([p for p in m.parameters() if p.requires_grad], lr=1e-3).step()
    for k, p in m.named_parameters():
        assert torch.equal(p, params[k]) == (not k.startswith("decoder.")), k
    assert all(torch.equal(b, buffers[k]) for k, b in m.named_buffers())
    with torch.no_grad():
        out, _ = m(x, noised, ts)
    assert out.grad_fn is None and not out.requires_grad
    m.compute_precision = "bf16"
    with pytest.raises(NotImplementedError, match='compute_precision = "fp32" and freeze_enc=True'):
        m(x, noised, ts)
    m2 = make_divae().train()
    m2.compute_precision = "fp32"
    with pytest.raises(NotImplementedError, match='compute_precision = "fp32" and freeze_enc=True'):
        m2(x, noised, ts)
