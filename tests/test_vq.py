"""VQ tokenizer front end: the CPU oracle against the upstream fixtures (anywhere), the state_dict
layout of ``fourm.vq.VQ``, and — on the GPU — exact code assignment given identical latents plus the
end-to-end token agreement of the bf16 ViT pipeline."""
import os

import numpy as np
import pytest
import torch

from oracle import vq_oracle as V
from tests.golden.cases import VQ_CASES

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def case(name):
    c = VQ_CASES[name]
    cfg = V.vq_cfg(c["enc_type"], image=c["image"], patch=c["patch"], codebook=c["codebook"], post_mlp=c["post_mlp"])
    return c, cfg, V.seeded_vq_state_dict(cfg, seed=c["seed"]), V.synthetic_images(cfg, c["batch"], seed=c["seed"]), \
        np.load(os.path.join(GOLD, f"{name}.npz"))


def build(c, cfg):
    from fourm.vq import VQ
    return VQ(image_size=cfg.image, enc_type=c["enc_type"], patch_size=cfg.patch, post_mlp=cfg.post_mlp, codebook_size=cfg.codebook,
              latent_dim=cfg.latent, norm_codes=True, sync_codebook=False)


@pytest.mark.parametrize("name", list(VQ_CASES))
def test_vq_oracle_matches_upstream_fixture(name):
    c, cfg, sd, x, g = case(name)
    assert sum(float(v.double().abs().sum()) for v in sd.values()) == pytest.approx(float(g["meta/weight_checksum"]), rel=1e-9)
    assert float(x.double().abs().sum()) == pytest.approx(float(g["meta/input_checksum"]), rel=1e-9)
    quant, tokens, z = V.vq_encode(sd, cfg, x)
    assert np.array_equal(tokens.numpy(), g["tokens"])                       # integer output: bit-exact
    np.testing.assert_allclose(z.numpy(), g["latents"], rtol=0, atol=2e-5 * float(np.abs(g["latents"]).max()))
    assert float(quant.double().sum()) == pytest.approx(float(g["quant_sum"]), rel=1e-6)


@pytest.mark.parametrize("name", list(VQ_CASES))
def test_vq_state_dict_layout(name):
    c, cfg, sd, x, g = case(name)
    model = build(c, cfg)
    own = model.state_dict()
    assert list(own.keys()) == g["meta/keys"].tolist()
    assert [",".join(map(str, v.shape)) for v in own.values()] == g["meta/shapes"].tolist()
    assert not model.load_state_dict(sd, strict=True).missing_keys
    with pytest.raises(RuntimeError, match="move it to the GPU"):
        model.eval().tokenize(x)                                             # no CPU fallback


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(VQ_CASES))
def test_code_assignment_bit_exact_given_latents(name):
    """fm_vq_assign on the upstream latents reproduces the upstream tokens exactly (also with ties)."""
    from fourm.hip import _lib as L, ops
    c, cfg, sd, x, g = case(name)
    z = torch.from_numpy(g["latents"]).reshape(-1, cfg.latent).cuda().contiguous()
    R, K = z.shape[0], cfg.codebook
    embed = sd["quantize._codebook.embed"].cuda()
    en = torch.empty_like(embed)
    L.check(L.l2norm_rows(ops._p(embed), embed.stride(0), ops._p(en), en.stride(0), K, cfg.latent, ops._stream()))
    assert float((en - torch.nn.functional.normalize(embed, dim=-1)).abs().max()) < 1e-6
    for splits in (1, 4, 16):
        wv, wi = torch.empty(R, splits, device="cuda"), torch.empty(R, splits, dtype=torch.int32, device="cuda")
        tok = torch.empty(R, dtype=torch.int64, device="cuda")
        G = cfg.grid ** 2
        quant = torch.empty(R // G, cfg.latent, G, device="cuda")
        L.check(L.vq_assign(ops._p(z), z.stride(0), ops._p(en), ops._p(embed), K, cfg.latent, R, G, 1, ops._p(wv), ops._p(wi), splits,
                            ops._p(tok), ops._p(quant), ops._stream()))
        assert np.array_equal(tok.cpu().numpy(), g["tokens"].reshape(-1)), splits
        assert float(quant.double().sum()) == pytest.approx(float(g["quant_sum"]), rel=1e-6)
    # exact ties: duplicate code rows -> the lower index must win
    embed2 = embed.clone(); embed2[K - 1] = embed2[3]; z2 = embed2[[3, K - 1, 7]].contiguous() * 2.5
    en2 = torch.nn.functional.normalize(embed2, dim=-1)
    tok = torch.empty(3, dtype=torch.int64, device="cuda")
    wv, wi = torch.empty(3, 4, device="cuda"), torch.empty(3, 4, dtype=torch.int32, device="cuda")
    L.check(L.vq_assign(ops._p(z2), z2.stride(0), ops._p(en2), ops._p(embed2), K, cfg.latent, 3, 1, 1, ops._p(wv), ops._p(wi), 4, ops._p(tok),
                        None, ops._stream()))
    assert tok.tolist() == [3, 3, 7]


@pytest.mark.gpu
def test_tokenize_sub_batches_in_flight_on_several_streams():
    """fourm.vq.tokenize_sub_batches (upstream's loop over sub-batches, save_vq_tokens.py:262-288, with 2 / 3 of them in flight on their own HIP
    streams): the same tokens, bit for bit, as one call after the other - the engines keep a scratch set per stream."""
    from fourm.vq import VQ, tokenize_sub_batches
    torch.manual_seed(3)
    model = VQ(image_size=224, enc_type="vit_b_enc", patch_size=16, post_mlp=True, codebook_size=16384, latent_dim=32, norm_codes=True, sync_codebook=False).cuda().eval()
    subs = [torch.rand(16 if i % 3 else 24, 3, 224, 224, device="cuda") * 2 - 1 for i in range(7)]        # ragged sub-batch sizes
    want = [model.tokenize(x).clone() for x in subs]
    for n in (2, 3, 1):
        for _ in range(6):
            got = tokenize_sub_batches(model, subs, n_streams=n)
            torch.cuda.synchronize()
            assert len(got) == len(want) and all(torch.equal(g, w) for g, w in zip(got, want)), n
    assert tokenize_sub_batches(model, []) == []


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(VQ_CASES))
def test_tokenize_end_to_end(name):
    c, cfg, sd, x, g = case(name)
    model = build(c, cfg)
    model.load_state_dict(sd)
    model = model.cuda().eval()
    quant, loss, tokens = model.encode(x.cuda())
    assert tokens.dtype == torch.int64 and tuple(tokens.shape) == (c["batch"], cfg.grid, cfg.grid)
    assert tuple(quant.shape) == (c["batch"], cfg.latent, cfg.grid, cfg.grid) and float(loss) == 0.0
    z = model._last_latents.float().cpu()
    ref = torch.from_numpy(g["latents"])
    rel = float((z - ref).norm() / ref.norm())
    assert rel < 3e-2, rel                                                   # bf16 ViT blocks vs the all-fp32 upstream latents
    # against the oracle with upstream's autocast rounding points (bf16 in the 12 blocks, fp32 post-MLP / projection /
    # search - no deviation switched into the checker any more)
    _, tok_bf, z_bf = V.vq_encode(sd, cfg, x, emulate_bf16=True)
    rel_bf = float((z - z_bf).norm() / z_bf.norm())
    agree_fp32 = float((tokens.cpu() == torch.from_numpy(g["tokens"]).long()).float().mean())
    agree_bf16 = float((tokens.cpu() == tok_bf).float().mean())
    oracle_self = float((tok_bf == torch.from_numpy(g["tokens"]).long()).float().mean())      # the reference's own autocast-vs-fp32 figure
    from tests.parity_log import record
    record("vq.tokenize", case=name, latent_rel_vs_fp32=rel, latent_rel_vs_autocast_oracle=rel_bf, token_agreement_vs_fp32=agree_fp32,
           token_agreement_vs_autocast_oracle=agree_bf16, oracle_autocast_vs_fp32=oracle_self)
    assert rel_bf < 8e-3, rel_bf
    # upstream measured 97.1 % agreement between its own bf16-autocast and fp32 encoders on real images; with the
    # seeded random weights of this fixture the autocast oracle agrees with fp32 at `oracle_self`
    assert agree_fp32 > 0.95 * oracle_self and agree_fp32 > 0.9 and agree_bf16 > 0.93, (agree_fp32, agree_bf16, oracle_self)
    # every disagreement with the bf16-emulating oracle is a near tie in that oracle's similarities
    en = torch.nn.functional.normalize(sd["quantize._codebook.embed"], dim=-1)
    sims = torch.nn.functional.normalize(z_bf.reshape(-1, cfg.latent), dim=-1) @ en.t()
    bad = (tokens.cpu().reshape(-1) != tok_bf.reshape(-1)).nonzero().flatten()
    for r in bad.tolist():
        top = sims[r].topk(2).values
        mine = sims[r, tokens.cpu().reshape(-1)[r]]
        assert float(top[0] - mine) < 2e-2, (r, float(top[0] - mine))
    print(f"{name}: latent rel err {rel:.2e}, token agreement fp32 {agree_fp32:.3f} / bf16-oracle {agree_bf16:.3f}")


@pytest.mark.gpu
@pytest.mark.parametrize("K,R,thr", [(64, 500, 0.0), (16384, 12544, 0.25), (128, 40, 2.0)])
def test_codebook_ema_update(K, R, thr):
    """Training-mode codebook update (fm_vq_code_stats + fm_vq_ema_update + dead-code replacement) against the oracle restatement of
    upstream CosineSimCodebook.forward's training branch (pinned to upstream by tests/test_vq_ema_oracle.py)."""
    from fourm.vq.quantizers.quantize_lucid import CosineSimCodebook
    g = torch.Generator().manual_seed(K + R)
    cb = CosineSimCodebook(dim=32, codebook_size=K, decay=0.9, threshold_ema_dead_code=thr, code_replacement_policy="batch_random")
    cb.cluster_size.copy_(torch.rand(K, generator=g) * 3)
    e0, c0 = cb.embed.clone(), cb.cluster_size.clone()
    z = torch.randn(R, 32, generator=g) * 1.7
    ind, _ = V.assign_codes(z, e0)
    cb = cb.cuda().train()
    bins = cb.ema_update_(z.cuda(), ind.cuda(), generator=torch.Generator(device="cuda").manual_seed(5))
    assert torch.equal(bins.cpu(), torch.bincount(ind, minlength=K).float())
    e1, c1 = V.codebook_ema_update(e0, c0, z, ind, 0.9)
    rows = None
    if thr > 0 and bool((c1 < thr).any()):
        n = int((c1 < thr).sum())
        gen = torch.Generator(device="cuda").manual_seed(5)
        idx = (torch.randperm(R, device="cuda", generator=gen)[:n] if R >= n else torch.randint(0, R, (n,), device="cuda", generator=gen)).cpu()
        rows = torch.nn.functional.normalize(z[idx], dim=-1)
        e1, c1 = V.codebook_ema_update(e0, c0, z, ind, 0.9, threshold_dead=thr, replace_rows=rows)
    assert torch.allclose(cb.cluster_size.cpu(), c1, rtol=1e-6, atol=1e-7)
    err = float((cb.embed.cpu() - e1).abs().max())
    assert err < 2e-6, err                                       # fp32 atomics order + one fused multiply-add
    assert cb.epoch == 1


@pytest.mark.gpu
def test_training_mode_encode_updates_the_codebook():
    """VQ.encode in training mode (parameters frozen): same tokens / quantised vectors as eval, the commitment term's value, and the
    codebook moved exactly as the oracle update of the kernel's own latents says; the next encode searches the UPDATED codebook."""
    c, cfg, sd, x, g = case("vq_small")
    vq = build(c, cfg)
    vq.load_state_dict(sd, strict=True)
    for p in vq.parameters():
        p.requires_grad = False
    vq = vq.cuda().eval()
    q0, l0, t0 = vq.encode(x.cuda())
    assert float(l0) == 0.0
    e0, c0 = vq.quantize._codebook.embed.cpu().clone(), vq.quantize._codebook.cluster_size.cpu().clone()
    vq.train()
    vq.quantize._codebook.threshold_ema_dead_code = 0.0
    q1, l1, t1 = vq.encode(x.cuda())
    assert torch.equal(t1, t0) and torch.equal(q1, q0)
    z = vq._last_latents.float().cpu()
    want = torch.nn.functional.mse_loss(q1.cpu().flatten(2).transpose(1, 2), z)
    assert abs(float(l1) - float(want)) < 1e-6 * max(1.0, float(want))
    e1, c1 = V.codebook_ema_update(e0, c0, z, t1.cpu(), vq.ema_decay)
    assert float((vq.quantize._codebook.embed.cpu() - e1).abs().max()) < 2e-6 and torch.allclose(vq.quantize._codebook.cluster_size.cpu(), c1, rtol=1e-6)
    assert float((e1 - e0).abs().max()) > 1e-4                                      # it did move
    t2 = vq.eval().tokenize(x.cuda())
    ind2, _ = V.assign_codes(z.reshape(-1, z.shape[-1]), vq.quantize._codebook.embed.cpu())
    assert (t2.cpu().reshape(-1) == ind2).float().mean() > 0.999                   # the cached normalised codes were rebuilt
    with pytest.raises(NotImplementedError):
        for p in vq.parameters():
            p.requires_grad = True
        vq.train().encode(x.cuda())


# ---- k-means codebook initialisation (kmeans_init=True) ---------------------------------------------------------------------------------
def _clustered(K, per, d, seed):
    g = torch.Generator().manual_seed(seed)
    centres = torch.nn.functional.normalize(torch.randn(K, d, generator=g), dim=-1)
    pts = centres.repeat_interleave(per, 0) + 0.02 * torch.randn(K * per, d, generator=g)
    pts = pts * (0.5 + torch.rand(K * per, 1, generator=g))             # raw latents: arbitrary norms
    perm = torch.randperm(K * per, generator=g)
    return pts[perm].contiguous()


def test_kmeans_oracle_matches_upstream():
    """upstream's kmeans(use_cosine_sim=True) on these point sets and initial rows, recorded by tests/golden/make_golden_upstream_pins.py."""
    pins = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "upstream_pins.npz"))
    for K, per, seed in ((16, 20, 0), (64, 3, 1), (8, 2, 2)):
        x = torch.nn.functional.normalize(_clustered(K, per, 32, seed), dim=-1)
        idx = torch.randperm(x.shape[0], generator=torch.Generator().manual_seed(seed))[:K + 3]
        ref, rb = torch.from_numpy(pins[f"kmeans.{seed}.means"]), torch.from_numpy(pins[f"kmeans.{seed}.bins"])
        got, gb = V.kmeans_cosine(x, idx, 10)
        assert torch.equal(rb, gb) and torch.allclose(ref, got, atol=1e-6), (K, per)


@pytest.mark.gpu
@pytest.mark.parametrize("K,per", [(64, 12), (2048, 4)])
def test_kmeans_init_matches_oracle(K, per):
    from fourm.vq.quantizers.quantize_lucid import CosineSimCodebook
    z = _clustered(K, per, 32, seed=K)
    cb = CosineSimCodebook(dim=32, codebook_size=K, kmeans_init=True, kmeans_iters=10).cuda()
    assert not bool(cb.initted) and float(cb.embed.abs().sum()) == 0.0
    idx = torch.randperm(z.shape[0], generator=torch.Generator().manual_seed(3))[:K]
    cb.init_embed_(z.cuda(), init_index=idx)
    means, bins = V.kmeans_cosine(torch.nn.functional.normalize(z, dim=-1), idx, 10)
    assert bool(cb.initted)
    assert torch.equal(cb.cluster_size.cpu().long(), bins)                          # well separated clusters: the same partition
    assert float((cb.embed.cpu() - means).abs().max()) < 5e-6
    cb.init_embed_(torch.zeros_like(z).cuda())                                      # initialised: a second call is a no-op
    assert float((cb.embed.cpu() - means).abs().max()) < 5e-6


@pytest.mark.gpu
def test_kmeans_init_inside_encode():
    """kmeans_init=True end to end: the first training-mode encode initialises the codebook from its own latents, then assigns."""
    from fourm.vq import VQ
    c, cfg, sd, x, g = case("vq_small")
    vq = VQ(image_size=cfg.image, enc_type=c["enc_type"], patch_size=cfg.patch, post_mlp=cfg.post_mlp, codebook_size=32, latent_dim=cfg.latent,
            norm_codes=True, sync_codebook=False, kmeans_init=True, threshold_ema_dead_code=0)
    vq.load_state_dict({k: v for k, v in sd.items() if not k.startswith("quantize.")}, strict=False)
    for p in vq.parameters():
        p.requires_grad = False
    vq = vq.cuda().train()
    torch.manual_seed(0)
    quant, loss, tokens = vq.encode(x.cuda())
    cbk = vq.quantize._codebook
    assert bool(cbk.initted) and int(tokens.max()) < 32 and float(loss) > 0
    assert torch.allclose(cbk.embed.norm(dim=-1).cpu(), torch.ones(32), atol=1e-4)
    assert len(tokens.unique()) > 8                                                 # 48 latents spread over the 32 initial means
