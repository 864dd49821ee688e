"""MLP + Memcodes tokenizers (human poses, DINOv2 / ImageBind global features), host side (no GPU): VQVAE(enc_type / dec_type
"BottleneckMLP/..." or "MLP/...", quant_type="memcodes") has upstream's state-dict layout (fixture of the unmodified upstream model,
tests/golden/make_golden_memcodes.py), loads upstream-named weights strictly, build_mlp parses upstream's ids, get_image_tokenizer builds
the model from a checkpoint whose arguments are written like upstream's YAMLs
(cfgs/default/tokenization/vqvae/{DINOv2-B14-global,ImageBind-H14-global,human_poses}/), and everything that is not built raises
NotImplementedError before any kernel is launched."""
import argparse
import os

import numpy as np
import pytest
import torch

from tests import memcodes_util as M

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def fixture():
    return np.load(os.path.join(GOLD, "memcodes_small.npz"))


def _untouched(model):
    """No engine was ever built for any part of the model: no workspace, no kernel."""
    return all(getattr(getattr(model, part, None), "_hip_engine", None) is None for part in ("encoder", "decoder", "quantize"))


@pytest.mark.parametrize("name", list(M.CASES))
def test_state_dict_layout_matches_upstream(name):
    from fourm.vq import VQVAE
    from fourm.vq.quantizers import Memcodes
    g, c = fixture(), M.CASES[name]
    sd, xs = M.state_dict(c), M.inputs(name, c)
    assert M.checksum(sd.values()) == pytest.approx(float(g[f"{name}/weight_checksum"]), rel=1e-9)
    assert M.checksum(xs.values()) == pytest.approx(float(g[f"{name}/input_checksum"]), rel=1e-9)
    m = VQVAE(**M.kwargs(c))
    own = m.state_dict()
    shapes = dict(zip(g[f"{name}/keys"].tolist(), g[f"{name}/shapes"].tolist()))
    assert set(own) == set(shapes) == set(sd), set(own) ^ set(shapes)
    for k, v in own.items():
        assert ",".join(map(str, v.shape)) == shapes[k], k
    assert isinstance(m.quantize, Memcodes) and sorted(m.quantize.state_dict()) == ["codes", "to_k.weight", "to_v.weight"]
    assert m.enc_dim == m.encoder.dim_out == c["width"] and m.dec_dim == m.decoder.dim_in == c["width"]
    assert m.encoder.dim_in == c["channels"] and m.decoder.dim_out == c["channels"]
    msg = m.load_state_dict(sd, strict=True)
    assert not msg.missing_keys and not msg.unexpected_keys
    for k, v in sd.items():
        assert torch.equal(m.state_dict()[k], v), k
    # parameter holders: no CPU forward, no fall-back
    with pytest.raises(RuntimeError, match="no stand-alone forward"):
        m.encoder(torch.zeros(1, c["channels"], 1, 1))
    with pytest.raises(RuntimeError, match="move it to the GPU"):
        m.eval().tokenize(xs["g1"])
    with pytest.raises(RuntimeError, match="move it to the GPU"):
        m.eval().decode_quant(torch.zeros(1, c["latent"], 1, 1))
    assert m._inference_only() is not None and "inference only" in m._inference_only()


def test_build_mlp_parses_upstream_ids():
    from fourm.vq.models.mlp_models import BottleneckBlock, BottleneckMLP, StandardMLP, build_mlp
    b = build_mlp("BottleneckMLP/B_6-Wi_1024", dim_in=768, dim_out=None)
    assert isinstance(b, BottleneckMLP) and (b.dim_in, b.dim_out) == (768, 1024) and len(b.blocks) == len(b.layernorms) == 6
    assert b.block_dims == [[4096, 1024]] * 6 and isinstance(b.blocks[0], BottleneckBlock)
    assert tuple(b.blocks[5].block[0].weight.shape) == (4096, 1024) and tuple(b.blocks[5].block[2].weight.shape) == (1024, 4096)
    assert tuple(b.linear_in.weight.shape) == (1024, 768) and b.layernorms[0].eps == 1e-5
    e2 = build_mlp("BottleneckMLP/B_3-Wi_32-E_2", dim_in=None, dim_out=7)
    assert (e2.dim_in, e2.dim_out) == (32, 7) and e2.block_dims == [[64, 32]] * 3 and tuple(e2.linear_out.weight.shape) == (7, 32)
    s = build_mlp("MLP/B_4-Wi_48", dim_in=10)
    assert isinstance(s, StandardMLP) and s.widths == [48] * 4 and len(s.layers) == len(s.layernorms) == 3 and (s.dim_in, s.dim_out) == (10, 48)
    assert sorted(k for k in s.state_dict() if k.startswith("layers.2")) == ["layers.2.bias", "layers.2.weight"]
    with pytest.raises(AssertionError, match="not supported"):
        build_mlp("ResMLP/B_2-Wi_32")


@pytest.mark.parametrize("domain,codebook,channels", [("DINOv2-B14-global", 8192, 40), ("human_poses", 1024, 28)])
def test_get_image_tokenizer_builds_the_mlp_configurations(tmp_path, domain, codebook, channels):
    """Arguments as upstream's trainer writes them (encoder_type / decoder_type / quantizer_type names, num_codebooks, the global-feature
    domains switch patch_proj off); widths scaled down, the id grammar and the code path are the real ones."""
    from fourm.vq import VQ, VQVAE, get_image_tokenizer
    kw = dict(enc_type="BottleneckMLP/B_2-Wi_32", dec_type="BottleneckMLP/B_2-Wi_32", n_channels=channels, latent_dim=32, num_codebooks=4,
              codebook_size=codebook, quant_type="memcodes")
    m = VQVAE(**kw)
    args = dict(encoder_type=kw["enc_type"], decoder_type=kw["dec_type"], quantizer_type="memcodes", codebook_size=codebook, num_codebooks=4, latent_dim=32,
                norm_codes=True, norm_latents=False, patch_size=1, input_size_min=1, input_size_max=1, resolution_step=1, coef_ema_dead_code=32.0,
                code_replacement_policy="batch_random", commitment_weight=1.0, quantizer_ema_decay=0.99, kmeans_init=False, loss_fn="cosine",
                domain=domain, batch_size=256, model_type="VQVAE", use_xformer=False)
    torch.save({"model": m.state_dict(), "args": argparse.Namespace(**args)}, tmp_path / "tok.pth")
    t, a = get_image_tokenizer("tok", str(tmp_path), device="cpu", verbose=False)
    assert isinstance(t, VQVAE) and a.n_channels == channels and t.quant_type == "memcodes" and t.num_codebooks == 4 and not t.training
    assert t.encoder.dim_in == channels and t.decoder.dim_out == channels and t.quantize.codebook_size == codebook
    for k, v in m.state_dict().items():
        assert torch.equal(t.state_dict()[k], v), k
    enc, _ = get_image_tokenizer("tok", str(tmp_path), encoder_only=True, device="cpu", verbose=False)
    assert type(enc) is VQ and not any("decoder" in k or "post_quant_proj" in k for k in enc.state_dict())
    assert torch.equal(enc.quantize.codes, m.quantize.codes) and torch.equal(enc.encoder.linear_in.weight, m.encoder.linear_in.weight)


def test_what_is_not_built_raises_before_any_launch():
    from fourm.vq import VQ, VQVAE
    from fourm.vq.quantizers import Memcodes
    mlp = "BottleneckMLP/B_2-Wi_32"
    ok = dict(enc_type=mlp, n_channels=8, latent_dim=32, num_codebooks=2, codebook_size=16, quant_type="memcodes")
    # the pairings no upstream configuration uses
    with pytest.raises(NotImplementedError, match="BottleneckMLP/B_2-Wi_32.*'lucid'"):
        VQ(**dict(ok, quant_type="lucid"))
    with pytest.raises(NotImplementedError, match="'vit_s_enc'.*'memcodes'"):
        VQ(image_size=32, enc_type="vit_s_enc", patch_size=8, codebook_size=16, latent_dim=32, quant_type="memcodes")
    with pytest.raises(NotImplementedError, match="ViT / MLP mix"):
        VQVAE(dec_type="vit_s_dec", **ok)
    with pytest.raises(NotImplementedError, match="ViT / MLP mix"):
        VQVAE(image_size=32, enc_type="vit_s_enc", dec_type=mlp, patch_size=8, codebook_size=16, latent_dim=32)
    with pytest.raises(NotImplementedError, match="has no HIP kernel"):
        VQ(**dict(ok, quant_type="gumbel"))
    with pytest.raises(NotImplementedError, match="conv_enc not implemented"):
        VQ(**dict(ok, enc_type="conv_enc"))
    # class maps / standardised pixels are inputs of the ViT tokenizers
    with pytest.raises(NotImplementedError, match="n_labels / undo_std"):
        VQ(**dict(ok, n_labels=5))
    with pytest.raises(NotImplementedError, match="n_labels / undo_std"):
        VQ(**dict(ok, n_channels=3, undo_std=True))
    # training mode
    m = VQVAE(dec_type=mlp, **ok)
    x = torch.zeros(2, 8, 1, 1)
    with pytest.raises(NotImplementedError, match="inference only"):
        m.train()(x)
    with pytest.raises(NotImplementedError, match="inference only"):
        m.eval()(x)                                                   # gradients enabled, trainable parameters
    with torch.no_grad():
        with pytest.raises(NotImplementedError, match="inference only"):
            m.train()(x)
        with pytest.raises(NotImplementedError, match="training-mode quantizer"):
            m.train().encode(x)
    with pytest.raises(NotImplementedError):
        m.train().encode(x)
    with pytest.raises(NotImplementedError, match="gumbel-softmax"):
        m.quantize.train()(torch.zeros(2, 32, 1, 1))
    # token shapes without a well-defined embedding
    m.eval()
    for shape in [(2, 2, 1, 3), (2, 2, 2, 2), (2, 2), (2, 3, 1, 1), (2, 1, 1)]:
        with pytest.raises(NotImplementedError, match="not an image-shaped latent"):
            m.tokens_to_embedding(torch.zeros(shape, dtype=torch.int64))
    one = Memcodes(dim=32, codebook_size=16, heads=1)
    with pytest.raises(NotImplementedError, match="not an image-shaped latent"):
        one.indices_to_embedding(torch.zeros(2, 1, 1, 1, dtype=torch.int64))
    with pytest.raises(NotImplementedError, match="accept_image_fmap"):
        Memcodes(dim=32, codebook_size=16, heads=2, accept_image_fmap=False)
    assert _untouched(m) and getattr(one, "_hip_engine", None) is None
    # head widths the search kernel cannot serve are refused before the encoder runs (checked on the host)
    from fourm.vq import engine as E
    with pytest.raises(NotImplementedError, match="head width 4"):
        E._check_memcodes(Memcodes(dim=32, codebook_size=16, heads=8))
    with pytest.raises(NotImplementedError, match="head width 18"):
        E._check_memcodes(Memcodes(dim=36, codebook_size=16, heads=2))
