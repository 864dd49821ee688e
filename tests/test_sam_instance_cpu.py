"""SAM-instance tokenizer, host side (no GPU): VQVAE(out_conv=True, latent_dim=1024) has upstream's state-dict layout (fixture of the
unmodified upstream model, tests/golden/make_golden_sam_instance.py), loads upstream-named weights strictly, and get_image_tokenizer
builds it from a checkpoint whose arguments are written like upstream's SAM-instance YAML
(cfgs/default/tokenization/vqvae/sam_instance/ViTB-ViTB_1k_224_64.yaml)."""
import argparse
import os

import numpy as np
import pytest
import torch

from tests import sam_instance_util as S

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def fixture():
    return np.load(os.path.join(GOLD, "sam_instance_small.npz"))


def test_seeds_reproduce_the_fixture_inputs():
    g = fixture()
    sd, x = S.sam_state_dict(), S.synthetic_masks(S.SAM_SMALL["batch"], S.SAM_SMALL["image"], seed=S.SAM_SMALL["seed"])
    assert sum(float(v.double().abs().sum()) for v in sd.values()) == pytest.approx(float(g["meta/weight_checksum"]), rel=1e-9)
    assert float(x.double().abs().sum()) == pytest.approx(float(g["meta/input_checksum"]), rel=1e-9)
    assert set(x.unique().tolist()) == {0.0, 1.0}
    _, cx = S.convnext_c3_case()
    assert float(cx.double().abs().sum()) == pytest.approx(float(g["convnext_c3/input_checksum"]), rel=1e-9)


def test_out_conv_state_dict_layout_matches_upstream():
    from fourm.vq import VQVAE
    g = fixture()
    m = VQVAE(**S.sam_kwargs())
    own = m.state_dict()
    shapes = dict(zip(g["meta/keys"].tolist(), g["meta/shapes"].tolist()))
    assert set(own) == set(shapes), set(own) ^ set(shapes)
    for k, v in own.items():
        assert ",".join(map(str, v.shape)) == shapes[k], k
    for i in range(2):
        for leaf in ("dwconv.weight", "dwconv.bias", "norm.weight", "norm.bias", "pwconv1.weight", "pwconv1.bias", "pwconv2.weight", "pwconv2.bias", "gamma"):
            assert f"decoder.out_conv.{i}.{leaf}" in own
    # upstream's initialisation: layer scale 1e-6, unit LayerNorm, zero Linear biases
    blk = m.decoder.out_conv[0]
    assert torch.equal(blk.gamma.detach(), torch.full((1,), 1e-6)) and float(blk.norm.weight.detach()) == 1.0 and float(blk.norm.bias.detach()) == 0.0
    assert float(blk.pwconv1.bias.detach().abs().sum()) == 0.0 and tuple(blk.dwconv.weight.shape) == (1, 1, 7, 7)
    sd = S.sam_state_dict()
    msg = m.load_state_dict(sd, strict=True)
    assert not msg.missing_keys and not msg.unexpected_keys
    for k, v in sd.items():
        assert torch.equal(m.state_dict()[k], v), k
    with pytest.raises(RuntimeError):
        m.decoder.out_conv[0](torch.zeros(1, 1, 8, 8))                 # parameter holder: computed by fm_convnext_block in the engine
    with pytest.raises(RuntimeError, match="move it to the GPU"):
        m.eval().tokenize(S.synthetic_masks(1, 64))                    # no CPU fallback


def test_convnext_sequential_keys_match_upstream():
    from fourm.vq.models.vit_models import ConvNeXtBlock
    g = fixture()
    seq = torch.nn.Sequential(ConvNeXtBlock(3), ConvNeXtBlock(3))
    assert list(seq.state_dict().keys()) == g["convnext_c3/keys"].tolist()
    sd, _ = S.convnext_c3_case()
    assert not seq.load_state_dict(sd, strict=True).missing_keys


def test_out_conv_limits_are_refused_in_the_constructor():
    from fourm.vq import VQVAE
    from fourm.vq.models.vit_models import vit_s_dec
    with pytest.raises(NotImplementedError, match="at most 4 channels"):
        vit_s_dec(out_channels=5, patch_size=8, resolution=32, out_conv=True)
    with pytest.raises(NotImplementedError, match="at most 4 channels"):
        VQVAE(image_size=32, n_channels=8, n_labels=20, enc_type="vit_s_enc", dec_type="vit_s_dec", patch_size=8, codebook_size=64, latent_dim=8, out_conv=True)
    assert hasattr(vit_s_dec(out_channels=4, patch_size=8, resolution=32, out_conv=True), "out_conv")
    assert not hasattr(vit_s_dec(out_channels=4, patch_size=8, resolution=32), "out_conv")


def test_get_image_tokenizer_builds_the_sam_instance_configuration(tmp_path):
    """Arguments as upstream's YAML writes them: encoder_type / decoder_type / quantizer_type names, mask_size next to input_size_min / max."""
    from fourm.vq import VQVAE, get_image_tokenizer
    m = VQVAE(**S.sam_kwargs())
    m.load_state_dict(S.sam_state_dict(), strict=True)
    args = dict(encoder_type="vit_s_enc", decoder_type="vit_s_dec", out_conv=True, patch_size=16, input_size_min=224, input_size_max=224, resolution_step=1,
                mask_size=64, codebook_size=1024, latent_dim=1024, norm_codes=True, quantizer_type="lucid", coef_ema_dead_code=32.0,
                code_replacement_policy="batch_random", commitment_weight=1.0, quantizer_ema_decay=0.99, kmeans_init=False, loss_fn="binary_cross_entropy",
                post_mlp=True, domain="sam_mask", batch_size=384, input_size_eval=64)
    torch.save({"model": m.state_dict(), "args": argparse.Namespace(**args)}, tmp_path / "sam_instance.pth")
    t, a = get_image_tokenizer("sam_instance", str(tmp_path), device="cpu", verbose=False)
    assert isinstance(t, VQVAE) and a.image_size == 64 and t.image_size == 64 and t.latent_dim == 1024 and a.n_channels == 1
    assert hasattr(t.decoder, "out_conv") and t.decoder.out_channels == 1 and not t.training
    for k, v in m.state_dict().items():
        assert torch.equal(t.state_dict()[k], v), k
    enc, _ = get_image_tokenizer("sam_instance", str(tmp_path), encoder_only=True, device="cpu", verbose=False)
    assert not any("decoder" in k for k in enc.state_dict()) and enc.latent_dim == 1024
