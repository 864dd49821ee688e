"""compute_precision = "fp32" of fourm.vq (DiVAE decoder + ViT tokenizer), what can be checked without a GPU: the C ABI of csrc/unet_f32.hip, the
public switch and its refusals, and the float64 yardstick of the GPU tests (tests/divae_f64_util.py) pinned to upstream's fixture in fp32."""
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ml-4m_amd"))
from oracle import divae_oracle as DO  # noqa: E402
from tests import divae_f64_util as F64  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "divae_small.npz")
SMALL = dict(image_size=32, in_channels=3, out_channels=3, cond_channels=8, patch_size=4, model_channels=64, num_res_blocks=1,
             attention_resolutions=(2,), channel_mult=(1, 2))        # = tests/test_divae.py SMALL
NEW = ("fm_unet_im2col_f32", "fm_groupnorm_nhwc_f32", "fm_unet_attention_f32", "fm_add_f32", "fm_silu_f32", "fm_timestep_embedding_f32")


def rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).norm() / (b.norm() + 1e-30))


def test_f32_unet_entry_points_are_declared_exported_and_additive():
    from fourm.hip import _lib
    header = open(os.path.join(ROOT, "include", "fourm_hip.h")).read()
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(_lib.lib, name), name
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert getattr(_lib.lib, name).argtypes is not None, name
    assert _lib.lib.fm_abi_version() == 11 and _lib.ABI_VERSION == 11          # purely additive: the ABI version does not move
    assert "unet_f32.hip" in open(os.path.join(ROOT, "ml-4m_amd", "build_ext.py")).read()
    src = open(os.path.join(ROOT, "ml-4m_amd", "csrc", "unet_f32.hip")).read()
    assert "asm" not in src and "atomicAdd" not in src and "atomicMin" not in src      # plain C++: no inline assembly, no atomics


def _divae(**kw):
    from fourm.vq import DiVAE
    return DiVAE(image_size=32, n_channels=3, enc_type="vit_s_enc", patch_size=16, codebook_size=64, latent_dim=8, post_mlp=True, scheduler="ddim", **kw)


def test_compute_precision_switch_of_vq_and_divae():
    from fourm.vq import VQ
    vq = VQ(image_size=32, enc_type="vit_s_enc", patch_size=16, codebook_size=64, latent_dim=8)
    assert vq.compute_precision == "bf16"
    with pytest.raises(ValueError, match="'bf16' or 'fp32'"):
        vq.compute_precision = "fp16"
    assert vq.compute_precision == "bf16"
    vq.compute_precision = "fp32"
    assert vq.compute_precision == "fp32" and vq.encoder.compute_precision == "fp32"
    assert "compute_precision" not in "".join(vq.state_dict())                  # a plain attribute: not part of a checkpoint
    m = _divae()
    assert m.compute_precision == "bf16" and m.decoder.compute_precision == "bf16"
    m.compute_precision = "fp32"
    assert (m.compute_precision, m.encoder.compute_precision, m.decoder.compute_precision) == ("fp32", "fp32", "fp32")
    m.compute_precision = "bf16"
    assert (m.compute_precision, m.encoder.compute_precision, m.decoder.compute_precision) == ("bf16", "bf16", "bf16")
    # the UNet reads its attribute at the next evaluation and refuses anything else, before it looks at the device
    m.decoder.compute_precision = "fp16"
    with pytest.raises(ValueError, match="compute_precision 'fp16': 'bf16' or 'fp32'"):
        m.decoder(torch.zeros(1, 3, 32, 32), 10, torch.zeros(1, 8, 2, 2))


def test_fp32_is_refused_where_it_is_not_built(monkeypatch):
    from fourm.vq import VQVAE
    monkeypatch.setenv("FOURM_PRECISION", "fp32")                               # (the trunk's variable: not consulted by fourm.vq)
    v = VQVAE(image_size=32, enc_type="vit_s_enc", dec_type="vit_s_dec", patch_size=16, codebook_size=64, latent_dim=8)
    with pytest.raises(NotImplementedError, match="ViT decoder of VQVAE"):
        v.compute_precision = "fp32"
    assert v.compute_precision == "bf16" and getattr(v.encoder, "compute_precision", "bf16") == "bf16"
    v.compute_precision = "bf16"                                                # the default can always be assigned
    from tests import memcodes_util as M
    kw = M.kwargs(M.CASES["bmlp_small"])
    mlp = VQVAE(**kw)                                                           # MLP encoder / decoder with the Memcodes quantizer
    from fourm.vq import VQ
    enc_only = VQ(**{k: v for k, v in kw.items() if k != "dec_type"})
    with pytest.raises(NotImplementedError, match="MLP tokenizers"):
        enc_only.compute_precision = "fp32"
    assert mlp._is_mlp() and mlp.compute_precision == "bf16"
    with pytest.raises(NotImplementedError, match="MLP tokenizers"):
        mlp.compute_precision = "fp32"
    assert mlp.compute_precision == "bf16"
    d = _divae()
    assert d.compute_precision == "bf16" and d.decoder.compute_precision == "bf16"      # despite FOURM_PRECISION


def test_float64_helper_in_fp32_reproduces_upstream_fixture():
    """The yardstick's arithmetic is upstream's: run in fp32 it reproduces the fixture dumped from the unmodified upstream classes as tightly as
    the oracle does (tests/test_divae.py); run in float64 it differs from that fixture by fp32 rounding only."""
    fx = np.load(GOLD)
    cfg = DO.UNetCfg(**SMALL)
    sd = DO.seeded_unet_state_dict(cfg, seed=3)
    x, cond, ts, mask = (torch.from_numpy(fx[k]) for k in ("x", "cond", "ts", "mask"))
    for dt, b_eval, b_loop in ((torch.float32, 2e-6, 2e-5), (torch.float64, 5e-6, 5e-5)):
        P = F64.cast_state(sd, dt)
        for name, t, m in (("unet", ts, None), ("unet_masked", ts, mask), ("unet_t250", 250, None)):
            y = F64.unet_forward(P, cfg, x, t, cond, m, dtype=dt)
            assert y.dtype == dt and rel(y, fx[name]) < b_eval, (dt, name, rel(y, fx[name]))
        for kind, n in (("ddim", 4), ("ddpm", 3)):
            gen = torch.Generator().manual_seed(5)
            noise0 = torch.randn(3, 3, 32, 32, generator=gen)
            step_noise = [torch.randn(3, 3, 32, 32, generator=gen) for _ in range(n)] if kind == "ddpm" else None
            img, outs = F64.sample_loop(P, cfg, DO.SchedCfg(kind=kind), cond, noise0, n, "trailing", step_noise, dtype=dt)
            assert img.dtype == dt and rel(img, fx[f"loop_{kind}"]) < b_loop and rel(outs[0], fx[f"loop_{kind}_out0"]) < b_eval, (dt, kind)
        # the schedule table: the oracle's bound in fp32; in float64 the fixture's own fp32 product of 1000 factors <= 1 shows (<= 1000 * 2^-24)
        assert float((F64.alphas_cumprod(DO.SchedCfg(), dt).double() - torch.from_numpy(fx["ac_cos"]).double()).abs().max()) < (1e-7 if dt == torch.float32 else 1000 * 2.0 ** -24)
