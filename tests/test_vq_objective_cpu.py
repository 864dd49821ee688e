"""The tokenizer training objective without a GPU: the C ABI additions (header, ctypes mirrors, struct layout), the refusals of
fourm.vq.training, the host path of compute_codebook_usage, and ModelEma where it is upstream's torch expression (a CPU-resident EMA,
the checkpoint round trip).  The kernels themselves are tested on the GPU (tests/test_vq_objective_gpu.py)."""
import ctypes
import math
import os
import re
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from torch import nn

from tests.test_trainer_cpu import child

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["fm_reconst_loss_scratch", "fm_reconst_loss", "fm_scale_f32", "fm_mask_out_samples", "fm_ema_update", "fm_diffusion_pair", "fm_token_usage"]


def _header():
    return open(os.path.join(ROOT, "include", "fourm_hip.h")).read()


def test_abi_additions_are_declared_exported_and_built():
    from fourm.hip import _lib
    import importlib.util
    header = _header()
    for name in NEW:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib.EXPORTS and hasattr(_lib.lib, name), name
    assert _lib.ABI_VERSION == 11 and _lib.lib.fm_abi_version() == 11 and re.search(r"#define FM_ABI_VERSION 11\b", header)
    for name, val in dict(FM_LOSS_MSE=_lib.LOSS_MSE, FM_LOSS_L1=_lib.LOSS_L1, FM_LOSS_SMOOTH_L1=_lib.LOSS_SMOOTH_L1, FM_LOSS_CE_INDEX=_lib.LOSS_CE_INDEX,
                          FM_LOSS_BCE=_lib.LOSS_BCE, FM_LOSS_COSINE=_lib.LOSS_COSINE, FM_LOSS_COSINE_1D=_lib.LOSS_COSINE_1D,
                          FM_RECONST_CHUNK=_lib.RECONST_CHUNK, FM_EMA_CHUNK=_lib.EMA_CHUNK).items():
        assert re.search(rf"{name}\s*(=|\s)\s*{val}\b", header), name
    assert _lib.TOKEN_USAGE_MAX_K == 1 << 20 and "#define FM_TOKEN_USAGE_MAX_K (1 << 20)" in header
    spec = importlib.util.spec_from_file_location("build_ext", os.path.join(ROOT, "ml-4m_amd", "build_ext.py"))
    be = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(be)
    assert "train_objective.hip" in be.SOURCES and "-ffp-contract=off" in be.EXTRA_FLAGS["train_objective.hip"]


def test_ema_job_mirror_matches_the_header_layout(tmp_path):
    """sizeof and every field offset of fm_ema_job as gcc lays it out against the ctypes mirror (the method of
    tests/test_model_cpu.py::test_ctypes_mirrors_match_the_header_layout)."""
    from fourm.hip import _lib
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler")
    body = re.search(r"typedef struct fm_ema_job \{(.*?)\} fm_ema_job;", _header(), re.S).group(1)
    names = [re.search(r"([A-Za-z_][A-Za-z0-9_]*)\s*$", d.strip()).group(1) for d in body.split(";") if d.strip()]
    assert names == [f[0] for f in _lib.EmaJob._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "fourm_hip.h"', 'int main(void) {', '  printf("size %zu\\n", sizeof(fm_ema_job));']
    lines += [f'  printf("{n} %zu\\n", offsetof(fm_ema_job, {n}));' for n in names] + ["  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert ctypes.sizeof(_lib.EmaJob) == int(out["size"]) == 32
    for n in names:
        assert getattr(_lib.EmaJob, n).offset == int(out[n]), n


def test_modules_import_and_refuse_without_a_gpu():
    from fourm.vq import training as T
    from fourm.vq import vq_utils
    assert callable(vq_utils.compute_codebook_usage) and set(T.LOSS_FNS) == {"mse", "l1", "smooth_l1", "cross_entropy", "binary_cross_entropy", "cosine", "cosine_1d"}
    x, t = torch.randn(2, 3, 4, 4, requires_grad=True), torch.randn(2, 3, 4, 4)
    with pytest.raises(ValueError, match="Unknown loss function huber"):
        T.compute_reconst_loss(x, t, "huber")
    for fn in T.LOSS_FNS:
        tt = torch.zeros(2, 4, 4, dtype=torch.int64) if fn == "cross_entropy" else t
        with pytest.raises(RuntimeError, match="HIP kernels only"):
            T.compute_reconst_loss(x, tt, fn)
    with pytest.raises(NotImplementedError, match="target"):
        T.compute_reconst_loss(x, t.clone().requires_grad_(True), "mse")
    # mask_out_samples: untouched without a mask or a value (upstream's contract, CPU tensors included), otherwise the kernel or nothing
    assert T.mask_out_samples(t) is t and T.mask_out_samples(t, torch.ones(2, 1, 4, 4, dtype=torch.bool)) is t and T.mask_out_samples(t, None, 0.0) is t
    with pytest.raises(RuntimeError, match="HIP kernels only"):
        T.mask_out_samples(t, torch.ones(2, 1, 4, 4, dtype=torch.bool), 0.0)
    from fourm.vq.scheduling import DDPMScheduler
    sch = DDPMScheduler(num_train_timesteps=10)
    with pytest.raises(RuntimeError, match="HIP kernels only"):
        T.diffusion_training_pair(sch, t, torch.randn_like(t), torch.tensor([0, 9]), "v_prediction")
    with pytest.raises(ValueError, match="prediction_type"):
        T.diffusion_training_pair(sch, t, torch.randn_like(t), torch.tensor([0, 9]), "flow")


def test_utils_model_ema_still_needs_a_checkout():
    """fourm.vq.training.ModelEma is NOT exported from fourm.utils: that name keeps resolving to upstream only."""
    out = child("""
        import fourm.utils as U
        from fourm.vq.training import ModelEma
        assert "ModelEma" not in vars(U)
        try:
            U.ModelEma
        except AttributeError as e:
            assert "FOURM_UPSTREAM" in str(e), e
        else:
            raise SystemExit("fourm.utils.ModelEma resolved without an upstream checkout")
        print("ok")
    """)
    assert out.strip().endswith("ok")


def _np_usage(tokens, K, window):
    """Independent count: numpy.unique per full window."""
    a = tokens.numpy()
    n = len(a) // window
    vals = [len(np.unique(a[i * window:(i + 1) * window])) / K for i in range(n)]
    return float(np.mean(vals)) if vals else float("nan")


@pytest.mark.parametrize("dtype", [torch.int64, torch.int32, torch.int16])
def test_codebook_usage_on_cpu_tokens_equals_numpy_unique(dtype):
    from fourm.vq.vq_utils import compute_codebook_usage
    g = torch.Generator().manual_seed(3)
    K, window = 64, 100
    tokens = torch.cat([torch.randint(0, K, (window,), generator=g), torch.arange(window) % K, torch.full((window,), 5), torch.randint(0, 7, (window,), generator=g),
                        torch.randint(0, K, (37,), generator=g)]).to(dtype)                  # four full windows and a ragged tail that is dropped
    got = compute_codebook_usage(tokens, codebook_size=K, window_size=window)
    assert isinstance(got, float) and got == _np_usage(tokens, K, window)
    assert math.isnan(compute_codebook_usage(tokens[:window - 1], codebook_size=K, window_size=window))      # no full window
    assert compute_codebook_usage(torch.arange(16384).to(torch.int64), codebook_size=16384, window_size=16384) == 1.0
    bad = tokens.clone()
    bad[3] = K
    with pytest.raises(ValueError, match="outside"):
        compute_codebook_usage(bad, codebook_size=K, window_size=window)
    bad[3] = -1
    with pytest.raises(ValueError, match="outside"):
        compute_codebook_usage(bad, codebook_size=K, window_size=window)
    with pytest.raises(ValueError, match="codebook_size"):
        compute_codebook_usage(tokens, codebook_size=(1 << 20) + 1, window_size=window)


class _Net(nn.Module):
    """Parameters of several sizes, float buffers and an integer buffer (BatchNorm's num_batches_tracked)."""

    def __init__(self):
        super().__init__()
        self.a, self.bn, self.b = nn.Linear(7, 5), nn.BatchNorm1d(5), nn.Linear(5, 1, bias=False)
        self.register_buffer("scale", torch.tensor(3.0))


def _upstream_update(ema_sd, model_sd, decay):
    """upstream's ModelEma.update expression (model_ema.py:81) entry by entry, on clones."""
    return {k: (v * decay + (1. - decay) * model_sd[k]).to(v.dtype) for k, v in ema_sd.items()}


@pytest.mark.parametrize("decay", [0.9999, 0.8, 0.5])
def test_cpu_resident_model_ema_is_upstreams_expression(decay):
    from fourm.vq.training import ModelEma
    torch.manual_seed(0)
    model = _Net()
    ema = ModelEma(model, decay=decay)
    assert ema.decay == decay and ema.ema_has_module is False and ema.device == '' and not ema.ema.training
    assert all(not p.requires_grad for p in ema.ema.parameters()) and all(p.requires_grad for p in model.parameters())
    assert ema.ema is not model and ema.ema.a.weight.data_ptr() != model.a.weight.data_ptr()
    for step in range(2):
        with torch.no_grad():
            for p in model.parameters():
                p.add_(torch.randn_like(p))
            model.bn.running_mean.add_(0.25)
            model.bn.num_batches_tracked.add_(3)
        want = _upstream_update({k: v.clone() for k, v in ema.ema.state_dict().items()}, model.state_dict(), decay)
        ema.update(model)
        for k, v in ema.ema.state_dict().items():
            assert v.dtype == want[k].dtype and torch.equal(v, want[k]), (k, step)
    # device='cpu' (the EMA kept off the model's device): the same path
    ema_cpu = ModelEma(model, decay=decay, device='cpu')
    want = _upstream_update({k: v.clone() for k, v in ema_cpu.ema.state_dict().items()}, model.state_dict(), decay)
    ema_cpu.update(model)
    assert all(torch.equal(v, want[k]) for k, v in ema_cpu.ema.state_dict().items())


def test_checkpoint_round_trips_model_ema(tmp_path):
    from fourm.utils import NativeScalerWithGradNormCount, auto_load_model, save_model
    from fourm.vq.training import ModelEma
    torch.manual_seed(1)
    model = _Net()
    ema = ModelEma(model, decay=0.9)
    with torch.no_grad():
        for p in model.parameters():
            p.add_(1.0)
    ema.update(model)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3)
    scaler = NativeScalerWithGradNormCount(enabled=False)
    args = SimpleNamespace(output_dir=str(tmp_path), auto_resume=False, resume="", start_epoch=0)
    save_model(args, 2, model, model, opt, scaler, model_ema=ema)
    blob = torch.load(tmp_path / "checkpoint-2.pth", weights_only=False)
    assert set(blob["model_ema"]) == set(model.state_dict())
    model2 = _Net()
    ema2 = ModelEma(model2, decay=0.9)
    args.resume, args.model_ema = str(tmp_path / "checkpoint-2.pth"), True
    auto_load_model(args, model2, model2, torch.optim.AdamW(model2.parameters(), lr=1e-3), scaler, model_ema=ema2)
    for (k, a), b in zip(ema.ema.state_dict().items(), ema2.ema.state_dict().values()):
        assert torch.equal(a, b), k
    assert not torch.equal(ema2.ema.a.weight, model2.a.weight)                                     # the EMA weights, not the model's
    # resume='...' of the constructor reads upstream's 'state_dict_ema' layout
    torch.save({"state_dict_ema": ema.ema.state_dict()}, tmp_path / "ema.pth")
    ema3 = ModelEma(_Net(), decay=0.9, resume=str(tmp_path / "ema.pth"))
    assert all(torch.equal(a, b) for a, b in zip(ema.ema.state_dict().values(), ema3.ema.state_dict().values()))
