"""Training the DiVAE decoder on a frozen encoder (fp32 mode), what can be checked without a GPU: the C ABI of csrc/unet_f32_bwd.hip, its
argument checks (they return before anything is launched) and the float64 yardstick of tests/test_divae_train_gpu.py."""
import ctypes
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ml-4m_amd"))
from tests import divae_train_util as TU  # noqa: E402

NEW = ("fm_unet_col2im_f32", "fm_groupnorm_nhwc_bwd_f32", "fm_unet_attention_bwd_f32", "fm_silu_bwd_f32")


def test_backward_entry_points_are_declared_exported_and_additive():
    from fourm.hip import _lib
    header = open(os.path.join(ROOT, "include", "fourm_hip.h")).read()
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(_lib.lib, name), name
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert getattr(_lib.lib, name).argtypes is not None, name
    assert _lib.lib.fm_abi_version() == 11 and _lib.ABI_VERSION == 11          # purely additive: the ABI version does not move
    sys.path.insert(0, os.path.join(ROOT, "ml-4m_amd"))
    import build_ext
    assert "unet_f32_bwd.hip" in build_ext.SOURCES
    src = open(os.path.join(ROOT, "ml-4m_amd", "csrc", "unet_f32_bwd.hip")).read()
    assert "asm" not in src and "atomic" not in src.lower()                    # plain C++: no inline assembly, no atomics of any kind


def test_bad_arguments_are_refused_before_any_launch():
    """Every argument check returns -1 with its reason in fm_last_error(); nothing is dereferenced or launched (the pointers are made up)."""
    from fourm.hip import _lib as L
    p, odd, nul = ctypes.c_void_p(4096), ctypes.c_void_p(4100), None

    def refused(rc, text):
        assert rc == -1, (text, rc)
        assert text in L.lib.fm_last_error().decode(), (text, L.lib.fm_last_error().decode())

    # col2im(col, ldc, dsrc, ld, C, B, H, W, ksize, stride, up1, accumulate, stream)
    refused(L.unet_col2im_f32(nul, 36, p, 4, 4, 1, 5, 5, 3, 1, 0, 0, nul), "bad argument")
    refused(L.unet_col2im_f32(p, 36, p, 4, 4, 1, 5, 5, 1, 1, 0, 0, nul), "ksize=1")
    refused(L.unet_col2im_f32(p, 36, p, 4, 4, 1, 5, 5, 3, 3, 0, 0, nul), "stride=3")
    refused(L.unet_col2im_f32(p, 36, p, 4, 6, 1, 5, 5, 3, 1, 0, 0, nul), "C=6")
    refused(L.unet_col2im_f32(p, 32, p, 4, 4, 1, 5, 5, 3, 1, 0, 0, nul), "ldc=32")
    refused(L.unet_col2im_f32(p, 36, p, 4, 4, 1, 5, 5, 3, 1, 1, 0, nul), "up1")
    refused(L.unet_col2im_f32(p, 36, p, 4, 4, 1, 5, 5, 3, 1, 0, 2, nul), "accumulate=2")
    refused(L.unet_col2im_f32(p, 36, odd, 4, 4, 1, 5, 5, 3, 1, 0, 0, nul), "16-byte aligned")
    # gn_bwd(dy, lddy, x, ldx, add, ld_add, w, b, dx, lddx, dw, db, dadd, ld_dadd, scratch, B, HW, C, groups, eps, silu, stream)
    refused(L.groupnorm_nhwc_bwd_f32(p, 64, p, 64, nul, 0, p, p, nul, 64, nul, nul, nul, 0, nul, 1, 4, 64, 32, 1e-5, 0, nul), "bad argument")
    refused(L.groupnorm_nhwc_bwd_f32(p, 64, p, 64, nul, 0, p, p, p, 64, nul, nul, nul, 0, nul, 1, 4, 65, 32, 1e-5, 0, nul), "C=65")
    refused(L.groupnorm_nhwc_bwd_f32(p, 2048, p, 2048, nul, 0, p, p, p, 2048, nul, nul, nul, 0, nul, 1, 4, 2048, 32, 1e-5, 0, nul), "C=2048")
    refused(L.groupnorm_nhwc_bwd_f32(p, 32, p, 64, nul, 0, p, p, p, 64, nul, nul, nul, 0, nul, 1, 4, 64, 32, 1e-5, 0, nul), "lddy=32")
    refused(L.groupnorm_nhwc_bwd_f32(p, 64, p, 64, nul, 0, p, p, p, 64, nul, nul, p, 8, nul, 1, 4, 64, 32, 1e-5, 0, nul), "ld_dadd=8")
    refused(L.groupnorm_nhwc_bwd_f32(p, 64, p, 64, nul, 0, p, p, p, 64, p, nul, nul, 0, nul, 1, 4, 64, 32, 1e-5, 0, nul), "need the scratch")
    # attn_bwd(qkv, ld, dout, lddo, dqkv, lddqkv, scratch, B, T, heads, ch, stream)
    refused(L.unet_attention_bwd_f32(p, 192, p, 64, p, 192, nul, 1, 4, 1, 64, nul), "bad argument")
    refused(L.unet_attention_bwd_f32(p, 192, p, 64, p, 192, p, 1, 4, 1, 62, nul), "ch=62")
    refused(L.unet_attention_bwd_f32(p, 192, odd, 64, p, 192, p, 1, 4, 1, 64, nul), "16-byte aligned")
    refused(L.unet_attention_bwd_f32(p, 192, p, 64, p, 128, p, 1, 4, 1, 64, nul), "lddqkv=128")
    refused(L.unet_attention_bwd_f32(p, 192, p, 64, p, 192, p, 1, 16000, 1, 64, nul), "too large")
    # silu_bwd(dy, x, dx, n, stream)
    refused(L.silu_bwd_f32(p, p, nul, 4, nul), "bad argument")
    refused(L.silu_bwd_f32(p, p, p, 0, nul), "bad argument")


@pytest.mark.parametrize("name,n_tensors", [("small", 128), ("mid", 334)])
def test_the_yardstick_is_usable(name, n_tensors):
    """Every float64 gradient is non-zero and the fp32 side of the rule is a finite number of floor units: neither side of
    err <= 8 max(own, floor) is noise.  (model_channels = 32 would put one channel in a group: the biases in front of a GroupNorm then have an
    analytically zero gradient - not used.)"""
    ys = TU.yardstick(name)
    assert len(ys) == n_tensors
    units = []
    for k, (ref, bound, own, floor) in ys.items():
        assert bool(torch.isfinite(ref).all()) and float(ref.abs().max()) > 1e-7, (k, float(ref.abs().max()))
        assert floor > 0 and bound >= TU.FACTOR * floor and own < 1e3 * floor, (k, own, floor)
        units.append(own / floor)
    print(f"{name}: own between {min(units):.3g} and {max(units):.3g} floor units; smallest gradient maximum {min(float(r.abs().max()) for r, *_ in ys.values()):.3g}")
