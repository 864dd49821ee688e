"""fm_vit_patch_rows (csrc/vit_embed.hip) on a real MI355X, bit for bit: the kernel only moves pixels and rounds them to bf16, so there
is no tolerance.  Reference: ``pixels.to(bfloat16)`` (fp32 rows: the pixels themselves) rearranged by plain torch indexing to
(b, gy, gx) rows of (py, px, c) features.  Buffers are pre-filled with NaN: pad columns must come back zero, rows past the last patch
must keep their bits.  Plus fm_vit_emb_rows and every refusal of the entry point."""
import ctypes as C
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu


def ru(x, m):
    return (x + m - 1) // m * m


def reference_rows(px, P):
    B, Cc, H, W = px.shape
    gh, gw = H // P, W // P
    return px.reshape(B, Cc, gh, P, gw, P).permute(0, 2, 4, 3, 5, 1).reshape(B * gh * gw, P * P * Cc)


def pixels(B, Cc, H, W):
    """Distinct values with a fraction that rounds in bf16: any permutation error shows."""
    n = B * Cc * H * W
    return (torch.arange(n, dtype=torch.float32, device="cuda") * 1.001 + 0.37).reshape(B, Cc, H, W) / 7.0


SHAPES = [(B, Cc, P, grid, extra) for B, Cc, P, grid, extra in itertools.product((1, 3), (1, 3), (4, 8, 16), ((1, 1), (2, 3), (3, 2)), (0, 64))]


@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "fp32"])
def test_patch_rows_bit_exact(f32):
    from fourm.hip import ops
    dt = torch.float32 if f32 else torch.bfloat16
    for B, Cc, P, (gh, gw), extra in SHAPES:
        H, W, live = gh * P, gw * P, P * P * Cc
        ld = ru(live, 64) + extra
        px = pixels(B, Cc, H, W)
        R = B * gh * gw
        rows = torch.full((R + 2, ld), float("nan"), dtype=dt, device="cuda")
        ops.vit_patch_rows(px, rows, P)
        torch.cuda.synchronize()
        ref = reference_rows(px.to(dt), P)
        tag = (B, Cc, P, gh, gw, ld)
        bits = torch.int32 if f32 else torch.int16
        assert torch.equal(rows[:R, :live].contiguous().view(bits), ref.contiguous().view(bits)), tag
        assert bool((rows[:R, live:] == 0).all()) and not bool(torch.signbit(rows[:R, live:].float()).any()), tag      # +0.0 in every pad column
        assert bool(torch.isnan(rows[R:]).all()), tag                                                                 # the rows behind stay untouched


def test_patch_rows_scalar_path_and_several_strips():
    """P = 6 and a width that is no multiple of 4 pixels take the scalar loads; 40 patches of 16 x 16 x 3 per image row need 4 strips."""
    from fourm.hip import ops
    for B, Cc, P, gh, gw in ((2, 3, 6, 2, 3), (1, 3, 16, 1, 40), (2, 1, 4, 1, 5)):
        px = pixels(B, Cc, gh * P, gw * P)
        live, R = P * P * Cc, B * gh * gw
        for dt in (torch.bfloat16, torch.float32):
            rows = torch.full((R + 2, ru(live, 64)), float("nan"), dtype=dt, device="cuda")
            ops.vit_patch_rows(px, rows, P)
            assert torch.equal(rows[:R, :live], reference_rows(px.to(dt), P)), (B, Cc, P, gh, gw, dt)
            assert bool((rows[:R, live:] == 0).all()) and bool(torch.isnan(rows[R:]).all())


def test_emb_rows():
    from fourm.hip import ops
    B, Np, D = 3, 16, 128
    pos, mod = torch.randn(1, Np, D, device="cuda"), torch.randn(1, 1, D, device="cuda")
    x = torch.full((ru(B * Np, 128), D), float("nan"), device="cuda")
    ops.vit_emb_rows(pos, mod, x, B, Np)
    assert torch.equal(x[:B * Np].view(B, Np, D), (pos + mod).expand(B, Np, D)) and bool(torch.isnan(x[B * Np:]).all())


def test_refusals_launch_nothing():
    from fourm.hip import _lib as L
    px = pixels(1, 3, 32, 32)
    rows = torch.full((16, 256), float("nan"), dtype=torch.bfloat16, device="cuda")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(pixels_ptr, rows_ptr, ld, B, Cc, H, W, P, f32=0):
        rc = L.vit_patch_rows(pixels_ptr, rows_ptr, ld, B, Cc, H, W, P, f32, s)
        return rc, L.lib.fm_last_error().decode()
    p, r = px.data_ptr(), rows.data_ptr()
    cases = [
        ((p, r, 256, 1, 3, 30, 32, 8), "whole number"),
        ((p, r, 256, 1, 3, 32, 28, 8), "whole number"),
        ((p, r, 196, 1, 3, 32, 32, 8), "multiple of 8"),
        ((p, r, 128, 1, 3, 32, 32, 8), "smaller than the 192 features"),
        ((None, r, 256, 1, 3, 32, 32, 8), "null pointer"),
        ((p, None, 256, 1, 3, 32, 32, 8), "null pointer"),
        ((p + 4, r, 256, 1, 3, 32, 32, 8), "pixels are not 16-byte aligned"),
        ((p, r + 2, 256, 1, 3, 32, 32, 8), "rows are not 16-byte aligned"),
    ]
    for args, msg in cases:
        rc, err = call(*args)
        assert rc != 0 and msg in err, (args[2:], rc, err)
    torch.cuda.synchronize()
    assert bool(torch.isnan(rows).all())          # nothing was launched
    rc, _ = call(p, r, 256, 1, 3, 32, 32, 8)
    torch.cuda.synchronize()
    assert rc == 0 and not bool(torch.isnan(rows[:, :192]).any())


def test_colsum_is_the_double_sum_rounded_once():
    """fm_vit_colsum: db += column sums of an fp32 matrix, summed in double and rounded once - the float64 sum of torch, bit for bit;
    one and several row slices, columns that fill no whole 64-lane tile, a row stride above N; a short workspace is refused."""
    from fourm.hip import _lib as L, ops
    for R, N, ld in ((48, 128, 128), (1, 8, 8), (2100, 70, 72), (5000, 130, 136)):
        g = torch.Generator(device="cuda").manual_seed(R)
        dy = torch.randn(R + 3, ld, device="cuda", generator=g)
        db0 = torch.randn(N, device="cuda", generator=g)
        db = db0.clone()
        ws = torch.zeros(64 * N, dtype=torch.float64, device="cuda")
        ops.vit_colsum(dy[:, :N], db, ws, R=R)
        assert torch.equal(db, (db0.double() + dy[:R, :N].double().sum(0)).float()), (R, N, ld)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = L.vit_colsum(dy.data_ptr(), ld, db.data_ptr(), R, N, ws.data_ptr(), 8 * N, s)
    assert rc != 0 and "workspace" in L.lib.fm_last_error().decode()
    assert L.vit_colsum(None, ld, db.data_ptr(), R, N, ws.data_ptr(), ws.numel() * 8, s) != 0
