"""The image resize without a GPU: fm_resize_axis_table (a host function of libfourm_hip.so) against F.interpolate in float64 - the contract of
the resize kernels - and the argument checks of fourm.vq.resize / fourm.vq.training that need no device.  The kernels themselves are tested
on the GPU (tests/test_vq_resize_gpu.py)."""
import pytest
import torch
import torch.nn.functional as F

from tests import vq_resize_util as RU


def _ops():
    from fourm.hip import _lib as L, ops
    return L, ops


@pytest.fixture(scope="module")
def tables():
    """Every axis table the tests read, built once: (n_in, n_out, mode id) -> dict of CPU tensors."""
    L, ops = _ops()
    out = {}
    for (hi, wi), (ho, wo) in RU.TABLE_PAIRS:
        for mode in (L.RESIZE_BILINEAR, L.RESIZE_BILINEAR_AA, L.RESIZE_NEAREST):
            for n_in, n_out in ((hi, ho), (wi, wo)):
                if (n_in, n_out, mode) not in out:
                    out[n_in, n_out, mode] = ops.resize_axis_table(n_in, n_out, mode)
    return out


@pytest.mark.parametrize("antialias", [False, True], ids=["plain", "antialias"])
@pytest.mark.parametrize("sizes", RU.TABLE_PAIRS, ids=RU.shape_id)
def test_tables_reproduce_interpolate_in_float64(sizes, antialias, tables):
    """Mh x Mw^T with the dense float64 matrices of the two axis tables against F.interpolate of a float64 (2, 3, H, W) input: within 1e-12."""
    L, _ = _ops()
    (hi, wi), (ho, wo) = sizes
    mode = L.RESIZE_BILINEAR_AA if antialias else L.RESIZE_BILINEAR
    x = torch.randn(2, 3, hi, wi, dtype=torch.float64, generator=RU.gen(hi * 1000 + wo))
    Mh, Mw = RU.dense_matrix(tables[hi, ho, mode], hi), RU.dense_matrix(tables[wi, wo, mode], wi)
    got = torch.einsum("oh,bchw,pw->bcop", Mh, x, Mw)
    ref = RU.interp64(x, (ho, wo), antialias)
    err = float((got - ref).abs().max())
    print(f"{sizes} antialias={antialias}: max |table - F.interpolate| = {err:.3e}")
    assert got.shape == ref.shape and err <= 1e-12


def test_table_invariants(tables):
    """Per table: the fp32 weights are the double weights rounded once; every row sums to 1 within 2 fp32 ulps, has no negative and no zero
    weight inside its count and only zeros behind it; windows lie inside the input and do not move backwards; the transposed ranges are
    exactly the non-zero entries of every column; taps and t_taps are the largest counts."""
    L, _ = _ops()
    for (n_in, n_out, mode), t in tables.items():
        start, count, w32, w64 = t["start"].long(), t["count"].long(), t["weights"], t["weights_f64"]
        assert torch.equal(w32, w64.float()), (n_in, n_out, mode)
        assert t["taps"] == int(count.max()) <= L.RESIZE_MAX_TAPS and w32.shape == (n_out, t["taps"])
        inside = torch.arange(t["taps"])[None, :] < count[:, None]
        assert bool((w32[inside] > 0).all()) and bool((w32[~inside] == 0).all())
        assert float((w32.double().sum(1) - 1).abs().max()) <= 2 * 2.0 ** -23
        assert int(start.min()) >= 0 and int((start + count).max()) <= n_in and int(count.min()) >= 1
        assert bool((start[1:] >= start[:-1]).all()) and bool(((start + count)[1:] >= (start + count)[:-1]).all())
        M = RU.dense_matrix(t, n_in, "weights")
        ts, tc = t["t_start"].long(), t["t_count"].long()
        cover = (torch.arange(n_out)[:, None] >= ts[None, :]) & (torch.arange(n_out)[:, None] < (ts + tc)[None, :])
        assert torch.equal(cover, M != 0), (n_in, n_out, mode)
        assert t["t_taps"] == int(tc.max()) and bool((ts[1:] >= ts[:-1]).all()) and int(ts.min()) >= 0 and int((ts + tc).max()) <= n_out


def test_nearest_table_is_interpolates_index_rule(tables):
    """The start array of FM_RESIZE_NEAREST against F.interpolate(mode='nearest') of a ramp, for every pair and a few where fp32 rounding of
    the scale decides the index."""
    L, ops = _ops()
    pairs = {(k[0], k[1]) for k in tables} | {(7, 5), (10, 3), (299, 112), (1000, 999), (3, 700)}
    for n_in, n_out in sorted(pairs):
        t = tables.get((n_in, n_out, L.RESIZE_NEAREST)) or ops.resize_axis_table(n_in, n_out, L.RESIZE_NEAREST)
        ref = F.interpolate(torch.arange(n_in, dtype=torch.float32).view(1, 1, n_in, 1), (n_out, 1), mode="nearest").view(-1)
        assert torch.equal(t["start"].float(), ref) and t["taps"] == 1 and bool((t["count"] == 1).all()) and bool((t["weights"] == 1).all()), (n_in, n_out)


def test_table_refusals():
    """A window wider than FM_RESIZE_MAX_TAPS, bad sizes and an unknown mode return -1 with a message and write nothing."""
    L, ops = _ops()
    none = (None,) * 6
    assert L.RESIZE_MAX_TAPS == 64
    assert L.resize_axis_table(4096, 32, L.RESIZE_BILINEAR_AA, *none) == -1 and b"FM_RESIZE_MAX_TAPS" in L.lib.fm_last_error()
    assert L.resize_axis_table(100, 1, L.RESIZE_BILINEAR_AA, *none) == -1 and b"FM_RESIZE_MAX_TAPS" in L.lib.fm_last_error()
    assert L.resize_axis_table(64, 1, L.RESIZE_BILINEAR_AA, *none) == 64          # the widest window that is taken
    assert L.resize_axis_table(4096, 32, L.RESIZE_BILINEAR, *none) == 2           # (not antialiased: two taps whatever the scale)
    for bad in ((0, 4, L.RESIZE_BILINEAR), (4, 0, L.RESIZE_BILINEAR), (-3, 4, L.RESIZE_NEAREST), (4, 4, 3), (4, 4, -1), ((1 << 24) + 1, 4, L.RESIZE_NEAREST)):
        assert L.resize_axis_table(*bad, *none) == -1, bad
    with pytest.raises(RuntimeError, match="FM_RESIZE_MAX_TAPS"):
        ops.resize_axis_table(4096, 32, L.RESIZE_BILINEAR_AA)


def test_kernel_entry_points_refuse_bad_arguments_before_any_launch():
    """Null pointers, non-positive sizes and tap counts outside [1, FM_RESIZE_MAX_TAPS] are refused by the host code (no GPU is touched)."""
    L, _ = _ops()
    p = 4096          # never dereferenced: every call below is refused first
    ok_f = [p, p, 6, 8, 8, 4, 4, p, p, p, 2, p, p, p, 2, None, None, 3, None]
    assert L.resize_bilinear_fwd(*(ok_f[:0] + [None] + ok_f[1:])) == -1 and b"null" in L.lib.fm_last_error()
    assert L.resize_bilinear_fwd(*(ok_f[:3] + [0] + ok_f[4:])) == -1 and b"bad shape" in L.lib.fm_last_error()
    assert L.resize_bilinear_fwd(*(ok_f[:10] + [65] + ok_f[11:])) == -1 and b"taps" in L.lib.fm_last_error()
    assert L.resize_bilinear_fwd(*(ok_f[:14] + [0] + ok_f[15:])) == -1 and b"taps" in L.lib.fm_last_error()
    assert L.resize_bilinear_fwd(*(ok_f[:15] + [p, None] + ok_f[17:])) == -1 and b"together" in L.lib.fm_last_error()
    assert L.resize_bilinear_fwd(*([p + 2] + ok_f[1:])) == -1 and b"misaligned" in L.lib.fm_last_error()
    ok_b = [p, p, 6, 8, 8, 4, 4, p, p, p, 2, p, p, p, p, p, 2, p, p, None, 3, None]
    assert L.resize_bilinear_bwd(*(ok_b[:11] + [None] + ok_b[12:])) == -1 and b"null" in L.lib.fm_last_error()
    assert L.resize_bilinear_bwd(*(ok_b[:2] + [-1] + ok_b[3:])) == -1 and b"bad shape" in L.lib.fm_last_error()
    assert L.resize_nearest(p, p, 2, 6, 8, 8, 4, 4, p, p, None) == -1 and b"bytes" in L.lib.fm_last_error()
    assert L.resize_nearest(p, p, 4, 6, 8, 8, 4, 4, None, p, None) == -1 and b"null" in L.lib.fm_last_error()
    assert L.resize_nearest(p, p, 8, 6, 8, 0, 4, 4, p, p, None) == -1 and b"bad shape" in L.lib.fm_last_error()


def test_resize_images_argument_checks():
    from fourm.vq import training
    from fourm.vq.resize import resize_images
    assert training.resize_images is resize_images
    x = torch.zeros(1, 3, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        resize_images(x, 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        resize_images(torch.zeros(1, 8, 8, dtype=torch.int64), (4, 4), mode="nearest")
    for mode in ("bicubic", "area", "nearest-exact", None):
        with pytest.raises(ValueError, match="Unknown resize mode"):
            resize_images(x, 4, mode=mode)
    with pytest.raises(ValueError, match="antialias"):
        resize_images(x, 4, mode="nearest", antialias=True)


def test_prepare_inputs_and_perceptual_loss_argument_checks():
    from fourm.vq import training as T
    rgb = torch.zeros(2, 3, 8, 8)
    assert "CLIP-B16" in T.FEAT_MODALITIES and "DINOv2-B14-global" in T.FEAT_MODALITIES and len(T.FEAT_MODALITIES) == 8
    for domain in T.FEAT_MODALITIES:
        with pytest.raises(NotImplementedError, match="out of scope"):
            T.prepare_inputs({"rgb": rgb}, domain, torch.nn.Identity(), "cpu", image_size=4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        T.prepare_inputs({"rgb": rgb}, "rgb", None, "cpu", image_size=4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        T.prepare_inputs({"semseg_coco": torch.zeros(2, 8, 8, dtype=torch.int64)}, "semseg_coco", None, "cpu", image_size=4)
    # nothing to resize, nothing to mask: no device needed
    assert T.prepare_inputs({"rgb": rgb}, "rgb", None, "cpu") is rgb
    poses = torch.zeros(2, 5)
    assert T.prepare_inputs({"human_poses": poses}, "human_poses", None, "cpu", image_size=4).shape == (2, 5, 1, 1)
    inst = torch.arange(2 * 3 * 4 * 4, dtype=torch.float32).view(2, 3, 4, 4)
    valid = torch.tensor([[True, False, True], [False, False, True]])
    got = T.prepare_inputs({"sam_mask": dict(instance=inst, valid=valid)}, "sam_mask", None, "cpu", image_size=2)
    assert torch.equal(got, inst.flatten(end_dim=1)[valid.flatten()].unsqueeze(1)) and got.shape == (3, 1, 4, 4)
    with pytest.raises(TypeError, match="ClipPerceptualLoss or LpipsPerceptualLoss"):
        T.perceptual_loss(torch.nn.MSELoss(), rgb, rgb)
