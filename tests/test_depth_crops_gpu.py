"""fourm.data.crops.crop_resize_depth and fourm.data.multimodal_crops.crop_modalities on the GPU against Pillow's recorded I;16 values
(tests/golden/depth_crops.npz) and against the restatement (tests/pil_resize16_util.py): equal integers, equal statistics, and standardised
outputs within 2 fp32 ulps (one for sqrtf, one for the quotient; with equal statistics nothing is amplified).  Pillow is not needed here."""
import os

import numpy as np
import pytest
import torch

from tests import pil_resize16_util as U
from tests import pil_resize_util as U8

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "depth_crops.npz")


def _run(images, settings, S, filt, **kw):
    from fourm.data.crops import crop_resize_depth
    kw.setdefault("out", "uint16")
    return crop_resize_depth(images, [np.asarray(s).reshape(-1, 5) for s in settings], S, resample=filt, **kw)


@pytest.fixture(scope="module")
def fx():
    f = np.load(GOLDEN)
    return {k: f[k] for k in f.files}


@pytest.fixture(scope="module")
def seeded():
    """Images of different sizes (none above 96 x 80) with several crops each, per target size: random boxes, the whole image, a box with
    h = S, one with w = S, one-pixel-wide and one-pixel-high boxes; every third image saturated 0 / 65535.  The restatement of every crop
    is computed once per filter."""
    rng = np.random.default_rng(21)
    out = {}
    for S in (2, 3, 16, 33, 64):
        images, settings = [], []
        for it in range(3):
            H, W = int(rng.integers(S, 81)), int(rng.integers(S, 97))
            images.append(rng.integers(0, 65536, (H, W), dtype=np.uint16) if it else (rng.integers(0, 2, (H, W)) * 65535).astype(np.uint16))
            st = []
            for _ in range(2):
                h, w = int(rng.integers(1, H + 1)), int(rng.integers(1, W + 1))
                st.append((int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1)), h, w, int(rng.integers(0, 2))))
            st += [(0, 0, H, W, it % 2), (H - S, 0, S, W, 1), (0, W - S, H, S, 0), (0, 0, S, S, 1), (0, W // 2, H, 1, 0), (H // 2, 0, 1, W, 1)]
            settings.append(st)
        out[S] = (images, settings, {})
    return out


def _want(seeded, S, filt):
    images, settings, cache = seeded[S]
    if filt not in cache:
        cache[filt] = np.stack([U.crop_resize16(im, s, S, filt) for im, st in zip(images, settings) for s in st]).astype(np.int32)
    return images, settings, cache[filt]


def test_fixture_cases_equal_pillows_values(fx):
    """Every recorded case, one call per case - and all cases of one (source, S, filter) in a single call as well."""
    src = [fx[f"src_{k}"] for k in range(5)]
    names = fx["names"].tolist()
    groups = {}
    for i, (k, top, left, h, w, flip, S, f) in enumerate(fx["cases"].tolist()):
        got = _run([src[k]], [(top, left, h, w, flip)], S, U.FILTERS[f])
        assert got.shape == (1, S, S) and got.dtype == torch.int32
        assert torch.equal(got[0].cpu(), torch.from_numpy(fx[f"out_{i}"].astype(np.int32))), names[i]
        groups.setdefault((k, S, f), []).append((i, (top, left, h, w, flip)))
    for (k, S, f), members in groups.items():
        got = _run([src[k]], [[m[1] for m in members]], S, U.FILTERS[f]).cpu()
        for row, (i, _) in zip(got, members):
            assert torch.equal(row, torch.from_numpy(fx[f"out_{i}"].astype(np.int32))), names[i]
    for must in ("edge_up_bicubic", "edge_up_bicubic_flip", "checkerboard_up", "down_10x_bicubic", "h_eq_S_bicubic", "w_eq_S_bicubic", "both_eq_S_bicubic",
                 "one_wide_bicubic", "one_high_bicubic", "nearest_8_to_7", "S2_nearest", "S2_bilinear"):
        assert must in names
    i = names.index("edge_up_bicubic")          # the per-byte clamp decided this case: a plain 0 .. 65535 clamp gives other values
    k, top, left, h, w, flip, S, f = fx["cases"][i].tolist()
    assert not np.array_equal(U.crop_resize16(src[k], (top, left, h, w, flip), S, "bicubic", plain_clamp=True), fx[f"out_{i}"])


@pytest.mark.parametrize("filt", U.FILTERS + (None,))
def test_seeded_cases_equal_the_restatement(seeded, filt):
    """Several crops per image and images of different sizes in one call, at every target size; S = 33 and 64 take more than one workgroup
    per crop."""
    for S in (2, 3, 16, 33, 64):
        images, settings, want = _want(seeded, S, filt or "bicubic")
        got = _run(images, settings, S, filt)
        assert got.shape == want.shape and torch.equal(got.cpu(), torch.from_numpy(want)), (S, filt)


def test_float32_without_standardisation_is_v_over_65535(seeded):
    for S in (3, 33):
        images, settings, want = _want(seeded, S, "bicubic")
        u16, f32 = _run(images, settings, S, "bicubic", standardize=False, out=("uint16", "float32"))
        assert f32.shape == (want.shape[0], 1, S, S) and f32.dtype == torch.float32 and f32.is_contiguous()
        assert torch.equal(u16.cpu(), torch.from_numpy(want))
        assert torch.equal(f32.cpu()[:, 0], torch.from_numpy(U.unit_f32(want)))
        # torch.Tensor(np.array(img) / (2 ** 16 - 1.0)), as upstream's depth_to_tensor writes it
        assert torch.equal(f32.cpu()[:, 0], torch.Tensor(want.astype(np.uint16) / (2 ** 16 - 1.0)))
        only = _run(images, settings, S, "bicubic", standardize=False, out="float32")
        assert torch.equal(only, f32)
    one = _run(seeded[16][0][:1], [seeded[16][1][0][:1]], 1, "bicubic", standardize=False, out="float32")          # size 1 needs no rank range
    assert one.shape == (1, 1, 1, 1)


def _identity_call(crops, **kw):
    """Crops (S, S) uint16 through crop_resize_depth untouched: a box of the whole image at its own size, so that the standardisation sees
    exactly these values."""
    S = crops[0].shape[0]
    return _run(list(crops), [[(0, 0, S, S, 0)]] * len(crops), S, "bicubic", **kw)


def _check_standardised(crops, f32, stats, u16):
    for k, crop in enumerate(crops):
        want, (mean32, var32) = U.standardize(crop)
        assert torch.equal(u16[k].cpu(), torch.from_numpy(crop.astype(np.int32)))
        got_stats = stats[k].cpu().numpy()
        print(f"crop {k}: stats {got_stats.tolist()} want {[float(mean32), float(var32)]}, ulps {U.ulp_distance(f32[k, 0].cpu().numpy(), want)}")
        assert got_stats[0] == mean32 and got_stats[1] == var32, (k, got_stats, mean32, var32)          # equal bits
        assert U.ulp_distance(f32[k, 0].cpu().numpy(), want) <= 2, k


def test_standardised_fixture_crops(fx):
    """The crops upstream's own function was recorded on: uniform, ties straddling both rank boundaries, constant, a 50-level band, both
    boundaries inside one run of ties, and inside two runs that share a high byte; S in {2, 3, 16, 33}."""
    names = fx["std_names"].tolist()
    by_S = {}
    for i, name in enumerate(names):
        by_S.setdefault(fx[f"std_in_{i}"].shape[0], []).append(i)
    assert sorted(by_S) == [2, 3, 16, 33] and {"saturated_S16", "constant_S33", "one_run_S16", "two_runs_S33"} <= set(names)
    bound = float(fx["std_bound_units"])
    for S, idx in by_S.items():
        crops = [fx[f"std_in_{i}"] for i in idx]
        u16, f32, stats = _identity_call(crops, out=("uint16", "float32"), return_stats=True)
        assert f32.shape == (len(crops), 1, S, S) and stats.shape == (len(crops), 2) and stats.dtype == torch.float32
        _check_standardised(crops, f32, stats, u16)
        for k, i in enumerate(idx):
            if names[i].startswith("constant"):
                assert torch.all(f32[k] == 0.0) and stats[k, 1].item() == 0.0
            # and upstream's recorded output, within the bound of the CPU test (upstream sums in fp32)
            s = float(np.sqrt(np.float32(stats[k, 1].item()) + np.float32(1e-6)))
            allowed = 4.0 * bound * 2.0 ** -24 * float(U.unit_f32(crops[k]).max()) / s + 2 * 2.0 ** -23 * float(np.abs(fx[f"std_out_{i}"]).max())
            assert float(np.max(np.abs(f32[k, 0].cpu().numpy().astype(np.float64) - fx[f"std_out_{i}"]))) <= allowed, names[i]


def test_standardised_crops_of_a_resize(seeded):
    """The whole path - resize, then statistics over the resized values - at S = 64 (4096 values, four per thread) and S = 33."""
    for S in (33, 64):
        images, settings, want = _want(seeded, S, "bicubic")
        u16, f32, stats = _run(images, settings, S, "bicubic", out=("uint16", "float32"), return_stats=True)
        _check_standardised(list(want.astype(np.uint16)), f32, stats, u16)
        only = _run(images, settings, S, "bicubic", out="float32")          # without the integer output or the statistics
        assert torch.equal(only, f32)


def test_two_calls_and_another_order_give_the_same_bits(seeded):
    images, settings, _ = _want(seeded, 33, "bicubic")
    a_u, a_f, a_s = _run(images, settings, 33, "bicubic", out=("uint16", "float32"), return_stats=True)
    b_u, b_f, b_s = _run(images, settings, 33, "bicubic", out=("uint16", "float32"), return_stats=True)
    assert torch.equal(a_u, b_u) and torch.equal(a_f.view(torch.int32), b_f.view(torch.int32)) and torch.equal(a_s.view(torch.int32), b_s.view(torch.int32))
    r_u, r_f, r_s = _run(images[::-1], [st[::-1] for st in settings[::-1]], 33, "bicubic", out=("uint16", "float32"), return_stats=True)
    assert torch.equal(a_u, r_u.flip(0)) and torch.equal(a_f.view(torch.int32), r_f.flip(0).view(torch.int32))
    assert torch.equal(a_s.view(torch.int32), r_s.flip(0).view(torch.int32))
    s2 = torch.cuda.Stream()          # a side stream with its own workspace, tensors as input
    s2.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s2):
        side = _run([torch.from_numpy(im) for im in images], settings, 33, "bicubic", out="float32")
    s2.synchronize()
    assert torch.equal(a_f.view(torch.int32), side.view(torch.int32))


def test_box_outside_the_image_raises_before_any_launch():
    from fourm.data import crops
    from fourm.hip import _lib as L
    img = np.zeros((20, 30), np.uint16)
    calls = []
    real = L.pil_crop_resize16
    L.pil_crop_resize16 = lambda *a: calls.append(a) or real(*a)
    try:
        for bad in ([0, 0, 21, 5, 0], [0, 26, 5, 5, 1], [-1, 0, 5, 5, 0], [16, 0, 5, 5, 0]):
            with pytest.raises(ValueError, match="leaves the 20 x 30 image"):
                crops.crop_resize_depth([img], [np.array([[0, 0, 5, 5, 0], bad])], 8)
        with pytest.raises(ValueError, match="fewer than two elements"):
            crops.crop_resize_depth([img], [np.array([[0, 0, 5, 5, 0]])], 1)
        assert not calls
        crops.crop_resize_depth([img], [np.array([[15, 25, 5, 5, 1]])], 8)
        assert len(calls) == 1
    finally:
        L.pil_crop_resize16 = real


def test_crop_modalities_is_the_single_modality_calls_and_feeds_prepare_inputs():
    from fourm.data.crops import crop_resize, crop_resize_depth
    from fourm.data.multimodal_crops import crop_modalities
    from fourm.vq.training import mask_out_samples, prepare_inputs
    rng = np.random.default_rng(8)
    shapes = [(40, 64), (77, 31)]
    settings = [np.array([(0, 12, 40, 40, 0), (5, 9, 31, 44, 1)]), np.array([(3, 0, 60, 31, 1), (0, 0, 77, 31, 0), (20, 4, 16, 16, 1)])]
    samples = {
        "rgb": [rng.integers(0, 256, (*s, 3), dtype=np.uint8) for s in shapes],
        "normal": [rng.integers(0, 256, (*s, 3), dtype=np.uint8) for s in shapes],
        "depth": [rng.integers(0, 65536, s, dtype=np.uint16) for s in shapes],
        "semseg_coco": [rng.integers(0, 134, s, dtype=np.uint8) for s in shapes],
        "mask_valid": [(rng.integers(0, 4, shapes[0]) > 0).astype(np.uint8) * np.uint8(255), rng.integers(0, 4, shapes[1]) > 0],          # mode L, mode 1
    }
    samples["mask_valid"][0][3, 20] = 254          # not 255: invalid, as to_tensor(...) == 1.0 has it
    S, half = 16, (0.5, 0.5, 0.5)
    got = crop_modalities(samples, settings, S, resample_mode="bilinear")
    assert set(got) == set(samples)
    assert torch.equal(got["rgb"], crop_resize(samples["rgb"], settings, S, resample="bilinear", mean=half, std=half))
    assert torch.equal(got["normal"], crop_resize(samples["normal"], settings, S, resample="bilinear", mean=half, std=half, invert_on_flip=(0,)))
    assert torch.equal(got["depth"], crop_resize_depth(samples["depth"], settings, S, resample="bilinear"))
    assert torch.equal(got["semseg_coco"], crop_resize(samples["semseg_coco"], settings, S, resample="nearest", out="int64"))
    masks_u8 = [samples["mask_valid"][0], samples["mask_valid"][1].astype(np.uint8) * np.uint8(255)]
    u8 = crop_resize(masks_u8, settings, S, resample="nearest", out="uint8")
    assert got["mask_valid"].dtype == torch.bool and got["mask_valid"].shape == (5, 1, S, S)
    assert torch.equal(got["mask_valid"], (u8 == 255).permute(0, 3, 1, 2))
    k = 0
    for m, st in zip(masks_u8, settings):          # and the restatement of the 8-bit path
        for s in st:
            assert np.array_equal(got["mask_valid"][k, 0].cpu().numpy(), U8.crop_resize(m[:, :, None], s, S, "nearest")[..., 0] == 255)
            k += 1
    assert got["rgb"].shape == (5, 3, S, S) and got["depth"].shape == (5, 1, S, S) and got["semseg_coco"].shape == (5, S, S)
    assert got["semseg_coco"].dtype == torch.int64 and 0 < got["mask_valid"].sum().item() < got["mask_valid"].numel()
    for domain in ("rgb", "depth", "normal"):
        clean = got[domain].clone()
        out = prepare_inputs({k: (v.clone() if torch.is_tensor(v) else v) for k, v in got.items()}, domain, None, "cuda", mask_value=0.0)
        want = mask_out_samples(clean, got["mask_valid"], mask_value=0.0)
        assert out.shape == (5, clean.shape[1] + 1, S, S) and torch.equal(out, want)
        assert torch.all(out[:, :-1][~got["mask_valid"].expand(-1, clean.shape[1], -1, -1)] == 0.0)
        assert torch.equal(out[:, -1:] > 0, got["mask_valid"])
