"""fourm.data.crops.crop_resize on the GPU against Pillow's recorded bytes (tests/golden/pil_crops.npz) and against the numpy restatement
(tests/pil_resize_util.py): equal bytes, no tolerance.  Pillow is not needed here."""
import os

import numpy as np
import pytest
import torch

from tests import pil_resize_util as U

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "pil_crops.npz")


def _run(images, settings, S, filt, **kw):
    from fourm.data.crops import crop_resize
    kw.setdefault("out", "uint8")
    return crop_resize(images, [np.asarray(s).reshape(-1, 5) for s in settings], S, resample=filt, **kw)


@pytest.fixture(scope="module")
def fx():
    f = np.load(GOLDEN)
    return {k: f[k] for k in f.files}


def test_fixture_cases_equal_pillows_bytes(fx):
    """Every recorded case, one call per case - and all cases of one (source, S, filter, invert) in a single call as well."""
    src = [fx[f"src_{k}"] for k in range(6)]
    names = fx["names"].tolist()
    groups = {}
    for i, (k, top, left, h, w, flip, S, f, inv) in enumerate(fx["cases"].tolist()):
        got = _run([src[k]], [(top, left, h, w, flip)], S, U.FILTERS[f], invert_on_flip=(0,) if inv else ())
        assert got.shape == (1, S, S, src[k].shape[2]) and got.dtype == torch.uint8
        assert np.array_equal(got[0].cpu().numpy(), fx[f"out_{i}"]), names[i]
        groups.setdefault((k, S, f, inv), []).append((i, (top, left, h, w, flip)))
    for (k, S, f, inv), members in groups.items():
        got = _run([src[k]], [[m[1] for m in members]], S, U.FILTERS[f], invert_on_flip=(0,) if inv else ()).cpu().numpy()
        for row, (i, _) in zip(got, members):
            assert np.array_equal(row, fx[f"out_{i}"]), names[i]
    for must in ("up_5x7_bicubic", "down_90x17_bicubic", "h_eq_S", "w_eq_S", "edge_top", "edge_left", "edge_bottom", "edge_right", "S1_bicubic",
                 "checkerboard_up", "normal_invert_flip"):
        assert must in names
    i = names.index("checkerboard_up")
    assert fx[f"out_{i}"].min() == 0 and fx[f"out_{i}"].max() == 255


@pytest.mark.parametrize("filt", U.FILTERS + (None,))
@pytest.mark.parametrize("C", [1, 2, 3, 4])
def test_seeded_cases_equal_the_restatement(filt, C):
    """Odd image sizes, both flips, boxes from one pixel to the whole image, more than one workgroup per crop (S * S > 256)."""
    rng = np.random.default_rng(100 * C + len(str(filt)))
    for S in (1, 7, 24):
        images, settings = [], []
        for it in range(4):
            H, W = int(rng.integers(1, 75)), int(rng.integers(1, 75))
            images.append(rng.integers(0, 256, (H, W, C), dtype=np.uint8) if it else (rng.integers(0, 2, (H, W, C)) * 255).astype(np.uint8))
            st = []
            for _ in range(3):
                h, w = int(rng.integers(1, H + 1)), int(rng.integers(1, W + 1))
                st.append((int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1)), h, w, int(rng.integers(0, 2))))
            st.append((0, 0, H, W, it % 2))
            settings.append(st)
        got = _run(images, settings, S, filt, invert_on_flip=(C - 1,)).cpu().numpy()
        k = 0
        for im, st in zip(images, settings):
            for s in st:
                assert np.array_equal(got[k], U.crop_resize(im, s, S, filt or "bicubic", (C - 1,))), (im.shape, s, S, filt)
                k += 1
        assert k == got.shape[0]


def test_large_downscale_and_224_targets():
    """The shapes of real use: a 480 x 640 source to 224 with each filter (tables of up to 13 taps, 196 workgroups per crop), and a whole
    400 x 300 image to 8 with bicubic (tables of 200 taps)."""
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (480, 640, 3), dtype=np.uint8)
    st = [(0, 80, 480, 480, 0), (37, 101, 333, 419, 1)]
    for filt in U.FILTERS:
        got = _run([img], [st], 224, filt).cpu().numpy()
        for g, s in zip(got, st):
            assert np.array_equal(g, U.crop_resize(img, s, 224, filt)), (filt, s)
    small = rng.integers(0, 256, (400, 300, 3), dtype=np.uint8)
    assert np.array_equal(_run([small], [(0, 0, 400, 300, 1)], 8, "bicubic")[0].cpu().numpy(), U.crop_resize(small, (0, 0, 400, 300, 1), 8, "bicubic"))


def test_one_call_with_many_images_equals_separate_calls():
    from fourm.data.crops import make_crop_settings
    rng = np.random.default_rng(5)
    torch.manual_seed(0)
    images = [rng.integers(0, 256, s, dtype=np.uint8) for s in ((40, 64, 3), (77, 31, 3), (96, 96, 3))]
    settings = [make_crop_settings(im.shape[0], im.shape[1], n, 0.2) for im, n in zip(images, (1, 4, 10))]
    assert [len(s) for s in settings] == [1, 4, 10]
    together = _run(images, settings, 20, "bicubic")
    assert together.shape == (15, 20, 20, 3)
    k = 0
    for im, st in zip(images, settings):
        for s in st:
            alone = _run([im], [s], 20, "bicubic")
            assert torch.equal(together[k], alone[0]), (im.shape, s)
            assert np.array_equal(alone[0].cpu().numpy(), U.crop_resize(im, s, 20, "bicubic")), (im.shape, s)
            k += 1
    again = _run(images, settings, 20, "bicubic")
    assert torch.equal(together, again)          # two calls, the same bytes
    # tensors as input, and a side stream with its own workspace
    s2 = torch.cuda.Stream()
    s2.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s2):
        side = _run([torch.from_numpy(im) for im in images], settings, 20, "bicubic")
    s2.synchronize()
    assert torch.equal(together, side)


def test_float32_output_is_the_lookup_table_of_the_bytes():
    from fourm.data.crops import crop_resize, normalize_lut
    rng = np.random.default_rng(6)
    img = rng.integers(0, 256, (50, 70, 3), dtype=np.uint8)
    st = np.array([(0, 0, 50, 70, 0), (5, 9, 31, 44, 1), (10, 10, 16, 16, 1)])
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    u8, f32 = crop_resize([img], [st], 16, resample="bilinear", mean=mean, std=std, invert_on_flip=(0,), out=("uint8", "float32"))
    assert f32.shape == (3, 3, 16, 16) and f32.dtype == torch.float32 and f32.is_contiguous()
    lut = normalize_lut(3, mean, std).cuda()
    want = torch.stack([lut[c][u8[..., c].long()] for c in range(3)], dim=1)
    assert torch.equal(f32, want)
    # what to_tensor + normalize compute from the same bytes on the host, with torch's own ops
    t = u8.cpu().permute(0, 3, 1, 2).contiguous().to(torch.float32).div(255)
    ref = t.clone().sub_(torch.tensor(mean)[None, :, None, None]).div_(torch.tensor(std)[None, :, None, None])
    assert torch.equal(f32.cpu(), ref)
    only = crop_resize([img], [st], 16, resample="bilinear", mean=mean, std=std, invert_on_flip=(0,))
    assert torch.equal(only, f32)
    for k, s in enumerate(st):
        assert np.array_equal(u8[k].cpu().numpy(), U.crop_resize(img, s, 16, "bilinear", (0,)))
    b, plain = crop_resize([img], [st], 16, resample="bilinear", out=("uint8", "float32"))          # no statistics: byte / 255, to_tensor alone
    assert torch.equal(plain.cpu(), b.cpu().permute(0, 3, 1, 2).contiguous().to(torch.float32).div(255))


def test_int64_class_maps():
    from fourm.data.crops import crop_resize
    rng = np.random.default_rng(7)
    seg = rng.integers(0, 256, (45, 61, 1), dtype=np.uint8)
    st = np.array([(0, 0, 45, 61, 0), (3, 4, 40, 50, 1), (0, 11, 45, 45, 1)])
    got = crop_resize([seg, seg[:, :, 0]], [st, st[:1]], 32, resample="nearest", out="int64")
    assert got.shape == (4, 32, 32) and got.dtype == torch.int64
    for k, s in enumerate(list(st) + [st[0]]):
        assert np.array_equal(got[k].cpu().numpy(), U.crop_resize(seg, s, 32, "nearest")[..., 0].astype(np.int64))
    with pytest.raises(ValueError, match="int64"):
        crop_resize([seg], [st], 32, resample="bicubic", out="int64")


def test_box_outside_the_image_raises_before_any_launch():
    from fourm.data import crops
    from fourm.hip import _lib as L
    img = np.zeros((20, 30, 3), np.uint8)
    calls = []
    real = L.pil_crop_resize
    L.pil_crop_resize = lambda *a: calls.append(a) or real(*a)
    try:
        for bad in ([0, 0, 21, 5, 0], [0, 26, 5, 5, 1], [-1, 0, 5, 5, 0], [16, 0, 5, 5, 0]):
            with pytest.raises(ValueError, match="leaves the 20 x 30 image"):
                crops.crop_resize([img], [np.array([[0, 0, 5, 5, 0], bad])], 8)
        assert not calls
        crops.crop_resize([img], [np.array([[15, 25, 5, 5, 1]])], 8)
        assert len(calls) == 1
    finally:
        L.pil_crop_resize = real
    with pytest.raises(RuntimeError, match="leaves the 20 x 30 image"):          # the library's own check of the host job list
        j = (L.PilCropJob * 1)()
        j[0].H, j[0].W, j[0].top, j[0].h, j[0].w, j[0].taps_w, j[0].taps_h, j[0].blk_rows = 20, 30, 16, 5, 5, 1, 1, 7
        d = torch.zeros(4096, dtype=torch.uint8, device="cuda")
        p = L.vp(d.data_ptr())
        L.check(L.pil_crop_resize(j, p, 1, p, 1800, p, 48, p, 4096, 3, 8, 0, None, p, None, None, 1, None))
