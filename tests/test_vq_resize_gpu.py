"""The image resize on a real MI355X (fourm.vq.resize, csrc/resize.hip) against F.interpolate in float64 on the CPU, element by element, within
the derived bound of tests/vq_resize_util.py: forward and adjoint of both bilinear modes with and without a per-channel affine, nearest on fp32
and int64 exactly; outputs inside sentinel buffers, two calls bit-identical; autograd; prepare_inputs and perceptual_loss of fourm.vq.training."""
import pytest
import torch
import torch.nn.functional as F

from tests import vq_metrics_util as MU
from tests import vq_resize_util as RU
from tests.parity_log import record

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = -7.0


def _ops():
    from fourm.hip import _lib as L, ops
    return L, ops


def _tables(in_size, out_size, antialias):
    from fourm.vq.resize import axis_table
    L, _ = _ops()
    mode = L.RESIZE_BILINEAR_AA if antialias else L.RESIZE_BILINEAR
    return axis_table(in_size[0], out_size[0], mode, DEV), axis_table(in_size[1], out_size[1], mode, DEV)


def _affine(C, on):
    if not on:
        return None, None
    return RU.affine_vectors(C, 77 + C)


@pytest.fixture(scope="module")
def refs():
    """Per (shape, antialias): the fp32 input and incoming gradient and their float64 resize / adjoint, of the values and of the absolute
    values (the bound); computed once, never modified."""
    out = {}
    for bc, in_size, out_size in RU.SHAPES + RU.EXTRA_SHAPES:
        for aa in (False, True):
            g = RU.gen(100 * in_size[0] + out_size[1] + aa)
            x = torch.randn(*bc, *in_size, generator=g).float()
            dy = torch.randn(*bc, *out_size, generator=g).float()
            out[bc, in_size, out_size, aa] = dict(x=x, dy=dy, y=RU.interp64(x, out_size, aa), y_abs=RU.interp64(x.abs(), out_size, aa),
                                                  dx=RU.adjoint64(dy, in_size, aa), dx_abs=RU.adjoint64(dy.abs(), in_size, aa))
    return out


def _check(got, ref, bound, what, **tags):
    err = (got.double().cpu() - ref).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max()) if bool((bound > 0).any()) else 0.0
    assert bool((err[bound == 0] == 0).all()), f"{what}: an element with a zero bound is off"
    print(f"{what} {tags}: max |err| {float(err.max()):.3e}, max err / bound {ratio:.3f}")
    record(what, max_err=float(err.max()), max_err_over_bound=ratio, **tags)
    assert bool((err <= bound).all()), (what, tags, ratio)


@pytest.mark.parametrize("affine", [False, True], ids=["plain", "affine"])
@pytest.mark.parametrize("antialias", [False, True], ids=["bilinear", "antialias"])
@pytest.mark.parametrize("shape", RU.SHAPES + RU.EXTRA_SHAPES, ids=RU.shape_id)
def test_forward_against_float64(shape, antialias, affine, refs):
    """|got - ref| <= (T_h + T_w + 4) 2^-24 R(|x|) per element (with an affine: times |a_c|, plus 2^-23 |ref|); nothing written outside y; a
    second call gives the same bits."""
    _, ops = _ops()
    bc, in_size, out_size = shape
    r = refs[bc, in_size, out_size, antialias]
    th, tw = _tables(in_size, out_size, antialias)
    a, b = _affine(bc[1], affine)
    ref, bound = r["y"], (th["taps"] + tw["taps"] + 4) * RU.U * r["y_abs"]
    if affine:
        ref = a.double().view(1, -1, 1, 1) * ref + b.double().view(1, -1, 1, 1)
        bound = bound * a.double().abs().view(1, -1, 1, 1) + 2.0 ** -23 * ref.abs()
    x = r["x"].to(DEV)
    ad, bd = (a.to(DEV), b.to(DEV)) if affine else (None, None)
    outs = []
    for _ in range(2):
        buf, y = MU.sentinel_view((*bc, *out_size), torch.float32, DEV, SENTINEL)
        ops.resize_bilinear_fwd(x, y, th, tw, ad, bd)
        assert MU.sentinels_intact(buf, y.numel(), SENTINEL), "fm_resize_bilinear_fwd wrote outside y"
        outs.append(y.clone())
    assert torch.equal(outs[0], outs[1]), "two runs differ"
    _check(outs[0], ref, bound, "resize.fwd", shape=RU.shape_id(shape), antialias=antialias, affine=affine)


@pytest.mark.parametrize("affine", [False, True], ids=["plain", "affine"])
@pytest.mark.parametrize("antialias", [False, True], ids=["bilinear", "antialias"])
@pytest.mark.parametrize("shape", RU.SHAPES + RU.EXTRA_SHAPES, ids=RU.shape_id)
def test_adjoint_against_float64(shape, antialias, affine, refs):
    """dx = a R^T(dy) against the autograd gradient of F.interpolate in float64 for a random dy: the same bound with R^T(|dy|) and the
    transposed tap counts (times |a_c| with an affine; one more rounding, inside the + 4); sentinels; two calls, the same bits."""
    _, ops = _ops()
    bc, in_size, out_size = shape
    r = refs[bc, in_size, out_size, antialias]
    th, tw = _tables(in_size, out_size, antialias)
    a, _ = _affine(bc[1], affine)
    ref, bound = r["dx"], (th["t_taps"] + tw["t_taps"] + 4) * RU.U * r["dx_abs"]
    if affine:
        ref = a.double().view(1, -1, 1, 1) * ref
        bound = bound * a.double().abs().view(1, -1, 1, 1)
    dy = r["dy"].to(DEV)
    outs = []
    for _ in range(2):
        buf, dx = MU.sentinel_view((*bc, *in_size), torch.float32, DEV, SENTINEL)
        ops.resize_bilinear_bwd(dy, dx, th, tw, a.to(DEV) if affine else None)
        assert MU.sentinels_intact(buf, dx.numel(), SENTINEL), "fm_resize_bilinear_bwd wrote outside dx"
        outs.append(dx.clone())
    assert torch.equal(outs[0], outs[1]), "two runs differ"
    _check(outs[0], ref, bound, "resize.bwd", shape=RU.shape_id(shape), antialias=antialias, affine=affine)


@pytest.mark.parametrize("shape", RU.SHAPES[:5], ids=RU.shape_id)
def test_nearest_is_exact(shape):
    """fp32 (B, C, H, W) and int64 (B, H, W) class maps with values up to 2^40 (exact in the float64 reference): torch.equal with
    F.interpolate(mode='nearest'); sentinels around the raw kernel's output."""
    from fourm.vq.resize import axis_table, resize_images
    L, ops = _ops()
    bc, in_size, out_size = shape
    g = RU.gen(5 + in_size[0])
    x = torch.randn(*bc, *in_size, generator=g).float()
    m = torch.randint(0, 2 ** 40, (bc[0] * bc[1], *in_size), generator=g, dtype=torch.int64)
    m.view(-1)[0] = 2 ** 40
    assert torch.equal(resize_images(x.to(DEV), out_size, mode="nearest").cpu(), F.interpolate(x, out_size, mode="nearest"))
    got = resize_images(m.to(DEV), out_size, mode="nearest")
    assert got.dtype == torch.int64 and torch.equal(got.cpu(), F.interpolate(m.double().unsqueeze(1), out_size, mode="nearest").squeeze(1).long())
    ih, iw = (axis_table(in_size[k], out_size[k], L.RESIZE_NEAREST, DEV)["start"] for k in (0, 1))
    buf, y = MU.sentinel_view((m.shape[0], *out_size), torch.int64, DEV, -7)
    ops.resize_nearest(m.to(DEV), y, ih, iw)
    assert MU.sentinels_intact(buf, y.numel(), -7) and torch.equal(y, got)


def test_autograd_runs_the_adjoint_kernel():
    """resize_images(x.requires_grad_()).backward(g) leaves in x.grad exactly the bits of a direct adjoint call, with and without an affine;
    the input's own size without an affine returns the input."""
    from fourm.vq.resize import resize_images
    _, ops = _ops()
    g = RU.gen(3)
    x = torch.randn(2, 3, 37, 53, generator=g).to(DEV)
    gy = torch.randn(2, 3, 16, 24, generator=g).to(DEV)
    a, b = (v.to(DEV) for v in RU.affine_vectors(3, 8))
    for aa in (False, True):
        th, tw = _tables((37, 53), (16, 24), aa)
        for sc, sh in ((None, None), (a, b)):
            xr = x.clone().requires_grad_()
            y = resize_images(xr, (16, 24), antialias=aa, scale=sc, shift=sh)
            assert y.requires_grad and y.shape == (2, 3, 16, 24)
            y.backward(gy)
            direct = ops.resize_bilinear_bwd(gy, torch.empty_like(x), th, tw, sc)
            assert torch.equal(xr.grad, direct)
            assert torch.equal(y.detach(), ops.resize_bilinear_fwd(x, torch.empty_like(y), th, tw, sc, sh))
    assert resize_images(x, (37, 53)) is x and resize_images(x, (37, 53), antialias=True) is x
    same = resize_images(x, (37, 53), scale=a, shift=b)
    ref = a.double().cpu().view(1, -1, 1, 1) * x.double().cpu() + b.double().cpu().view(1, -1, 1, 1)
    assert bool(((same.double().cpu() - ref).abs() <= 2.0 ** -23 * ref.abs()).all())


# ---- prepare_inputs ---------------------------------------------------------------------------------------------------------------------------
def test_prepare_inputs_rgb_and_masking():
    """An rgb dict at 48 px with image_size=32 equals resize_images; with mask_valid and mask_value the result is mask_out_samples of the
    resized images, bit for bit."""
    from fourm.vq import training as T
    g = RU.gen(21)
    rgb = torch.randn(3, 3, 48, 48, generator=g)
    want = T.resize_images(rgb.to(DEV), 32)
    got = T.prepare_inputs({"rgb": rgb}, "rgb", None, DEV, image_size=32)
    assert got.shape == (3, 3, 32, 32) and got.is_cuda and torch.equal(got, want)
    valid = torch.rand(3, 1, 32, 32, generator=g) < 0.7
    masked = T.prepare_inputs({"rgb": rgb, "mask_valid": valid}, "rgb", None, DEV, image_size=32, mask_value=0.25)
    assert masked.shape == (3, 4, 32, 32) and torch.equal(masked, T.mask_out_samples(want.clone(), valid, 0.25))
    assert torch.equal(T.prepare_inputs({"rgb": rgb, "mask_valid": valid}, "rgb", None, DEV, image_size=32), want)          # no mask_value: no masking
    # a feature domain without an extractor reads the RGB
    assert torch.equal(T.prepare_inputs({"rgb": rgb}, "CLIP-B16", None, DEV, image_size=32), want)


def test_prepare_inputs_semseg_and_sam_mask():
    """A semseg int64 map goes through the nearest rule and keeps its dtype; a sam_mask dict with some invalid instances returns only the valid
    ones, unresized."""
    from fourm.vq import training as T
    g = RU.gen(22)
    seg = torch.randint(0, 134, (2, 48, 48), generator=g, dtype=torch.int64)
    got = T.prepare_inputs({"semseg_coco": seg}, "semseg_coco", None, DEV, image_size=32)
    want = F.interpolate(seg.unsqueeze(1).float(), 32, mode="nearest").to(seg.dtype).squeeze(1)
    assert got.dtype == torch.int64 and got.is_cuda and torch.equal(got.cpu(), want)
    seg32 = seg.to(torch.int32)
    got32 = T.prepare_inputs({"semseg_coco": seg32}, "semseg_coco", None, DEV, image_size=(24, 40))
    assert got32.dtype == torch.int32 and torch.equal(got32.cpu(), F.interpolate(seg.unsqueeze(1).float(), (24, 40), mode="nearest").to(torch.int32).squeeze(1))
    inst = torch.rand(2, 3, 16, 16, generator=g)
    valid = torch.tensor([[True, False, True], [False, False, True]])
    out = T.prepare_inputs({"sam_mask": dict(instance=inst, valid=valid)}, "sam_mask", None, DEV, image_size=8)
    assert out.is_cuda and out.shape == (3, 1, 16, 16) and torch.equal(out.cpu(), inst.flatten(end_dim=1)[valid.flatten()].unsqueeze(1))
    poses = torch.randn(2, 7, generator=g)
    assert torch.equal(T.prepare_inputs({"human_poses": poses}, "human_poses", None, DEV, image_size=8).cpu(), poses[:, :, None, None])


# ---- perceptual_loss --------------------------------------------------------------------------------------------------------------------------
def _clip_loss(precision="fp32"):
    from fourm.utils.clip.model import VisionTransformer
    from fourm.vq.percept_losses import ClipPerceptualLoss
    from tests import clip_util as CU
    vis = VisionTransformer(**CU.CASES["clip_a"])
    vis.load_state_dict(CU.seeded_state_dict("clip_a"), strict=True)
    vis.compute_precision = precision
    return ClipPerceptualLoss(vis, "blocks.0-blocks.1", feature_loss="cosine").to(DEV)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_perceptual_loss_at_another_resolution(precision):
    """The clip_a tower (resolution 32) on 48 x 48 predictions and images.  The value is loss(resized_p, resized_t).mean() of tensors resized
    beforehand by resize_images(..., antialias=True, scale, shift), bit for bit; the gradient at the 48 x 48 predictions is the direct adjoint
    of the gradient the loss returns at its 32 x 32 input, bit for bit.  Both pieces that this adds - the transformed tensors and the adjoint
    of that gradient - are within the derived bound of the float64 composition a R(x) + b / a R^T(g) (the tower itself is compared with
    float64 by tests/test_clip_percept_gpu.py)."""
    from fourm.vq import training as T
    _, ops = _ops()
    mod = _clip_loss(precision)
    g = RU.gen(31)
    t48 = (0.5 * torch.randn(2, 3, 48, 48, generator=g)).clamp(-1, 1)
    p48 = (t48 + 0.2 * torch.randn(2, 3, 48, 48, generator=g)).float()
    with pytest.raises(NotImplementedError, match="resize before the loss"):
        mod(p48.to(DEV), t48.to(DEV))
    p = p48.to(DEV).requires_grad_()
    value = T.perceptual_loss(mod, p, t48.to(DEV))
    assert value.dim() == 0 and value.dtype == torch.float32
    value.backward()
    # by hand
    rp = T.resize_images(p48.to(DEV), 32, antialias=True, scale=mod._scale, shift=mod._shift).requires_grad_()
    rt = T.resize_images(t48.to(DEV), 32, antialias=True, scale=mod._scale, shift=mod._shift)
    by_hand = mod(rp, rt).mean()
    by_hand.backward()
    assert torch.equal(value.detach(), by_hand.detach())
    th, tw = _tables((48, 48), (32, 32), True)
    direct = ops.resize_bilinear_bwd(rp.grad.contiguous(), torch.empty(2, 3, 48, 48, device=DEV), th, tw, mod._scale)
    assert torch.equal(p.grad, direct) and float(p.grad.abs().max()) > 0
    # the float64 composition
    a, b = mod._scale.double().cpu().view(1, -1, 1, 1), mod._shift.double().cpu().view(1, -1, 1, 1)
    ref = a * RU.interp64(p48, (32, 32), True) + b
    bound = (th["taps"] + tw["taps"] + 4) * RU.U * RU.interp64(p48.abs(), (32, 32), True) * a.abs() + 2.0 ** -23 * ref.abs()
    _check(rp.detach(), ref, bound, "resize.percept.transform", precision=precision)
    g32 = rp.grad.cpu()
    ref_g = a * RU.adjoint64(g32, (48, 48), True)
    bound_g = (th["t_taps"] + tw["t_taps"] + 4) * RU.U * RU.adjoint64(g32.abs(), (48, 48), True) * a.abs()
    _check(p.grad, ref_g, bound_g, "resize.percept.grad", precision=precision)


def test_perceptual_loss_at_the_towers_resolution():
    """At 32 x 32 the result is today's loss(percept_transform(p), percept_transform(t)).mean(), value and gradient."""
    from fourm.vq import training as T
    from tests import clip_util as CU
    mod = _clip_loss("bf16")
    t = CU.images("clip_a", "native").clamp(-1, 1).to(DEV)
    p0 = (t + 0.1).clamp(-1, 1)
    p1, p2 = p0.clone().requires_grad_(), p0.clone().requires_grad_()
    v1 = T.perceptual_loss(mod, p1, t)
    v1.backward()
    v2 = mod(mod.percept_transform(p2), mod.percept_transform(t)).mean()
    v2.backward()
    assert torch.equal(v1.detach(), v2.detach()) and torch.equal(p1.grad, p2.grad)
