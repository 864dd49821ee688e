"""The LPIPS validation metric end to end on the GPU: LpipsAlex.scores and LearnedPerceptualImagePatchSimilarity against the float64
restatement (tests/lpips_metric_util.py), the bit properties (zero, symmetry, batch and chunk invariance, additive state) and the opt-in use
from ReconstructionMetrics."""
import math

import pytest
import torch

from tests import lpips_metric_util as MU
from tests import parity_log

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(4, 64, 64), (2, 33, 46)]


@pytest.fixture(scope="module")
def net():
    from fourm.vq.percept_losses.lpips_alex import LpipsAlex
    return LpipsAlex(MU.seeded_state_dict()).to(DEV)


def _metric(net, **kw):
    from fourm.vq.metrics import LearnedPerceptualImagePatchSimilarity
    return LearnedPerceptualImagePatchSimilarity(net=net, **kw)


@pytest.mark.parametrize("normalize", [False, True], ids=["raw", "normalize"])
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_scores_and_metric_match_the_float64_restatement(net, B, H, W, normalize):
    fx = MU.fixture(B, H, W, normalize)
    a, b = fx["img0"].to(DEV), fx["img1"].to(DEV)
    got = net.scores(a, b, normalize)
    assert got.dtype == torch.float32 and tuple(got.shape) == (B,)
    tol, base = MU.tol(fx["ref64"], fx["ref32"])
    err = (got.cpu().double() - fx["ref64"]).abs()
    print(f"scores {B}x{H}x{W} normalize={normalize}: err {float(err.max()):.3e}, fp32 restatement {base:.3e}, bound {tol:.3e}, values {fx['ref64'].tolist()}")
    parity_log.record("test_scores_and_metric_match_the_float64_restatement", shape=[B, H, W], normalize=normalize, err=float(err.max()), fp32_restatement=base,
                      bound=tol, ratio=float(err.max()) / base if base else None)
    assert bool((err <= tol).all()), (err.tolist(), base, tol)
    assert torch.equal(net(a, b, normalize), got)
    for reduction in ("mean", "sum"):
        m = _metric(net, reduction=reduction, normalize=normalize)
        m.update(a, b)
        val = m.compute()
        assert val.dtype == torch.float32 and val.dim() == 0
        want = fx["ref64"].sum() / (B if reduction == "mean" else 1)
        scale = 1.0 if reduction == "mean" else float(B)
        assert abs(float(val) - float(want)) <= scale * tol + 2.0 ** -23 * abs(float(want)), (reduction, float(val), float(want))      # + the rounding of compute()
        # the state is the row-ordered float64 sum of the fp32 scores, exactly
        acc = 0.0
        for s in got.cpu().tolist():
            acc += s
        assert float(m.sum_scores[0]) == acc and int(m.total[0]) == B and m.sum_scores.dtype == torch.float64 and m.total.dtype == torch.int64


def test_bf16_input_equals_its_fp32_upcast(net):
    fx = MU.fixture(2, 33, 46, False)
    a, b = fx["img0"].to(DEV).bfloat16(), fx["img1"].to(DEV).bfloat16()
    assert torch.equal(net.scores(a, b, False), net.scores(a.float(), b.float(), False))
    h = fx["img0"].to(DEV).half()
    assert torch.equal(net.scores(h, b, False), net.scores(h.float(), b.float(), False))


def test_identical_pairs_are_exactly_zero_and_swapping_changes_no_bit(net):
    for B, H, W in SHAPES:
        fx = MU.fixture(B, H, W, False)
        a, b = fx["img0"].to(DEV), fx["img1"].to(DEV)
        assert bool((net.scores(a, a.clone(), False) == 0.0).all())
        ab, ba = net.scores(a, b, False), net.scores(b, a, False)
        assert torch.equal(ab, ba) and bool((ab > 0).all())
    m = _metric(net)
    m.update(a, a)
    assert float(m.compute()) == 0.0


def test_a_score_does_not_depend_on_the_batch_or_the_chunking(net):
    fx = MU.fixture(4, 64, 64, False)
    a, b = fx["img0"].to(DEV), fx["img1"].to(DEV)
    full = net.scores(a, b, False)
    for i in (0, 2, 3):
        assert torch.equal(net.scores(a[i:i + 1], b[i:i + 1], False)[0], full[i]), i
    for chunk in (1, 3, 4, 64):
        assert torch.equal(net.scores(a, b, False, chunk=chunk), full), chunk
    assert torch.equal(net.scores(a.flip(0), b.flip(0), False), full.flip(0))
    again = net.scores(a, b, False)
    assert torch.equal(again, full)


def test_two_plus_two_updates_equal_one_of_four_in_state_bits(net):
    fx = MU.fixture(4, 64, 64, True)
    a, b = fx["img0"].to(DEV), fx["img1"].to(DEV)
    one, two = _metric(net, normalize=True), _metric(net, normalize=True)
    one.update(a, b)
    two.update(a[:2], b[:2])
    two.update(a[2:], b[2:])
    assert torch.equal(one.sum_scores, two.sum_scores) and torch.equal(one.total, two.total) and int(two.total) == 4
    assert torch.equal(one.compute(), two.compute())
    assert one.sum_scores.is_cuda and one.total.is_cuda


def test_reset_to_and_empty():
    from fourm.vq.percept_losses.lpips_alex import LpipsAlex
    net = LpipsAlex(MU.seeded_state_dict()).to(DEV)                    # its own network: .to() moves it
    fx = MU.fixture(2, 33, 46, False)
    a, b = fx["img0"].to(DEV), fx["img1"].to(DEV)
    m = _metric(net)
    assert math.isnan(float(m.compute()))
    m.update(a, b)
    first = m.compute()
    assert float(first) > 0
    m.reset()
    assert float(m.sum_scores) == 0.0 and int(m.total) == 0 and m.sum_scores.is_cuda
    assert math.isnan(float(m.compute()))
    s = _metric(net, reduction="sum")
    s.update(a, b)
    s.reset()
    assert math.isnan(float(s.compute()))
    m.update(a, b)
    assert torch.equal(m.compute(), first)
    assert m.to(DEV) is m and m.sum_scores.device == torch.device(DEV)
    m.to("cpu")
    assert m.sum_scores.device.type == "cpu" and next(m.net.parameters()).device.type == "cpu"
    m.update(a, b)                                                     # the state and the network follow the images back
    assert m.sum_scores.is_cuda and int(m.total) == 4 and next(m.net.parameters()).is_cuda
    assert abs(float(m.compute()) - float(first)) <= 2.0 ** -23 * float(first)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.update(a.cpu(), b.cpu())
    with pytest.raises(ValueError, match="at least 31"):
        m.update(a[:, :, :30], b[:, :, :30])


def test_reconstruction_metrics_reports_lpips(net):
    from fourm.vq.metrics import ReconstructionMetrics
    g = MU.gen(31)
    images = torch.cat([MU.images(2, 176, 176, 5, -1.0, 1.0), torch.ones(2, 1, 176, 176)], 1).to(DEV)      # a validity mask rides along
    output = (images[:, :3] + 0.6 * (torch.rand(2, 3, 176, 176, generator=g) - 0.5).to(DEV)).contiguous()   # leaves [-1, 1] in places
    assert float(output.abs().max()) > 1.0
    plain, with_lpips = ReconstructionMetrics('rgb'), ReconstructionMetrics('rgb', lpips=_metric(net, normalize=True))
    for r in (plain, with_lpips):
        r.update(output, images)
    want, got = plain.compute('[Eval]', 176), with_lpips.compute('[Eval]', 176)
    assert list(got) == list(want) + ['[Eval] LPIPS@176']
    for k, v in want.items():
        assert got[k] == v, k                                          # Python floats from the same bits
    m = _metric(net, normalize=False)
    m.update(output.clamp(-1.0, 1.0), images[:, :3])
    assert got['[Eval] LPIPS@176'] == float(m.compute()) and 0.0 < got['[Eval] LPIPS@176'] < 1.0
    unclamped = _metric(net, normalize=False)
    unclamped.update(output, images[:, :3])
    assert float(unclamped.compute()) != got['[Eval] LPIPS@176']       # the clamp is in effect
    with_lpips.reset()
    assert math.isnan(with_lpips.compute()['[Eval] LPIPS@None'])
