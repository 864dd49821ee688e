"""fourm.utils.inception end to end on the GPU: the tower against the float64 restatement (tests/inception_util.py), batch and chunk
invariance, FID against a second float64 route, the Inception score, and both metrics through the tower."""
import json
import os

import numpy as np
import pytest
import torch

from tests import inception_util as IU
from tests import parity_log

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tower():
    from fourm.utils.inception import FidInceptionV3
    m = FidInceptionV3()
    m.load_state_dict(IU.fixture()["sd"])
    return m.to(DEV).eval().requires_grad_(False)


@pytest.fixture(scope="module")
def tower_out(tower):
    return tower(IU.fixture()["imgs"].to(DEV))


def test_tower_matches_the_float64_restatement(tower, tower_out):
    fx = IU.fixture()
    for key in ("pool", "logits_unbiased"):
        ref64, ref32 = fx["ref64"][key], fx["ref32"][key]
        got = tower_out[key]
        assert got.dtype == torch.float32 and tuple(got.shape) == tuple(ref64.shape)
        tol, base = IU.tower_tol(ref64, ref32)
        err = float((got.cpu().double() - ref64).abs().max()) / float(ref64.abs().max())
        print(f"tower {key}: err {err:.3e}, fp32 restatement {base:.3e}, bound {tol:.3e}")
        parity_log.record("test_tower_matches_the_float64_restatement", tensor=key, err=err, fp32_restatement=base, bound=tol, ratio=err / base if base else None)
        assert err <= tol, (key, err, base, tol)
    assert torch.equal(tower_out["logits"], tower_out["logits_unbiased"] + fx["sd"]["fc.bias"].to(DEV))


def test_tower_is_batch_and_chunk_invariant(tower, tower_out):
    imgs = IU.fixture()["imgs"].to(DEV)
    alone = tower(imgs[:1])
    chunked = tower(imgs, chunk=1)
    for key in ("pool", "logits_unbiased", "logits"):
        assert torch.equal(alone[key][0], tower_out[key][0]), key
        assert torch.equal(chunked[key], tower_out[key]), key


def test_features_entry_and_normalized_input(tower, tower_out):
    from fourm.utils.inception import ops
    imgs = IU.fixture()["imgs"].to(DEV)
    rows = ops.inception_preprocess(imgs)
    assert torch.equal(tower.features(rows)["pool"], tower_out["pool"])
    as_float = (imgs.float() + 0.5) / 255.0                            # trunc(255 v) is the byte again
    assert torch.equal(tower(as_float, normalize=True)["pool"], tower_out["pool"])
    with pytest.raises(TypeError):
        tower(as_float)
    with pytest.raises(RuntimeError, match="no CPU path"):
        tower(imgs.cpu())


def _gaussians():
    g = IU.gen(2024)
    real = (torch.randn(200, 16, generator=g) * torch.linspace(0.5, 2.0, 16)).float()
    fake = (0.3 + 1.2 * torch.randn(150, 16, generator=g)).float()
    return real, fake


def test_fid_from_features_against_the_second_float64_route():
    from fourm.utils.inception import FrechetInceptionDistance
    real, fake = _gaussians()
    fid = FrechetInceptionDistance(feature=2048, reset_real_features=True, normalize=False, sync_on_compute=True)
    for part in real.split(67):                                        # three updates each
        fid.update_features(part.to(DEV), real=True)
    for part in fake.split(50):
        fid.update_features(part.to(DEV), real=False)
    m1, m2 = IU.moments(real), IU.moments(fake)
    for got, ref in ((fid.real_sum, m1[0]), (fid.real_outer, m1[1]), (fid.fake_sum, m2[0]), (fid.fake_outer, m2[1])):
        assert got.dtype == torch.float64 and np.array_equal(got.cpu().numpy(), ref)      # the state is exact
    assert int(fid.real_n.item()) == 200 and int(fid.fake_n.item()) == 150
    tol, spread = IU.fid_tol(m1, m2)
    out = fid.compute()
    assert out.dtype == torch.float32 and out.dim() == 0
    from fourm.utils.inception import fid_from_moments
    got = float(fid_from_moments(fid.real_sum, fid.real_outer, 200, fid.fake_sum, fid.fake_outer, 150))
    ref = IU.fid_eigh(m1, m2)
    diff = abs(got - ref)
    assert ref > 0.1 and diff <= tol, (got, ref, tol, spread)
    assert float(out) == float(torch.tensor(got, dtype=torch.float64).float())      # what compute() returns is that float64 number rounded to fp32 once
    try:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        with open(os.path.join(ROOT, "profiles", "fid_parity.json"), "w") as f:
            json.dump(dict(case="d=16, 200 real / 150 fake, two Gaussians", fid_eigh_route=ref, fid_compute=got, difference=diff,
                           spread_between_float64_routes=spread, bound=tol), f, indent=1)
            f.write("\n")
    except OSError:
        pass
    # identical features on both sides
    same = FrechetInceptionDistance()
    same.update_features(real.to(DEV), real=True)
    same.update_features(real.to(DEV), real=False)
    assert abs(float(fid_from_moments(same.real_sum, same.real_outer, 200, same.fake_sum, same.fake_outer, 200))) <= tol


def test_fid_reset_and_to():
    from fourm.utils.inception import FrechetInceptionDistance
    real, fake = _gaussians()
    keep = FrechetInceptionDistance(reset_real_features=False)
    keep.update_features(real.to(DEV), real=True)
    keep.update_features(fake.to(DEV), real=False)
    before = float(keep.compute())
    real_sum = keep.real_sum.clone()
    keep.reset()
    assert torch.equal(keep.real_sum, real_sum) and int(keep.real_n.item()) == 200
    assert int(keep.fake_n.item()) == 0 and not keep.fake_sum.any() and not keep.fake_outer.any()
    with pytest.raises(RuntimeError, match="at least 2 samples"):
        keep.compute()
    keep.update_features(fake.to(DEV), real=False)
    assert float(keep.compute()) == before
    drop = FrechetInceptionDistance(reset_real_features=True)
    drop.update_features(real.to(DEV), real=True)
    drop.reset()
    assert int(drop.real_n.item()) == 0 and not drop.real_outer.any()
    snapshot = [getattr(keep, n).clone() for n in keep._STATE]
    keep.to("cpu")
    assert all(getattr(keep, n).device.type == "cpu" for n in keep._STATE)
    keep.to(DEV)
    assert all(torch.equal(getattr(keep, n), s) for n, s in zip(keep._STATE, snapshot))
    assert float(keep.compute()) == before
    with pytest.raises(ValueError):
        keep.update_features(torch.zeros(3, 8, device=DEV), real=True)


def test_fid_through_the_tower(tower):
    from fourm.utils.inception import FrechetInceptionDistance
    imgs = torch.randint(0, 256, (6, 3, 40, 56), generator=IU.gen(3), dtype=torch.uint8).to(DEV)
    fid = FrechetInceptionDistance(feature=tower)
    assert fid.inception is tower
    fid.update(imgs[:3], real=True)
    fid.update(imgs[3:], real=False)
    pool = tower(imgs)["pool"]
    for got, part in ((fid.real_sum, pool[:3]), (fid.fake_sum, pool[3:])):
        rs, _, _ = IU.moments(part)
        assert np.array_equal(got.cpu().numpy(), rs)
    assert int(fid.real_n.item()) == 3 and int(fid.fake_n.item()) == 3
    out = fid.compute()
    assert out.dtype == torch.float32 and bool(torch.isfinite(out))


def test_inception_score_from_logits():
    from fourm.utils.inception import InceptionScore
    g = IU.gen(31)
    logits = (2.0 * torch.randn(53, 1008, generator=g)).float()
    isc = InceptionScore(feature="logits_unbiased", splits=10, normalize=False, generator=IU.gen(99), sync_on_compute=True)
    for part in logits.split(20):
        isc.update_features(part.to(DEV))
    assert isc.n == 53 and torch.equal(isc.features[:53].cpu(), logits)
    mean, std = isc.compute()
    perm = torch.randperm(53, generator=IU.gen(99))
    ref_mean, ref_std = IU.inception_score(logits, 10, perm)
    assert ref_mean > 1.0 and ref_std > 0.0
    assert abs(float(mean) - ref_mean) <= 1e-6 * ref_mean, (float(mean), ref_mean)
    assert abs(float(std) - ref_std) <= 1e-6 * ref_std, (float(std), ref_std)
    isc.reset()
    assert isc.n == 0
    with pytest.raises(RuntimeError):
        isc.compute()


def test_inception_score_through_the_tower(tower):
    from fourm.utils.inception import InceptionScore
    imgs = torch.randint(0, 256, (4, 3, 40, 56), generator=IU.gen(4), dtype=torch.uint8).to(DEV)
    isc = InceptionScore(inception=tower, splits=2, generator=IU.gen(1))
    isc.update(imgs[:3])
    isc.update(imgs[3:])
    assert isc.n == 4 and torch.equal(isc.features[:4], tower(imgs)["logits_unbiased"])
    mean, std = isc.compute()
    assert bool(torch.isfinite(mean)) and bool(torch.isfinite(std))
