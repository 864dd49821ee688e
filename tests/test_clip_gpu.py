"""CLIP's vision tower on a real MI355X against the float64 restatement tests/clip_util.py::vit_forward (pinned to upstream's class by
tests/test_clip_cpu.py), for every run of tests/golden/clip_vit_micro.npz and each of the four results.

fp32 mode: max |out - ref| / max |ref| <= 8 x max(upstream's own fp32 distance from float64 (stored), half an fp32 ulp of the largest entry) -
           the project's standing fp32 rule.
bf16 mode: the same distance <= 2 x upstream's CPU-autocast distance (stored).  The engine rounds where autocast does not (bf16 LayerNorm
           outputs, bf16 attention probabilities) and keeps fp32 where autocast rounds (the residual stream), so the two errors are of one
           size but not equal: a factor of 2, not a fitted figure.  Every ratio goes to the parity log.
Measured on an MI355X (this file's run): see INTEGRATION.md, "CLIP vision tower"."""
import pytest
import torch

from tests import clip_util as U
from tests.parity_log import record

pytestmark = pytest.mark.gpu

DEV = "cuda"
RUN_IDS = [(c, r[0]) for c in U.CASES for r in U.RUNS[c]]


def make(case, precision="bf16"):
    from fourm.utils.clip.model import VisionTransformer
    m = VisionTransformer(**U.CASES[case])
    m.load_state_dict(U.seeded_state_dict(case), strict=True)
    m = m.to(DEV).eval().requires_grad_(False)
    m.compute_precision = precision
    return m


@pytest.fixture(scope="module")
def gold():
    return U.load_golden()


@pytest.fixture(scope="module")
def models():
    return {c: make(c) for c in U.CASES}


@pytest.fixture(scope="module")
def ref64():
    """float64 results, computed once on the host and shared (never modified)."""
    out = {}
    for case, run in RUN_IDS:
        sd, x = U.seeded_state_dict(case), U.images(case, run)
        for flag in U.FLAGS:
            out[case, run, flag] = U.vit_forward(sd, x, flag, torch.float64)
    return out


@pytest.mark.parametrize("flag", U.FLAGS)
@pytest.mark.parametrize("case,run", RUN_IDS)
def test_fp32_mode_against_float64(case, run, flag, models, gold, ref64):
    m = models[case]
    m.compute_precision = "fp32"
    try:
        out = m(U.images(case, run).to(DEV), **U.flag_kwargs(flag))
    finally:
        m.compute_precision = "bf16"
    ref = ref64[case, run, flag]
    assert out.dtype == torch.float32 and out.shape == ref.shape and out.is_cuda
    err, stored = U.rel_max(out, ref), float(gold[f"{case}/{run}/{flag}/err32"])
    bound = 8 * max(stored, 2.0 ** -24)
    print(f"clip fp32 {case}/{run}/{flag}: {err:.3e} vs float64 (upstream fp32 {stored:.3e}, ratio {err / stored:.2f}, bound {bound:.3e})")
    record("clip.tower.fp32", case=case, run=run, flag=flag, err=err, upstream_fp32_err=stored, ratio=err / stored)
    assert err <= bound, (case, run, flag, err, bound)


@pytest.mark.parametrize("flag", U.FLAGS)
@pytest.mark.parametrize("case,run", RUN_IDS)
def test_bf16_mode_against_float64(case, run, flag, models, gold, ref64):
    m = models[case]
    assert m.compute_precision == "bf16"
    out = m(U.images(case, run).to(DEV), **U.flag_kwargs(flag))
    ref = ref64[case, run, flag]
    assert out.dtype == torch.float32 and out.shape == ref.shape
    err, stored = U.rel_max(out, ref), float(gold[f"{case}/{run}/{flag}/err_ac"])
    print(f"clip bf16 {case}/{run}/{flag}: {err:.3e} vs float64 (upstream autocast {stored:.3e}, ratio {err / stored:.2f}, bound 2)")
    record("clip.tower.bf16", case=case, run=run, flag=flag, err=err, upstream_autocast_err=stored, ratio=err / stored)
    assert err <= 2 * stored, (case, run, flag, err, stored)


def test_precision_switch_and_back_is_bit_identical(models):
    m = models["clip_a"]
    x = U.images("clip_a", "interp").to(DEV)
    a = m(x, return_final_tokens_no_cls=True).clone()
    m.compute_precision = "fp32"
    f = m(x, return_final_tokens_no_cls=True).clone()
    m.compute_precision = "bf16"
    b = m(x, return_final_tokens_no_cls=True)
    assert torch.equal(a, b) and not torch.equal(a, f)
    with pytest.raises(ValueError, match="compute_precision"):
        m.compute_precision = "tf32"
    assert torch.equal(m(x, return_final_tokens_no_cls=True), a)


def test_batch_sizes_in_turn_reuse_the_cached_tables(models, gold, ref64):
    m = models["clip_b"]
    x = U.images("clip_b", "native").to(DEV)
    flag = "return_all_final_tokens"
    full = m(x, **U.flag_kwargs(flag)).clone()
    tables = dict(m._tables)
    part = m(x[:2], **U.flag_kwargs(flag)).clone()                              # another batch size: new row maps, the same position table
    again = m(x, **U.flag_kwargs(flag))
    assert torch.equal(again, full)
    assert all(m._tables[k] is v for k, v in tables.items()) and len(m._tables) == len(tables)       # all_final needs no row map
    assert U.rel_max(part, ref64["clip_b", "native", flag][:2]) <= 2 * float(gold[f"clip_b/native/{flag}/err_ac"])
    cls5, cls2 = m(x).clone(), m(x[:2]).clone()                                # the class-row maps of both sizes, then the first again
    assert torch.equal(m(x), cls5) and torch.equal(m(x[:2]), cls2)
    assert U.rel_max(cls2, ref64["clip_b", "native", "default"][:2]) <= 2 * float(gold["clip_b/native/default/err_ac"])
    xi = U.images("clip_b", "interp").to(DEV)                                   # another image size in between
    other = m(xi, return_all_tokens=True)
    assert other.shape == (2, 12, 192) and torch.equal(m(x, **U.flag_kwargs(flag)), full)


def test_adopted_state_dict_gives_the_same_bits(models):
    from fourm.utils.clip.model import VisionTransformer, build_visual
    direct = models["clip_a"]
    x = U.images("clip_a", "native").to(DEV)
    want = direct(x, return_final_tokens_no_cls=True).clone()
    sd = {"visual." + k: v for k, v in U.seeded_state_dict("clip_a").items()}
    built = build_visual(sd).to(DEV)
    assert torch.equal(built(x, return_final_tokens_no_cls=True), want)
    adopted = VisionTransformer.from_upstream(direct)
    assert adopted is not direct and adopted.class_embedding.is_cuda
    assert torch.equal(adopted(x, return_final_tokens_no_cls=True), want)
    direct.load_state_dict({k: v + 0.01 for k, v in U.seeded_state_dict("clip_a").items()})       # new weights reach the device images
    assert not torch.equal(direct(x, return_final_tokens_no_cls=True), want)
    direct.load_state_dict(U.seeded_state_dict("clip_a"))
    assert torch.equal(direct(x, return_final_tokens_no_cls=True), want)


def test_trainable_tower_is_refused_on_the_device():
    m = make("clip_a").requires_grad_(True)
    x = U.images("clip_a", "native").to(DEV)
    with pytest.raises(NotImplementedError, match="inference only"):
        m(x)
    with torch.no_grad():
        assert m(x).shape == (3, 64)
