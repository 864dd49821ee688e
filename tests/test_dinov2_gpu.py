"""DINOv2's vision tower on a real MI355X against the float64 restatement tests/dinov2_util.py::dino_forward (the written definition is the
contract; parity with the `facebookresearch/dinov2` package and with the real checkpoints is unpinned), for every run of
tests/golden/dinov2_micro.npz and every result, by the rule of tests/test_clip_gpu.py:

fp32 mode: max |out - ref| / max |ref| <= 8 x max(the restatement's own fp32 distance from float64 (stored), 2^-24).
bf16 mode: the same distance <= 2 x the restatement's CPU-autocast distance (stored).  The engine rounds where autocast does not (bf16
           LayerNorm outputs, bf16 attention probabilities) and keeps fp32 where autocast rounds, so the two errors are of one size but not
           equal: a factor of 2, not a fitted figure.  Every ratio goes to the parity log.
The LayerScale gammas are drawn from [-1.5, 1.5]: a dropped or misplaced LayerScale changes every result by far more than either bound.
Measured on an MI355X (this file's run): see INTEGRATION.md, "DINOv2 tower"."""
import pytest
import torch

from tests import dinov2_util as U
from tests.parity_log import record

pytestmark = pytest.mark.gpu

DEV = "cuda"
RUN_IDS = [(c, r[0]) for c in U.CASES for r in U.RUNS[c]]
RESULT_IDS = [(c, r, name) for c, r in RUN_IDS for name in U.results_of(c)]


def make(case, precision="bf16"):
    from fourm.utils.dinov2 import DinoVisionTransformer
    m = DinoVisionTransformer(**U.CASES[case])
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
    return {(case, run): U.dino_forward(case, U.seeded_state_dict(case), U.images(case, run), torch.float64) for case, run in RUN_IDS}


@pytest.fixture(scope="module")
def outs(models):
    """The tower's result dicts per (precision, case, run): one forward each, shared by the per-result checks."""
    res = {}
    for prec in ("fp32", "bf16"):
        for case, run in RUN_IDS:
            m = models[case]
            m.compute_precision = prec
            try:
                res[prec, case, run] = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in m(U.images(case, run).to(DEV), is_training=True).items()}
            finally:
                m.compute_precision = "bf16"
    return res


@pytest.mark.parametrize("case,run,name", RESULT_IDS)
def test_fp32_mode_against_float64(case, run, name, outs, gold, ref64):
    out, ref = outs["fp32", case, run][name], ref64[case, run][name]
    assert out.dtype == torch.float32 and out.shape == ref.shape and out.is_cuda and outs["fp32", case, run]["masks"] is None
    err, stored = U.rel_max(out, ref), float(gold[f"{case}/{run}/{name}/err32"])
    bound = 8 * max(stored, 2.0 ** -24)
    print(f"dinov2 fp32 {case}/{run}/{name}: {err:.3e} vs float64 (restatement fp32 {stored:.3e}, ratio {err / stored:.2f}, bound {bound:.3e})")
    record("dinov2.tower.fp32", case=case, run=run, result=name, err=err, restatement_fp32_err=stored, ratio=err / stored)
    assert err <= bound, (case, run, name, err, bound)


@pytest.mark.parametrize("case,run,name", RESULT_IDS)
def test_bf16_mode_against_float64(case, run, name, outs, gold, ref64):
    out, ref = outs["bf16", case, run][name], ref64[case, run][name]
    assert out.dtype == torch.float32 and out.shape == ref.shape
    err, stored = U.rel_max(out, ref), float(gold[f"{case}/{run}/{name}/err_ac"])
    print(f"dinov2 bf16 {case}/{run}/{name}: {err:.3e} vs float64 (restatement autocast {stored:.3e}, ratio {err / stored:.2f}, bound 2)")
    record("dinov2.tower.bf16", case=case, run=run, result=name, err=err, restatement_autocast_err=stored, ratio=err / stored)
    assert err <= 2 * stored, (case, run, name, err, stored)


@pytest.mark.parametrize("case,run", RUN_IDS)
def test_results_are_views_of_one_norm_and_forward_returns_the_class_token(case, run, models, outs):
    m = models[case]
    x = U.images(case, run).to(DEV)
    d = m(x, is_training=True)
    Rn = U.CASES[case]["num_register_tokens"]
    base = d["x_norm_clstoken"]._base
    assert base is not None and d["x_norm_patchtokens"]._base is base and d["x_norm_regtokens"]._base is base
    assert d["x_norm_regtokens"].shape[1] == Rn and set(d) == {"x_norm_clstoken", "x_norm_regtokens", "x_norm_patchtokens", "x_prenorm", "masks"}
    assert torch.equal(m(x), outs["bf16", case, run]["x_norm_clstoken"]) and torch.equal(m.forward_features(x)["x_prenorm"], outs["bf16", case, run]["x_prenorm"])


@pytest.mark.parametrize("case,run", [("dino_a", "interp"), ("dino_b", "interp")])
def test_get_intermediate_layers_in_both_forms(case, run, models, gold, ref64):
    m, cfg = models[case], U.CASES[case]
    x = U.images(case, run).to(DEV)
    ref, depth, Rn = ref64[case, run], cfg["depth"], cfg["num_register_tokens"]
    B, gh, gw = x.shape[0], x.shape[2] // 14, x.shape[3] // 14
    # form 1: the last n blocks, normalised patch tokens
    got = m.get_intermediate_layers(x, n=depth)
    assert isinstance(got, tuple) and len(got) == depth
    for i, o in enumerate(got):
        want = ref["norm"](ref["layers"][i])[:, 1 + Rn:]
        assert o.shape == want.shape == (B, gh * gw, cfg["embed_dim"])
        err, stored = U.rel_max(o, want), float(gold[f"{case}/{run}/layers/{i}/err_ac"])
        record("dinov2.layers.bf16", case=case, run=run, layer=i, err=err, restatement_autocast_err=stored, ratio=err / stored)
        assert err <= 2 * stored, (case, i, err, stored)
    # the last one is the forward's own result, to the bit
    assert torch.equal(got[-1], m(x, is_training=True)["x_norm_patchtokens"])
    # form 2: listed blocks, reshaped to maps, with the class tokens, without the final norm
    pairs = m.get_intermediate_layers(x, n=[0], reshape=True, return_class_token=True, norm=False)
    assert len(pairs) == 1 and len(pairs[0]) == 2
    maps, cls = pairs[0]
    assert maps.shape == (B, cfg["embed_dim"], gh, gw) and cls.shape == (B, cfg["embed_dim"]) and maps.is_contiguous()
    want = ref["layers"][0]
    stored = float(gold[f"{case}/{run}/layers/0/err_ac"])
    flat = torch.cat([cls.unsqueeze(1), maps.flatten(2).transpose(1, 2)], 1)
    assert U.rel_max(flat, torch.cat([want[:, :1], want[:, 1 + Rn:]], 1)) <= 2 * stored
    assert torch.equal(maps.flatten(2).transpose(1, 2), m.get_intermediate_layers(x, n=[0], norm=False)[0])
    with pytest.raises(ValueError, match="get_intermediate_layers"):
        m.get_intermediate_layers(x, n=depth + 1)


def test_precision_switch_and_back_is_bit_identical(models):
    m = models["dino_a"]
    x = U.images("dino_a", "interp").to(DEV)
    a = m(x, is_training=True)["x_norm_patchtokens"].clone()
    m.compute_precision = "fp32"
    f = m(x, is_training=True)["x_norm_patchtokens"].clone()
    m.compute_precision = "bf16"
    b = m(x, is_training=True)["x_norm_patchtokens"]
    assert torch.equal(a, b) and not torch.equal(a, f)


def test_batch_sizes_in_turn_reuse_the_cached_tables(models):
    m = models["dino_b"]
    x = U.images("dino_b", "interp").to(DEV)
    xn = torch.randn(2, 3, 42, 28, generator=torch.Generator().manual_seed(9)).to(DEV)      # grid 3 x 2: no other test uses it
    full = m(x, is_training=True)["x_prenorm"].clone()
    tables = dict(m._tables)
    assert not any(k[1:3] == (3, 2) for k in tables)
    part = m(x[:1], is_training=True)["x_prenorm"].clone()
    assert dict(m._tables).keys() == tables.keys()                         # another batch size: the same table
    other = m(xn)                                                          # another grid in between: its table joins, none leaves
    assert other.shape == (2, 192) and all(m._tables[k] is v for k, v in tables.items()) and len(m._tables) == len(tables) + 1
    assert sum(k[1:3] == (3, 2) for k in m._tables) == 1
    assert torch.equal(m(x, is_training=True)["x_prenorm"], full) and torch.equal(part, full[:1])


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_a_batch_of_three_equals_three_single_calls(precision, models):
    m = models["dino_a"]
    x = U.images("dino_a", "interp").to(DEV)
    assert x.shape[0] == 3
    m.compute_precision = precision
    try:
        whole = {k: v.clone() for k, v in m(x, is_training=True).items() if torch.is_tensor(v)}
        for i in range(3):
            one = m(x[i:i + 1], is_training=True)
            for k, v in whole.items():
                assert torch.equal(one[k], v[i:i + 1]), (precision, i, k)
    finally:
        m.compute_precision = "bf16"


def test_adopted_state_dict_gives_the_same_bits(models):
    from fourm.utils.dinov2 import DinoVisionTransformer, build_dinov2
    for case in U.CASES:
        direct = models[case]
        x = U.images(case, "interp").to(DEV)
        want = direct(x, is_training=True)["x_norm_patchtokens"].clone()
        built = build_dinov2(U.seeded_state_dict(case)).to(DEV)
        assert torch.equal(built(x, is_training=True)["x_norm_patchtokens"], want)
        adopted = DinoVisionTransformer.from_upstream(direct)
        assert adopted is not direct and adopted.cls_token.is_cuda
        assert torch.equal(adopted(x, is_training=True)["x_norm_patchtokens"], want)
        direct.load_state_dict({k: v + 0.01 for k, v in U.seeded_state_dict(case).items()})       # new weights reach the device images (w12's halves too)
        assert not torch.equal(direct(x, is_training=True)["x_norm_patchtokens"], want)
        direct.load_state_dict(U.seeded_state_dict(case))
        assert torch.equal(direct(x, is_training=True)["x_norm_patchtokens"], want)


def test_layerscale_fusion_switch_gives_the_same_bits(models, monkeypatch):
    """Settling every LayerScale sum with fm_layerscale_add (the measurement's baseline) or inside the next LayerNorm: one arithmetic."""
    from fourm.hip import engine as E
    m = models["dino_a"]
    x = U.images("dino_a", "native").to(DEV)
    fused = m(x, is_training=True)["x_prenorm"].clone()
    monkeypatch.setattr(E, "LS_FUSE", False)
    assert torch.equal(m(x, is_training=True)["x_prenorm"], fused)


def test_trainable_tower_is_refused_on_the_device():
    m = make("dino_a").requires_grad_(True)
    x = U.images("dino_a", "native").to(DEV)
    with pytest.raises(NotImplementedError, match="inference only"):
        m(x)
    with torch.no_grad():
        assert m(x).shape == (2, 128)
