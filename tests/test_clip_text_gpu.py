"""CLIP's text tower, the logits and the CLIP score on a real MI355X.

The tower against the float64 restatement tests/clip_text_util.py::text_forward (pinned to upstream's class by tests/test_clip_text_cpu.py), for
both cases of tests/golden/clip_text_micro.npz and each of the three results, with the two rules of tests/test_clip_gpu.py and the bounds read
from the fixture:
    fp32 mode: max |out - ref| / max |ref| <= 8 x max(upstream's own fp32 distance from float64, half an fp32 ulp of the largest entry);
    bf16 mode: the same distance <= 2 x upstream's CPU-autocast distance.
The three new kernels alone against torch / float64, causality (tokens behind the end-of-text position do not reach the result, bit for bit),
the few-row route of the projection against the tiled one, ``clip_logits``, ``ClipScore``, and the vision tower's bits before and after a text
forward.  Every ratio goes to the parity log; INTEGRATION.md ("CLIP text tower and CLIP score") quotes this file's run."""
import math

import pytest
import torch

from tests import clip_text_util as U
from tests import clip_util as V
from tests.parity_log import record

pytestmark = pytest.mark.gpu

DEV = "cuda"
ULP_100 = 2.0 ** -17          # one fp32 ulp of 100 (64 <= 100 < 128)


def make(case, precision="bf16"):
    from fourm.utils.clip.text import TextTransformer
    m = TextTransformer(**U.CASES[case])
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
    for case in U.CASES:
        sd, ids = U.seeded_state_dict(case), U.token_ids(case)
        for flag in U.FLAGS:
            out[case, flag] = U.text_forward(sd, ids, flag, torch.float64)
    return out


def run(m, ids, precision, **kw):
    m.compute_precision = precision
    try:
        return m(ids, **kw).clone()
    finally:
        m.compute_precision = "bf16"


# ---- the tower against float64 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flag", U.FLAGS)
@pytest.mark.parametrize("case", list(U.CASES))
def test_fp32_mode_against_float64(case, flag, models, gold, ref64):
    out = run(models[case], U.token_ids(case).to(DEV), "fp32", **U.flag_kwargs(flag))
    ref = ref64[case, flag]
    assert out.dtype == torch.float32 and out.shape == ref.shape and out.is_cuda
    err, stored = U.rel_max(out, ref), float(gold[f"{case}/{flag}/err32"])
    bound = 8 * max(stored, 2.0 ** -24)
    print(f"clip text fp32 {case}/{flag}: {err:.3e} vs float64 (upstream fp32 {stored:.3e}, ratio {err / stored:.2f}, bound {bound:.3e})")
    record("clip.text.fp32", case=case, flag=flag, err=err, upstream_fp32_err=stored, ratio=err / stored)
    assert err <= bound, (case, flag, err, bound)


@pytest.mark.parametrize("flag", U.FLAGS)
@pytest.mark.parametrize("case", list(U.CASES))
def test_bf16_mode_against_float64(case, flag, models, gold, ref64):
    m = models[case]
    assert m.compute_precision == "bf16"
    out = m.encode_text(U.token_ids(case).int().to(DEV), **U.flag_kwargs(flag))          # (int32 ids: the other accepted type)
    ref = ref64[case, flag]
    assert out.dtype == torch.float32 and out.shape == ref.shape
    err, stored = U.rel_max(out, ref), float(gold[f"{case}/{flag}/err_ac"])
    print(f"clip text bf16 {case}/{flag}: {err:.3e} vs float64 (upstream autocast {stored:.3e}, ratio {err / stored:.2f}, bound 2)")
    record("clip.text.bf16", case=case, flag=flag, err=err, upstream_autocast_err=stored, ratio=err / stored)
    assert err <= 2 * stored, (case, flag, err, stored)


# ---- the kernels alone ---------------------------------------------------------------------------------------------------------------------------
def embed_inputs(B, Lc, D, Vn, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, Vn, (B, Lc), generator=g)
    if Lc >= 4:                                                                  # row 0 carries its maximum twice: the first one counts
        ids[0] = torch.clamp(ids[0], max=max(Vn - 2, 0))
        ids[0, 2] = ids[0, Lc - 1] = Vn - 1
    return ids, torch.randn(Vn, D, generator=g), torch.randn(Lc, D, generator=g)


def launch_embed(ids, tok, pos, pad=4):
    from fourm.hip import ops
    (B, Lc), D = ids.shape, tok.shape[1]
    out = torch.full((B * Lc + 1, D + pad), -7.0, dtype=torch.float32, device=DEV)      # a sentinel row and sentinel columns: nothing lands there
    eot = torch.full((B,), -5, dtype=torch.int32, device=DEV)
    emap = torch.full((B * Lc,), -5, dtype=torch.int32, device=DEV)
    bad = torch.full((1,), 77, dtype=torch.int32, device=DEV)                            # (the call zeroes it)
    ops.clip_text_embed(ids.to(DEV), tok.to(DEV), pos.to(DEV), out, eot, bad, emap)
    return out.cpu(), eot.cpu(), emap.cpu(), int(bad.item())


@pytest.mark.parametrize("B,Lc,D,Vn", [(1, 1, 4, 1), (3, 12, 128, 50), (2, 77, 64, 300)])
def test_text_embed_kernel_is_the_gather_and_one_add(B, Lc, D, Vn):
    ids, tok, pos = embed_inputs(B, Lc, D, Vn, 11)
    out, eot, emap, bad = launch_embed(ids, tok, pos)
    want = tok[ids] + pos                                                        # fp32: one add per element
    assert torch.equal(out[:B * Lc, :D].view(B, Lc, D), want)
    assert bool((out[:, D:] == -7.0).all()) and bool((out[B * Lc:] == -7.0).all())
    arg = ids.argmax(dim=-1)
    if Lc >= 4:
        assert int(arg[0]) == 2                                                  # the tie row: torch.argmax documents the first maximum
    assert torch.equal(eot.long(), torch.arange(B) * Lc + arg)
    want_map = torch.full((B, Lc), -1, dtype=torch.int32)
    want_map[torch.arange(B), arg] = torch.arange(B, dtype=torch.int32)
    assert torch.equal(emap.view(B, Lc), want_map) and bad == 0


def test_text_embed_kernel_never_indexes_with_a_bad_id():
    B, Lc, D, Vn = 3, 12, 128, 50
    ids, tok, pos = embed_inputs(B, Lc, D, Vn, 12)
    ids[1, 3], ids[2, 5] = Vn, -1
    out, eot, emap, bad = launch_embed(ids, tok, pos)
    ok = (ids >= 0) & (ids < Vn)
    want = torch.where(ok[..., None], tok[ids.clamp(0, Vn - 1)] + pos, torch.zeros(()))
    assert torch.equal(out[:B * Lc, :D].view(B, Lc, D), want) and bad == 2
    assert bool((out[Lc + 3, :D] == 0).all()) and bool((out[2 * Lc + 5, :D] == 0).all())
    assert torch.equal(eot.long(), torch.arange(B) * Lc + ids.argmax(dim=-1))   # (the pick follows the ids as given, as torch.argmax would)


def pair_inputs(B, E, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, E, generator=g), torch.randn(B, E, generator=g) * 3.0


@pytest.mark.parametrize("B", [1, 300])
@pytest.mark.parametrize("E", [1, 40, 513])
def test_pair_score_kernel_against_float64(B, E):
    """Per pair: |score - 100 cos in float64| <= 4 fp32 ulps of 100 (an fp32 dot over E terms normalised by two fp32 norms; the kernel evaluates
    the normalisation of the three fp32 sums in double and rounds once).  The double sum is the exact sum of the kernel's own fp32 scores (every
    partial sum of at most 300 such values is representable, so the order cannot show).  Strided rows, a zero row, two calls."""
    from fourm.hip import ops
    img, txt = pair_inputs(B, E, 21 + E)
    if B > 1:
        img[7] = 0.0                                                             # a zero-norm row
    wide_i = torch.full((B, E + 3), 9.0)
    wide_i[:, :E] = img
    di, dt = wide_i.to(DEV)[:, :E], txt.to(DEV)                                  # (row stride E + 3 on one side)
    outs = []
    for _ in range(2):
        score = torch.full((B,), -1.0, dtype=torch.float32, device=DEV)
        total, count = torch.zeros(1, dtype=torch.float64, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV)
        ops.clip_pair_score(di, dt, score, total, count)
        outs.append((score.cpu(), total.cpu(), count.cpu()))
    score, total, count = outs[0]
    assert torch.equal(score, outs[1][0]) and torch.equal(total.view(torch.int64), outs[1][1].view(torch.int64))       # two calls: equal bits
    i64, t64 = img.double(), txt.double()
    den = i64.norm(dim=-1) * t64.norm(dim=-1)
    ref = torch.where(den > 0, 100.0 * (i64 * t64).sum(-1) / den.clamp_min(1e-300), torch.zeros((), dtype=torch.float64))
    err = float((score.double() - ref).abs().max())
    print(f"pair score B={B} E={E}: worst |score - float64| = {err:.3e} = {err / ULP_100:.2f} ulps of 100 (bound 4)")
    record("clip.pair_score", B=B, E=E, err=err, ulps_of_100=err / ULP_100)
    assert err <= 4 * ULP_100, (B, E, err)
    if B > 1:
        assert float(score[7]) == 0.0
    assert float(total) == math.fsum(score.tolist()) and int(count) == B
    # the accumulators accumulate: a second launch on the same state doubles both
    s2 = torch.empty(B, dtype=torch.float32, device=DEV)
    tot2, cnt2 = total.to(DEV), count.to(DEV)
    ops.clip_pair_score(di, dt, s2, tot2, cnt2)
    assert float(tot2) == 2 * float(total) and int(cnt2) == 2 * B


@pytest.mark.parametrize("R", [1, 300])
@pytest.mark.parametrize("E", [1, 40, 513])
def test_l2_normalize_rows_kernel_against_float64(R, E):
    """y = x f / |x| with f = factor * factor_dev[0].  Every |y| <= f, and the kernel rounds three times (the fp32 sum of squares, f / sqrt of
    it - evaluated in double -, the product): <= 4 fp32 ulps of f per element is the bound, as for the pair score.  Out of place, in place,
    strided, a zero row, two calls."""
    from fourm.hip import ops
    g = torch.Generator().manual_seed(31 + E)
    x = torch.randn(R, E, generator=g) * 5.0
    if R > 1:
        x[4] = 0.0
    factor, fdev = 2.0, torch.tensor([1.0 / 0.14], dtype=torch.float32)         # f = 14.2857..., CLIP's exp(logit_scale)
    f = factor * float(fdev)
    ulp_f = 2.0 ** (math.floor(math.log2(f)) - 23)
    n64 = x.double().norm(dim=-1, keepdim=True)
    ref = torch.where(n64 > 0, x.double() * f / n64.clamp_min(1e-300), torch.zeros((), dtype=torch.float64))
    wide = torch.full((R, E + 5), 9.0, device=DEV)
    wide[:, :E] = x.to(DEV)
    y = torch.full((R, E + 2), -3.0, device=DEV)
    ops.l2_normalize_rows(wide[:, :E], y[:, :E], factor, fdev.to(DEV))           # out of place, both strided
    again = torch.full((R, E + 2), -3.0, device=DEV)
    ops.l2_normalize_rows(wide[:, :E], again[:, :E], factor, fdev.to(DEV))
    assert torch.equal(y, again) and bool((y[:, E:] == -3.0).all())
    inplace = x.to(DEV).clone()
    assert ops.l2_normalize_rows(inplace, None, f) is inplace                    # in place, the factor by value
    err = float((y[:, :E].cpu().double() - ref).abs().max())
    err_in = float((inplace.cpu().double() - ref).abs().max())
    print(f"l2 normalise R={R} E={E}: worst error {err:.3e} = {err / ulp_f:.2f} ulps of f (in place {err_in / ulp_f:.2f}; bound 4)")
    record("clip.l2_normalize", R=R, E=E, ulps_of_f=err / ulp_f, ulps_of_f_in_place=err_in / ulp_f)
    assert err <= 4 * ulp_f and err_in <= 4 * ulp_f, (R, E, err, err_in)
    if R > 1:
        assert bool((y[4, :E] == 0).all()) and bool((inplace[4] == 0).all())
    unit = ops.l2_normalize_rows(x.to(DEV), torch.empty(R, E, device=DEV))       # no factor: unit rows
    rows = unit.cpu().double().norm(dim=-1)
    keep = torch.ones(R, dtype=torch.bool)
    if R > 1:
        keep[4] = False
    assert float((rows[keep] - 1).abs().max()) <= 4 * 2.0 ** -24 * max(1.0, E ** 0.5)


# ---- causality ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
@pytest.mark.parametrize("case", list(U.CASES))
def test_tokens_behind_the_end_of_text_do_not_reach_the_result(case, precision, models):
    """Every token after a row's end-of-text position replaced by another id below the maximum: the default result and the normalised rows up to
    that position keep their bits (row-local kernels and a causal mask; a key that leaked through a tile's mask would show here)."""
    m = models[case]
    ids = U.token_ids(case)
    other = ids.clone()
    top = U.CASES[case]["vocab_size"] - 1
    eot = ids.argmax(dim=-1)
    changed = 0
    for b in range(ids.shape[0]):
        tail = slice(int(eot[b]) + 1, None)
        other[b, tail] = (ids[b, tail] * 7 + 3) % (top - 1)                      # other ids, all below the maximum (the second maximum goes too)
        changed += int((other[b] != ids[b]).sum())
    assert changed > 0 and torch.equal(other.argmax(dim=-1), eot)
    a, b_ = run(m, ids.to(DEV), precision), run(m, other.to(DEV), precision)
    assert torch.equal(a, b_)
    pa, pb = run(m, ids.to(DEV), precision, return_patch_tokens=True), run(m, other.to(DEV), precision, return_patch_tokens=True)
    differs = False
    for b in range(ids.shape[0]):
        e = int(eot[b])
        assert torch.equal(pa[b, :e + 1], pb[b, :e + 1]), (case, precision, b)
        differs = differs or (e + 1 < ids.shape[1] and not torch.equal(pa[b, e + 1:], pb[b, e + 1:]))
    assert differs                                                               # (the replaced tokens themselves did change)


# ---- batch routes -------------------------------------------------------------------------------------------------------------------------------
def test_few_row_and_tiled_projection_routes_agree(models, gold, ref64):
    """Case A at 33 samples (past the 32-row few-row kernel of the bf16 projection) against 3 samples: the first three results within the bf16
    bound of the test above, both ways.  fp32 mode: fm_gemm_f32 picks kernel and tiling from strides and alignment, never from the number of
    rows (csrc/fp32_verify.hip: 128 x 128 tiles, no split over K), and every other kernel of the path is row- or sample-local, so there the
    first three samples are required to be the SAME BITS."""
    m = models["text_a"]
    small, big = U.token_ids("text_a").to(DEV), U.token_ids("text_a", 33).to(DEV)
    assert torch.equal(big[:3], small)
    ref, stored = ref64["text_a", "default"], float(gold["text_a/default/err_ac"])
    o3, o33 = run(m, small, "bf16"), run(m, big, "bf16")
    assert o33.shape == (33, 40)
    e3, e33 = U.rel_max(o3, ref), U.rel_max(o33[:3], ref)
    print(f"clip text batch routes: B=3 {e3:.3e}, B=33 first three {e33:.3e} (bound {2 * stored:.3e}); equal bits: {torch.equal(o3, o33[:3])}")
    record("clip.text.batch_routes", err_b3=e3, err_b33=e33, bound=2 * stored, equal_bits_bf16=bool(torch.equal(o3, o33[:3])))
    assert e3 <= 2 * stored and e33 <= 2 * stored
    f3, f33 = run(m, small, "fp32"), run(m, big, "fp32")
    assert torch.equal(f3, f33[:3])


# ---- logits -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("as_tensor", [True, False])
def test_clip_logits_against_the_float64_formula(as_tensor):
    """logits_per_image = exp(logit_scale) norm(img) norm(txt)^T.  With s = exp(logit_scale): a normalised element carries <= 3 roundings, the
    fp32 dot over E = 40 terms <= E more, all relative to s |a| |b| = s (Cauchy-Schwarz): (E + 8) 2^-24 s bounds the absolute error."""
    from fourm.utils.clip import clip_logits
    g = torch.Generator().manual_seed(41)
    img, txt = torch.randn(5, 40, generator=g) * 2.0, torch.randn(7, 40, generator=g) * 0.3
    ls = math.log(1 / 0.07)
    scale = torch.nn.Parameter(torch.tensor(ls)).to(DEV) if as_tensor else ls
    li, lt = clip_logits(img.to(DEV), txt.to(DEV), scale)
    assert li.shape == (5, 7) and lt.shape == (7, 5) and li.dtype == torch.float32
    assert lt.data_ptr() == li.data_ptr() and torch.equal(lt, li.t())           # the transposed view
    s = math.exp(float(torch.tensor(ls)))                                        # (the parameter is fp32)
    i64, t64 = img.double(), txt.double()
    ref = s * (i64 / i64.norm(dim=-1, keepdim=True)) @ (t64 / t64.norm(dim=-1, keepdim=True)).t()
    err, bound = float((li.cpu().double() - ref).abs().max()), (40 + 8) * 2.0 ** -24 * s
    print(f"clip logits (tensor scale {as_tensor}): worst error {err:.3e} (bound {bound:.3e})")
    record("clip.logits", as_tensor=as_tensor, err=err, bound=bound)
    assert err <= bound


# ---- the score ----------------------------------------------------------------------------------------------------------------------------------
def test_clip_score_accumulates_the_definition():
    from fourm.utils.clip import ClipScore
    g = torch.Generator().manual_seed(51)
    f = [torch.randn(n, 40, generator=g) for n in (5, 5, 9, 9)]
    metric = ClipScore(None, None)
    assert metric.compute() != metric.compute()                                  # nan before anything was seen
    s1 = metric.update_features(f[0].to(DEV), f[1].to(DEV))
    s2 = metric.update_features(f[2].to(DEV), f[3].to(DEV))
    assert s1.shape == (5,) and s2.shape == (9,) and s1.dtype == torch.float32
    cos = torch.cat([torch.nn.functional.cosine_similarity(f[0].double(), f[1].double()), torch.nn.functional.cosine_similarity(f[2].double(), f[3].double())])
    want = max(float(100.0 * cos.mean()), 0.0)
    got = metric.compute()
    assert isinstance(got, float) and int(metric.count) == 14 and metric.sum.dtype == torch.float64 and metric.sum.is_cuda
    assert float(metric.sum) == math.fsum(s1.tolist() + s2.tolist())
    mean = float(100.0 * cos.mean())
    assert abs(got - max(mean, 0.0)) <= 4 * ULP_100 and (mean > 0) == (got > 0), (got, want)
    metric.reset()
    assert int(metric.count) == 0 and float(metric.sum) == 0.0
    # a negative mean is clamped: the clamp acts on the mean, the per-pair scores keep their sign
    neg = metric.update_features(f[0].to(DEV), (-f[0]).to(DEV))
    assert float(neg.max()) < -99.9 and metric.compute() == 0.0
    metric.reset()
    metric.update_features(f[0].to(DEV), f[0].to(DEV) * 3.0)
    assert abs(metric.compute() - 100.0) <= 4 * ULP_100


def test_clip_score_update_is_update_features_of_the_towers(models):
    from fourm.utils.clip import ClipScore, VisionTransformer
    text = models["text_a"]
    cfg = dict(V.CASES["clip_a"], output_dim=U.CASES["text_a"]["embed_dim"])
    sd = V.seeded_state_dict("clip_a")
    sd["proj"] = sd["proj"][:, :cfg["output_dim"]].contiguous()
    visual = VisionTransformer(**cfg)
    visual.load_state_dict(sd, strict=True)
    visual = visual.to(DEV).eval().requires_grad_(False)
    images, ids = V.images("clip_a", "native").to(DEV), U.token_ids("text_a").to(DEV)
    a, b = ClipScore(visual, text), ClipScore(visual, text)
    sa = a.update(images, ids)
    sb = b.update_features(visual(images).clone(), text(ids).clone())
    assert sa.shape == (3,) and torch.equal(sa, sb) and a.compute() == b.compute() and int(a.count) == 3
    with pytest.raises(ValueError, match="outside"):                             # the text tower's id check reaches the caller
        a.update(images, torch.full_like(ids, U.CASES["text_a"]["vocab_size"]))
    assert text(torch.full_like(ids, -1), check_ids=False).shape == (3, 40)      # ... and can be switched off


# ---- unchanged callers ----------------------------------------------------------------------------------------------------------------------------
def test_vision_tower_keeps_its_bits_around_a_text_forward(models):
    """The block loop's new keyword at its default, and no scratch or cache shared by name: VisionTransformer.forward on the clip_vit_micro case
    is the same bits before and after a text forward on the same device, in both precisions, and against a tower that never saw a text tower."""
    from fourm.utils.clip import VisionTransformer
    def tower():
        v = VisionTransformer(**V.CASES["clip_a"])
        v.load_state_dict(V.seeded_state_dict("clip_a"), strict=True)
        return v.to(DEV).eval().requires_grad_(False)
    visual, x = tower(), V.images("clip_a", "native").to(DEV)
    before = {f: visual(x, **V.flag_kwargs(f)).clone() for f in V.FLAGS}
    text, ids = models["text_a"], U.token_ids("text_a").to(DEV)
    t0 = text(ids).clone()
    for precision in ("bf16", "fp32"):
        run(text, ids, precision, return_all_tokens=True)
        for f in V.FLAGS:
            assert torch.equal(visual(x, **V.flag_kwargs(f)), before[f]), (precision, f)
    assert torch.equal(text(ids), t0)
    names = [k[0] for k in text.__dict__["_hip_engine"].ws.bufs]
    assert any(n.startswith("cliptext.") for n in names) and not any(n.startswith("clip.") for n in names)
    assert not any(k[0].startswith("cliptext") for k in visual.__dict__["_hip_engine"].ws.bufs)
