"""The attention bounds of tests/attn_f64_util.py, proven on the CPU before any GPU run:
  * they HOLD: for every case of the GPU table (same shapes, seeds, masks) a torch restatement of the kernels' rounding points stays
    inside them against the float64 reference;
  * they BITE: deliberately wrong restatements are rejected by the same ``within`` check, on a named element;
  * the float64 reference itself is torch.autograd's float64 result to 1e-12.
No test here runs the code under test."""
import re

import pytest
import torch

from tests import attn_f64_util as A
from tests.attn_f64_util import B, H, heads, within

MATH_CASES = list({c.math_key: c for c in A.CASES}.values())
WORST = {}


def run_emulation(c):
    """Emulated forward and backward of case ``c`` against the float64 reference and the bounds -> worst err / tol per output."""
    fx = A.fixture(c)
    blk = fx.mask.blocked
    sh = (B, H, c.Nq, c.Nk, fx.scale)
    ref = A.ref_forward(fx.q, fx.k, fx.v, *sh, blk, c.zero_attn)
    tO, tm, tl = A.fwd_bounds(fx.q, fx.k, fx.v, *sh, ref, blk)
    o, m, l = A.emu_forward(fx.q, fx.k, fx.v, *sh, blk, c.zero_attn)
    r = dict(O=within("O", heads(o, B, c.Nq, H), ref["O"], tO), m=within("stat_m", m, ref["m"], tm), l=within("stat_l", l, ref["l"], tl))
    rb = A.ref_backward(fx.q, fx.k, fx.v, o, fx.do, m, l, *sh, blk)
    tq, tk, tv = A.bwd_bounds(fx.q, fx.k, fx.v, o, fx.do, m, l, *sh, rb, blk)
    dq, dk, dv = A.emu_backward(fx.q, fx.k, fx.v, o, fx.do, m, l, *sh, blk)
    r.update(dQ=within("dQ", heads(dq, B, c.Nq, H), rb["dQ"], tq), dK=within("dK", heads(dk, B, c.Nk, H), rb["dK"], tk),
             dV=within("dV", heads(dv, B, c.Nk, H), rb["dV"], tv))
    return r, ref, rb, (tq, tk, tv)


@pytest.mark.parametrize("c", MATH_CASES, ids=lambda c: c.id)
def test_bounds_hold_under_emulation(c):
    r, ref, rb, (tq, tk, tv) = run_emulation(c)
    print(c.id, {k: f"{v:.3f}" for k, v in r.items()})
    for k, v in r.items():
        WORST[k] = max(WORST.get(k, 0.0), v)
        assert v < 1.0, (c.id, k, v)
    blk = A.fixture(c).mask.blocked
    if blk is not None:                                   # the structural zeros: the bound is EXACTLY zero there, so the test demands zero
        full = blk.all(-1)[:, None].expand(B, H, c.Nq)
        if not c.zero_attn:
            assert bool((tq[full] == 0).all()) and bool((rb["dQ"][full] == 0).all())
        dead = blk.all(-2)[:, None].expand(B, H, c.Nk)
        assert bool((tk[dead] == 0).all()) and bool((rb["dK"][dead] == 0).all())
        nofull = ~blk.all(-1).any(-1)                     # samples without a fully blocked row
        dead_v = dead & nofull[:, None, None]
        assert bool((tv[dead_v] == 0).all()) and bool((rb["dV"][dead_v] == 0).all())
    if c.zero_attn and blk is not None:                   # a fully blocked row under softmax1: O = 0, m = 0, l = 1
        full = blk.all(-1)[:, None].expand(B, H, c.Nq)
        assert bool((ref["O"][full] == 0).all()) and bool((ref["m"][full] == 0).all()) and bool((ref["l"][full] == 1).all())


def test_worst_ratio_is_reported():
    """Prints the worst err / tol per output over the whole table (DESIGN.md quotes it); gathers it itself when run alone."""
    if not WORST:
        for c in MATH_CASES:
            for k, v in run_emulation(c)[0].items():
                WORST[k] = max(WORST.get(k, 0.0), v)
    print("worst err/tol under emulation:", {k: round(v, 3) for k, v in WORST.items()})
    assert max(WORST.values()) < 1.0


def test_mask_fixtures_hold_the_required_cases():
    """What the GPU table relies on the fixtures to contain."""
    big = A.largest_modality_id()
    assert 2047 < big < 32768                             # beyond the 11-bit key field of the packed decoder compare, inside int16
    for Nq, Nk in ((128, 128), (96, 96), (130, 65), (544, 544)):
        mk = A.make_mask("dec", B, Nq, Nk, 1)
        assert bool((mk.cs == 0).any()) and bool((mk.cs > Nk).any()) and int(mk.cs.max()) > 1023
        ids = set(mk.modq.flatten().tolist())
        assert big in ids and len(ids) >= 3 and all(abs(a - b) > 1 for a in ids for b in ids if a != b)
        assert bool(mk.blocked.all(-1).any()) and not bool(mk.blocked.all())
        assert A.make_mask("dec_nomod", B, Nq, Nk, 1).modq is None and A.make_mask("dec_modonly", B, Nq, Nk, 1).cs is None
        kp = A.make_mask("keypad", B, Nq, Nk, 1).kpad
        assert bool(kp[0].all()) and bool(kp[1:].any(-1).all()) and not bool(kp[1:].all(-1).any())      # a whole blocked sample; padded and free keys elsewhere
        d = A.make_mask("dense", B, Nq, Nk, 1).dense
        assert bool(d.all(-1).any(-1).all()) and bool(d.all(-2).any(-1).all()) and not bool(d.all(-1).all())      # full rows and dead keys inside normal samples


def test_ramps_do_what_they_are_for():
    """rise: the row maximum moves in every 64-key tile (for some row of every head); fall: every row meets its maximum in the first tile."""
    for c in MATH_CASES:
        if c.ramp == "flat" or c.mask != "none" or c.Nk <= 64:
            continue
        fx = A.fixture(c)
        t = heads(fx.q, B, c.Nq, H) @ heads(fx.k, B, c.Nk, H).transpose(-1, -2)
        pad = (-c.Nk) % 64
        tm = torch.nn.functional.pad(t, (0, pad), value=-float("inf")).reshape(B, H, c.Nq, -1, 64).max(-1).values.cummax(-1).values
        if c.ramp == "fall":
            assert bool((tm[..., 0:1] == tm).all()), c.id
        else:
            assert bool((tm[..., 1:] > tm[..., :-1]).any(-2).all()), c.id


# ------------------------------------------------------------------------------------------------
# the bounds bite
# ------------------------------------------------------------------------------------------------
def case(Nq, Nk, mask, zero_attn=False):
    return next(c for c in MATH_CASES if (c.Nq, c.Nk, c.mask, c.zero_attn, c.ramp) == (Nq, Nk, mask, zero_attn, "flat"))


def fwd_setup(c):
    fx = A.fixture(c)
    sh = (B, H, c.Nq, c.Nk, fx.scale)
    ref = A.ref_forward(fx.q, fx.k, fx.v, *sh, fx.mask.blocked, c.zero_attn)
    return fx, sh, ref, A.fwd_bounds(fx.q, fx.k, fx.v, *sh, ref, fx.mask.blocked)


def rejected(name, got, ref, tol):
    with pytest.raises(AssertionError, match=re.escape(name) + r": \d+ of \d+ outside the bound.*first at \(\d+, \d+, \d+"):
        within(name, got, ref, tol)


@pytest.mark.parametrize("Nq,Nk,mask", [(128, 128, "keypad"), (130, 65, "dense"), (96, 96, "dec")])
def test_rejects_one_leaking_key(Nq, Nk, mask):
    """One blocked key of one (non-full) row treated as unblocked."""
    c = case(Nq, Nk, mask)
    fx, sh, ref, (tO, tm, tl) = fwd_setup(c)
    blk = fx.mask.blocked.clone()
    b = B - 1
    rows = (~blk[b].all(-1)).nonzero().flatten()
    q = int(rows[len(rows) // 2])
    k = int(blk[b, q].nonzero().flatten()[0])
    blk[b, q, k] = False
    o, m, l = A.emu_forward(fx.q, fx.k, fx.v, *sh, blk, False)
    rejected("O", heads(o, B, Nq, H), ref["O"], tO)
    rejected("stat_l", l, ref["l"], tl)


@pytest.mark.parametrize("Nq,Nk,mask", [(96, 96, "dec"), (128, 128, "dec_nomod")])
def test_rejects_the_decoder_bound_off_by_one(Nq, Nk, mask):
    c = case(Nq, Nk, mask)
    fx, sh, ref, (tO, tm, tl) = fwd_setup(c)
    wrong = A.decoder_blocked(fx.mask.cs, fx.mask.modq, fx.mask.modk, Nq, Nk, off_by_one=True)
    o, m, l = A.emu_forward(fx.q, fx.k, fx.v, *sh, wrong, False)
    rejected("O", heads(o, B, Nq, H), ref["O"], tO)


@pytest.mark.parametrize("Nq,Nk,mask", [(33, 70, "none"), (130, 65, "keypad")])
def test_rejects_the_first_key_past_Nk(Nq, Nk, mask):
    c = case(Nq, Nk, mask)
    fx, sh, ref, (tO, tm, tl) = fwd_setup(c)
    g = torch.Generator().manual_seed(5)
    ext = lambda x: torch.cat([x.reshape(B, Nk, -1), (torch.randn(B, 1, x.shape[1], generator=g) * 1.5).bfloat16()], 1).reshape(B * (Nk + 1), -1)
    blk = None if fx.mask.blocked is None else torch.cat([fx.mask.blocked, torch.zeros(B, Nq, 1, dtype=torch.bool)], -1)
    o, m, l = A.emu_forward(fx.q, ext(fx.k), ext(fx.v), B, H, Nq, Nk + 1, fx.scale, blk, False)
    rejected("O", heads(o, B, Nq, H), ref["O"], tO)
    rejected("stat_l", l, ref["l"], tl)


@pytest.mark.parametrize("Nq,Nk,mask", [(128, 128, "keypad"), (64, 64, "dense"), (96, 96, "dec")])
def test_rejects_a_zero_output_in_a_fully_blocked_row(Nq, Nk, mask):
    c = case(Nq, Nk, mask)
    fx, sh, ref, (tO, tm, tl) = fwd_setup(c)
    assert bool(fx.mask.blocked.all(-1).any())
    o, m, l = A.emu_forward(fx.q, fx.k, fx.v, *sh, fx.mask.blocked, False, full_row_zero=True)
    rejected("O", heads(o, B, Nq, H), ref["O"], tO)


def test_rejects_the_next_heads_V():
    c = case(128, 128, "none")
    fx, sh, ref, (tO, tm, tl) = fwd_setup(c)
    o, m, l = A.emu_forward(fx.q, fx.k, fx.v.roll(-A.HD, 1), *sh, None, False)
    rejected("O", heads(o, B, 128, H), ref["O"], tO)


def test_rejects_zero_attn_ignored_in_l():
    c = case(64, 64, "none", True)
    fx, sh, ref, (tO, tm, tl) = fwd_setup(c)
    o, m, l = A.emu_forward(fx.q, fx.k, fx.v, *sh, None, True, zero_attn_not_in_l=True)
    rejected("stat_l", l, ref["l"], tl)                  # (with row maxima of several bits the zero logit hardly moves O: stat_l is what the backward reads)


def bwd_setup(c):
    fx = A.fixture(c)
    sh = (B, H, c.Nq, c.Nk, fx.scale)
    blk = fx.mask.blocked
    o, m, l = A.emu_forward(fx.q, fx.k, fx.v, *sh, blk, c.zero_attn)
    rb = A.ref_backward(fx.q, fx.k, fx.v, o, fx.do, m, l, *sh, blk)
    return fx, sh, (o, m, l), rb, A.bwd_bounds(fx.q, fx.k, fx.v, o, fx.do, m, l, *sh, rb, blk)


@pytest.mark.parametrize("Nq,Nk,mask", [(128, 128, "keypad"), (64, 64, "dense"), (96, 96, "dec")])
def test_rejects_dS_kept_in_a_fully_blocked_row(Nq, Nk, mask):
    c = case(Nq, Nk, mask)
    fx, sh, (o, m, l), rb, (tq, tk, tv) = bwd_setup(c)
    dq, dk, dv = A.emu_backward(fx.q, fx.k, fx.v, o, fx.do, m, l, *sh, fx.mask.blocked, ds_in_full_rows=True)
    rejected("dQ", heads(dq, B, Nq, H), rb["dQ"], tq)
    rejected("dK", heads(dk, B, Nk, H), rb["dK"], tk)


@pytest.mark.parametrize("Nq,Nk,mask", [(128, 128, "none"), (33, 70, "keypad")])
def test_rejects_a_missing_delta(Nq, Nk, mask):
    c = case(Nq, Nk, mask)
    fx, sh, (o, m, l), rb, (tq, tk, tv) = bwd_setup(c)
    dq, dk, dv = A.emu_backward(fx.q, fx.k, fx.v, o, fx.do, m, l, *sh, fx.mask.blocked, no_delta=True)
    rejected("dQ", heads(dq, B, Nq, H), rb["dQ"], tq)
    rejected("dK", heads(dk, B, Nk, H), rb["dK"], tk)


def test_rejects_scale_applied_twice_to_dK():
    c = case(128, 128, "none")
    fx, sh, (o, m, l), rb, (tq, tk, tv) = bwd_setup(c)
    dq, dk, dv = A.emu_backward(fx.q, fx.k, fx.v, o, fx.do, m, l, *sh, None, scale_twice_dk=True)
    rejected("dK", heads(dk, B, 128, H), rb["dK"], tk)
    within("dQ", heads(dq, B, 128, H), rb["dQ"], tq)      # (the mutation touches dK alone)


# ------------------------------------------------------------------------------------------------
# the reference against torch.autograd in float64
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask,zero_attn", [("none", False), ("keypad", False), ("dec", False), ("causal", False), ("dense", False),
                                            ("none", True), ("dense", True)])
def test_reference_is_autograd_in_float64(mask, zero_attn):
    Nq, Nk = (40, 40) if mask in ("dec", "causal") else (33, 40)
    mk = A.make_mask(mask, B, Nq, Nk, seed=3)
    q, k, v, do = A.make_inputs(B, H, Nq, Nk, 11, "flat", mk.kpad)
    scale = A.HD ** -0.5
    ref = A.ref_forward(q, k, v, B, H, Nq, Nk, scale, mk.blocked, zero_attn)
    qh, kh, vh = (heads(x, B, n, H).requires_grad_(True) for x, n in ((q, Nq), (k, Nk), (v, Nk)))
    s = (qh @ kh.transpose(-1, -2)) * scale
    if mk.blocked is not None:
        s = s.masked_fill(mk.blocked[:, None], A.NEG_FILL)
    if zero_attn:                                         # softmax1 (fm_utils.py): a zero logit joins the softmax, its probability is dropped
        p = torch.softmax(torch.cat([s, torch.zeros_like(s[..., :1])], -1), -1)[..., :-1]
    else:
        p = torch.softmax(s, -1)
    out = p @ vh
    out.backward(heads(do, B, Nq, H))
    sc = lambda x: float(x.detach().abs().max()) + 1e-300
    assert float((ref["O"] - out.detach()).abs().max()) <= 1e-12 * sc(out)
    assert float((ref["P"] - p.detach()).abs().max()) <= 1e-12
    # the reference backward from the reference's own o, m, l (float64: nothing is rounded)
    o64 = A.unheads(ref["O"])
    rb = A.ref_backward(q.double(), k.double(), v.double(), o64, do.double(), ref["m"], ref["l"], B, H, Nq, Nk, scale, mk.blocked)
    for name, want in (("dQ", qh.grad), ("dK", kh.grad), ("dV", vh.grad)):
        assert float((rb[name] - want).abs().max()) <= 1e-12 * sc(want), name
