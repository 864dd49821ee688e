"""The reference of tests/select_embed_util.py proved without a GPU: it reproduces the upstream-recorded fixtures exactly, agrees with the
oracle's independent formulation on irregular batches the fixtures do not contain, and its autograd backward passes a finite-difference
check.  tests/test_select_embed_kernels_gpu.py then holds the HIP kernels to it."""
import os

import numpy as np
import pytest
import torch

from oracle import fourm_oracle as O
from tests import select_embed_util as S
from tests.golden.cases import build_case

GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.mark.parametrize("name", ["micro_swiglu", "micro_pad", "micro_gelu"])
def test_reference_reproduces_upstream_fixtures(name):
    g = np.load(os.path.join(GOLD, f"{name}.npz"))
    case = build_case(name)
    cfg = case["cfg"]
    enc_order = [n for n in case["mod_dict"] if cfg.mod(n).in_enc]
    e = S.reference(S.side_from_case(case, False, enc_order))
    assert np.array_equal(e["out_mask"].bool()[:, None, :].numpy(), g["enc/mask"])
    assert np.array_equal(e["out_mod"].numpy(), g["enc/mod_mask"])
    assert np.array_equal(e["emb"].numpy(), g["enc/emb"])
    d = S.reference(S.side_from_case(case, True, g["meta/order"].tolist()))
    assert np.array_equal(d["out_mask"].bool()[:, None, :].numpy(), g["dec/mask"])
    assert np.array_equal(d["out_mod"].numpy(), g["dec/mod_mask"])
    assert np.array_equal(d["target_ids"].numpy(), g["dec/target_ids"])
    assert np.array_equal(d["emb"].numpy(), g["dec/emb"])
    assert np.array_equal(d["tokens"].numpy(), g["dec/tokens"])
    dense = S.dense_mask_reference(d["out_cs"], d["out_mod_pre"], cfg.causal, True, cfg.sep)
    assert np.array_equal(np.packbits(dense.numpy(), axis=-1), g["dec/attn_mask"])
    # the fixtures exercise what they are meant to: registers, padding slots and an empty head
    if name == "micro_gelu":
        assert bool((e["slot_mod"][:, :2] == -2).all())
    if name == "micro_pad":
        assert bool(e["out_mask"].any()) and bool(d["out_mask"].any())


def irregular_sides():
    """Three of the irregular cases of the GPU file: scattered sequence masks, truncation inside a modality, max_len collapse."""
    enc = [(S.SEQ, 9, {}), (S.TOK, 6, {}), (S.SEQ_EMB, 7, {}), (S.PATCH, 4, dict(grid_w=2))]
    dec = [(S.SEQ, 9, dict(max_len=20)), (S.TOK, 6, {}), (S.SEQ, 5, dict(max_len=20))]
    yield "scattered_enc", S.make_side(1, enc, B=3, D=8, n_keep=26)
    yield "scattered_dec", S.make_side(2, dec, B=3, D=8, n_keep=20, is_decoder=True)
    yield "truncated_enc", S.make_side(3, enc, B=3, D=8, n_keep=5, p_mask=0.2)
    yield "truncated_dec", S.make_side(4, dec, B=3, D=8, n_keep=4, is_decoder=True, p_mask=0.1)
    yield "max_len_collapse", S.make_side(5, [(S.SEQ, 12, dict(max_len=3)), (S.TOK, 4, {})], B=2, D=8, n_keep=14, is_decoder=True, p_mask=0.1)


@pytest.mark.parametrize("label,side", list(irregular_sides()), ids=[n for n, _ in irregular_sides()])
def test_reference_equals_oracle_on_irregular_batches(label, side):
    """Two independent formulations (float argsort here, integer prefix sums in the oracle, which is pinned to upstream by
    tests/test_oracle_golden.py) agree on ids_keep, the masks, the modality ids and the embedding rows."""
    r = S.reference(side)
    P, cfg, md, order = S.to_oracle(side)
    if side.is_decoder:
        o = O.select_decoder(P, cfg, md, side.n_keep, order)
        assert torch.equal(o["target_ids"], r["target_ids"])
        assert torch.equal(o["dam"].int(), r["dam"].int())
        assert torch.equal(o["attn_mask"], S.dense_mask_reference(r["out_cs"], r["out_mod_pre"], cfg.causal, True, cfg.sep))
    else:
        o = O.select_encoder(P, cfg, md, side.n_keep, O._Num(False))
    assert torch.equal(o["ids_keep"], r["ids_keep"])
    assert torch.equal(o["mask"][:, 0], r["out_mask"].bool())
    assert torch.equal(o["mod_mask"], r["out_mod"])
    assert torch.equal(o["emb"], r["emb"])
    assert torch.equal(o["tokens"], r["tokens"])
    if label == "max_len_collapse":
        used = r["slot_pos"][r["slot_mod"] == 0]
        assert int(used.max()) == 2 and int((used == 0).sum()) > side.B       # ranks >= 3 wrapped to row 0
    if label.startswith("truncated"):
        assert not bool(r["out_mask"].any())                                   # more selectable positions than n_keep in every sample


def test_backward_reference_finite_differences():
    """d/dtheta sum(x0 * dx) by central differences in float64 (x0 is linear in every parameter: exact up to rounding)."""
    side = S.make_side(7, [(S.SEQ, 4, dict(learned_pos=True, padding_idx=1, vocab=3)), (S.TOK, 3, dict(learned_pos=True, vocab=4)),
                           (S.SEQ_EMB, 3, dict(learned_pos=True))], B=2, D=4, n_keep=7, n_reg=1, p_mask=0.3)
    dx = torch.randn(side.B, side.Nt, side.D, generator=S.gen(8), dtype=torch.float64)
    grads, _ = S.reference_backward(side, dx)

    def f(P):
        return float((S.reference(side, P, torch.float64)["x0"] * dx).sum())

    checked = 0
    for name, (gr, n, s_abs) in grads.items():
        P = S.params_of(side, torch.float64)
        t = P[name] if isinstance(name, str) else P["mods"][name[1]][name[0]]
        fd = torch.zeros_like(t)
        flat, fdf = t.view(-1), fd.view(-1)
        for k in range(flat.numel()):
            old = float(flat[k])
            flat[k] = old + 0.5
            hi = f(P)
            flat[k] = old - 0.5
            lo = f(P)
            flat[k] = old
            fdf[k] = hi - lo
        if isinstance(name, tuple) and name[0] == "table" and side.mods[name[1]].padding_idx is not None:
            pad = side.mods[name[1]].padding_idx
            assert bool((gr[pad] == 0).all()) and bool((n[pad] == 0).all())   # F.embedding(padding_idx): no gradient, though x0 depends on it
            fd[pad] = 0
        assert torch.allclose(fd, gr, rtol=0, atol=1e-12), name
        assert bool((s_abs + 1e-12 >= gr.abs()).all()) and bool((n == n.round()).all()) and bool(((n == 0) == (s_abs == 0)).all()), name
        checked += flat.numel()
    assert checked > 50
