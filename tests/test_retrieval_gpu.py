"""The flat k-NN index on a real MI355X against the float64 brute-force reference of tests/retrieval_util.py.

Integer inputs (entries in [-3, 3], d <= 1024): every product, sum, |x|^2, key and distance is an exact fp32 integer below 2^24 in any
summation order, so D and I must EQUAL the reference, ties included (lowest index first) - no tolerance.  Real-valued inputs: with u = 2^-24
the fp32 selection key is within E_q = (d + 2) u (|q| + max |x|)^2 (l2) or (d + 1) u |q| max |x| (ip) of float64, so every returned row is
within E_q of the k-th float64 value and every row more than E_q inside it is returned; the reported distance is a sum of non-negative
terms, |D - d64| <= (d + 3) u d64 (ip: |D - s64| <= (d + 1) u sum |q_i x_i|).  For at least 85 % of the recipes' queries the float64 gap at
rank k exceeds 2 E_q (asserted first), so their result sets are fixed by float64 alone.  Everything else is bit for bit: a query alone or in
a batch (the 32- and 128-wide query tiles), one add or two, any forced gallery split, two calls, numpy or torch queries."""
import ctypes

import numpy as np
import pytest
import torch

from tests import memcodes_util as M
from tests import retrieval_util as R

pytestmark = pytest.mark.gpu

_REF = {}


def reference(case, metric):
    """(Q, X, D64, I) of an integer case: computed once, shared, left unchanged."""
    if (case, metric) not in _REF:
        nq, n, d, k = case
        Q, X = R.integer_case(nq, n, d, k)
        _REF[(case, metric)] = (Q, X) + R.brute_force(Q, X, k, metric)
    return _REF[(case, metric)]


def index_of(X, metric):
    from fourm.utils.retrieval import FlatIndex
    ix = FlatIndex(X.shape[1], metric)
    ix.add(X)
    return ix


@pytest.mark.parametrize("metric", ["l2", "ip"])
@pytest.mark.parametrize("case", R.INTEGER_CASES, ids=lambda c: "x".join(map(str, c)))
def test_integer_inputs_equal_the_reference(case, metric):
    nq, n, d, k = case
    Q, X, D64, I64 = reference(case, metric)
    ix = index_of(torch.from_numpy(X), metric)
    assert ix.ntotal == n and tuple(ix.vectors.shape) == (n, d) and torch.equal(ix.vectors.cpu(), torch.from_numpy(X))
    want_D, want_I = torch.from_numpy(D64.astype(np.float32)), torch.from_numpy(I64)
    for splits in (None,) + R.FORCED_SPLITS:                                   # the split chosen for the device, then the forced ones
        if splits is not None and splits * k > 4096:
            continue
        D, I = ix.search(torch.from_numpy(Q).cuda(), k, splits=splits)
        assert D.dtype == torch.float32 and I.dtype == torch.int64 and D.shape == I.shape == (nq, k) and D.is_cuda
        assert torch.equal(I.cpu(), want_I), (splits, (I.cpu() != want_I).nonzero()[:4].tolist())
        assert torch.equal(D.cpu(), want_D), splits
    for tile in (32, 128):                                                     # both tile widths, whatever nq would pick
        D, I = ix.search(torch.from_numpy(Q).cuda(), k, query_tile=tile)
        assert torch.equal(I.cpu(), want_I) and torch.equal(D.cpu(), want_D), tile


@pytest.mark.parametrize("metric", ["l2", "ip", "cosine"])
@pytest.mark.parametrize("name", ["A", "B"])
def test_real_inputs_stay_inside_the_band(name, metric):
    from fourm.hip import ops
    Q, X, k = R.recipe(name)
    ix = index_of(X, metric)                                                   # numpy in ...
    D, I = ix.search(Q, k)
    assert isinstance(D, np.ndarray) and isinstance(I, np.ndarray) and D.dtype == np.float32 and I.dtype == np.int64          # ... numpy out
    base = "l2" if metric == "l2" else "ip"
    if metric == "cosine":                                                     # the ip statement on the rows as the index normalised them
        X = ix.vectors.cpu().numpy()
        Q = ops.l2_normalize_rows(torch.from_numpy(Q).cuda()).cpu().numpy()
        assert np.allclose((X.astype(np.float64) ** 2).sum(1), 1.0, atol=1e-5)
    val, E = R.scores64(Q, X, base), R.band(Q, X, base)
    share = float(R.determined(val, k, E, base).mean())
    print(f"recipe {name} {metric}: determined share {share:.3f}")
    assert share >= 0.85, share
    worst = R.check_band(val, k, E, base, D, I, Q, X)
    print(f"recipe {name} {metric}: worst |D - ref| / bound {worst:.3f}")
    fixed = R.determined(val, k, E, base)                                      # where float64 fixes the set, the sets are equal
    I64 = R.brute_force(Q, X, k, base)[1]
    assert all(set(I[i].tolist()) == set(I64[i].tolist()) for i in np.nonzero(fixed)[0])


def test_invariances_bit_for_bit():
    from fourm.utils.retrieval import FlatIndex, knn_refine_l2, knn_search
    Q, X, k = R.recipe("A")
    Qd, Xd = torch.from_numpy(Q).cuda(), torch.from_numpy(X).cuda()
    for metric in ("l2", "ip", "cosine"):
        ix = index_of(Xd, metric)
        D, I = ix.search(Qd, k)
        D2, I2 = ix.search(Qd, k)                                              # two identical calls
        assert torch.equal(D, D2) and torch.equal(I, I2)
        for i in (0, 63, 64, 129):                                             # a query alone (the 32-wide tile) or in its batch (the 128-wide one)
            Di, Ii = ix.search(Qd[i:i + 1], k)
            assert torch.equal(Di[0], D[i]) and torch.equal(Ii[0], I[i]), (metric, i)
        D32, I32 = ix.search(Qd, k, query_tile=32)
        assert torch.equal(D32, D) and torch.equal(I32, I)
        two = FlatIndex(X.shape[1], metric)                                    # 1000 + 3099 rows: storage grows once
        two.add(Xd[:1000])
        two.add(X[1000:])
        assert two.ntotal == ix.ntotal == 4099 and torch.equal(two.vectors, ix.vectors)
        Dt, It = two.search(Qd, k)
        assert torch.equal(Dt, D) and torch.equal(It, I), metric
        Dn, In = ix.search(Q, k)                                               # a numpy query: the numpy image of the torch result
        assert np.array_equal(Dn, D.cpu().numpy()) and np.array_equal(In, I.cpu().numpy())
    # forced splits through the low-level entry point, keys included
    ix = index_of(Xd, "l2")
    x, xn = ix._store[:ix.ntotal], ix._norms[:ix.ntotal]
    for metric in ("l2", "ip"):
        outs = [knn_search(Qd, x, xn if metric == "l2" else None, k, metric, splits=s, query_tile=t) for s in R.FORCED_SPLITS for t in (0, 32)]
        for Ds, Is in outs[1:]:
            assert torch.equal(Ds, outs[0][0]) and torch.equal(Is, outs[0][1]), metric
    Dk, Ik = knn_search(Qd, x, xn, k, "l2", splits=7)
    Dr, Ir = knn_refine_l2(Qd, x, Dk.clone(), Ik.clone())
    D, I = ix.search(Qd, k)
    assert torch.equal(Dr, D) and torch.equal(Ir, I)
    assert torch.equal(Ir.sort(dim=1).values, Ik.sort(dim=1).values)           # the refinement re-orders, it does not re-select


def test_addressing_past_4_gib():
    """n = 2^20 + 3 rows of d = 1024: 4.29 GB, the last row starts past 2^32 bytes.  The query is a copy of the last row."""
    from fourm.utils.retrieval import FlatIndex
    n, d = 2 ** 20 + 3, 1024
    ix = FlatIndex(d, "l2")
    X = torch.randn(n, d, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))      # filled on the device from a seed
    ix.add(X)
    del X
    assert ix.ntotal == n and ix.vectors.data_ptr() % 16 == 0 and (n - 1) * d * 4 > 2 ** 32
    D, I = ix.search(ix.vectors[n - 1:].clone(), 3)
    assert int(I[0, 0]) == n - 1 and float(D[0, 0]) == 0.0 and float(D[0, 1]) > 0.0


def test_c_entry_points_refuse_bad_arguments_and_write_nothing():
    from fourm.hip import _lib as L
    nq, n, d, k = 3, 200, 8, 4
    q = torch.ones(nq, d, device="cuda")
    x = torch.ones(n, d, device="cuda")
    xn = torch.ones(n, device="cuda")
    scratch = torch.zeros(nq * 2 * k, dtype=torch.int64, device="cuda")
    D = torch.full((nq, k), 7.0, device="cuda")
    I = torch.full((nq, k), 7, dtype=torch.int64, device="cuda")
    P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def search(q=q, nq=nq, x=x, xn=xn, n=n, d=d, k=k, metric=L.KNN_L2, splits=2, tile=0, scratch=scratch, nbytes=None, D=D, I=I, qoff=0):
        nbytes = nq * 2 * k * 8 if nbytes is None else nbytes
        qp = ctypes.c_void_p(q.data_ptr() + qoff) if q is not None else None
        return L.knn_search(qp, nq, P(x), P(xn), n, d, k, metric, splits, tile, P(scratch), nbytes, P(D), P(I), stream)

    bad = [dict(q=None), dict(x=None), dict(scratch=None), dict(D=None), dict(I=None), dict(xn=None), dict(nq=0), dict(n=0), dict(d=6), dict(d=0),
           dict(d=4100), dict(k=0), dict(k=L.KNN_MAX_K + 1), dict(metric=2), dict(splits=0), dict(splits=L.KNN_MAX_MERGE // k + 1), dict(tile=64),
           dict(nbytes=nq * 2 * k * 8 - 8), dict(qoff=4)]
    for kw in bad:
        assert search(**kw) == -1, kw
        assert b"fm_knn_search" in L.lib.fm_last_error(), kw
    assert search(xn=None, metric=L.KNN_IP) == 0                               # the norms are not needed for ip
    torch.cuda.synchronize()
    assert bool((D == float(d)).all()) and I[:, 0].tolist() == [0, 0, 0]
    D.fill_(7.0)
    I.fill_(7)
    for args in ((None, nq, P(x), n, d, k, P(D), P(I)), (P(q), nq, None, n, d, k, P(D), P(I)), (P(q), nq, P(x), n, d, k, None, P(I)),
                 (P(q), nq, P(x), n, d, k, P(D), None), (P(q), 0, P(x), n, d, k, P(D), P(I)), (P(q), nq, P(x), 0, d, k, P(D), P(I)),
                 (P(q), nq, P(x), n, 7, k, P(D), P(I)), (P(q), nq, P(x), n, d, 0, P(D), P(I)), (P(q), nq, P(x), n, d, L.KNN_MAX_K + 1, P(D), P(I))):
        assert L.knn_refine_l2(*args, stream) == -1 and b"fm_knn_refine_l2" in L.lib.fm_last_error(), args
    for args in ((None, n, d, P(xn)), (P(x), n, d, None), (P(x), 0, d, P(xn)), (P(x), n, 6, P(xn)), (P(x), n, 4100, P(xn))):
        assert L.row_sqnorms(*args, stream) == -1 and b"fm_row_sqnorms" in L.lib.fm_last_error(), args
    torch.cuda.synchronize()
    assert bool((D == 7.0).all()) and bool((I == 7).all()) and bool((xn == 1.0).all())
    # an index outside the gallery is padding for the refinement, never an offset
    I[:] = torch.tensor([0, n, -1, 5], device="cuda")
    assert L.knn_refine_l2(P(q), nq, P(x), n, d, k, P(D), P(I), stream) == 0
    assert I.tolist() == [[0, 5, -1, -1]] * nq and D[:, :2].tolist() == [[0.0, 0.0]] * nq and bool(torch.isinf(D[:, 2:]).all())


def test_python_refusals_leave_the_last_error_alone():
    from fourm.hip import _lib as L
    from fourm.utils.retrieval import MAX_K, FlatIndex
    ix = index_of(torch.ones(5, 8, device="cuda"), "l2")
    before = L.lib.fm_last_error()
    for call in (lambda: ix.search(torch.ones(1, 9, device="cuda"), 1), lambda: ix.search(torch.ones(1, 8, device="cuda"), 0),
                 lambda: ix.search(torch.ones(1, 8, device="cuda"), MAX_K + 1), lambda: ix.add(torch.ones(1, 8, device="cuda").long()),
                 lambda: FlatIndex(8, "dot")):
        with pytest.raises(ValueError):
            call()
    assert L.lib.fm_last_error() == before and ix.ntotal == 5
    # an empty index and an empty query launch no search; reset empties; growth keeps the rows
    empty = FlatIndex(8, "ip")
    D, I = empty.search(torch.ones(2, 8), 3)
    assert bool((I == -1).all()) and bool((D == float("-inf")).all()) and D.is_cuda
    D, I = ix.search(torch.ones(0, 8), 3)
    assert D.shape == I.shape == (0, 3)
    ix.add(np.full((4, 8), 2.0, dtype=np.float64))
    assert ix.ntotal == 9 and ix.vectors[:5].eq(1).all() and ix.vectors[5:].eq(2).all()
    D, I = ix.search(torch.full((1, 8), 2.0), 9)
    assert I[0].tolist() == [5, 6, 7, 8, 0, 1, 2, 3, 4] and D[0].tolist() == [0.0] * 4 + [8.0] * 5
    ix.reset()
    assert ix.ntotal == 0 and tuple(ix.vectors.shape) == (0, 8)
    moved = index_of(torch.ones(3, 8), "l2").to("cuda:0")
    assert moved.search(torch.ones(1, 8), 1)[1].tolist() == [[0]]


# ---- glue: tokens -> embeddings -> neighbours, on the small MLP + Memcodes tokenizer ----
@pytest.fixture(scope="module")
def tokenizer():
    from fourm.vq import VQVAE
    c = M.CASES["bmlp_small"]
    m = VQVAE(**M.kwargs(c))
    m.load_state_dict(M.state_dict(c), strict=True)
    return m.cuda().eval()


@pytest.mark.parametrize("B", [1, 5])
def test_global_embeddings_are_the_decoded_tokens(tokenizer, B):
    from fourm.utils.retrieval import global_embeddings
    tokens = torch.randint(0, 50, (B, 4), generator=torch.Generator().manual_seed(B)).cuda()
    want = tokenizer.decode_tokens(tokens.view(B, 4, 1, 1)).reshape(B, 24)
    for form in (tokens, tokens.view(B, 4, 1, 1), tokens.int(), {"tensor": tokens}):
        got = global_embeddings(form, tokenizer)
        assert got.dtype == torch.float32 and tuple(got.shape) == (B, 24) and torch.equal(got, want)
    with pytest.raises(ValueError, match="4 heads"):
        global_embeddings(tokens[:, :3], tokenizer)


def test_retrieval_set_returns_the_item_and_its_payload(tokenizer, tmp_path):
    from fourm.utils.retrieval import RetrievalSet
    g = torch.Generator().manual_seed(9)
    tokens = torch.randint(0, 50, (50, 4), generator=g)
    tokens[17] = torch.tensor([49, 0, 31, 7])
    twin = (tokens == tokens[17]).all(1)
    twin[17] = False
    tokens[twin] = 1                                                           # item 17 is the only one with its tokens
    payload = {"tok_depth": torch.randint(0, 1000, (50, 9), generator=g), "row": torch.arange(50)}
    rs = RetrievalSet(tokenizer, metric="l2")
    rs.add_tokens(tokens[:20].cuda(), {k: v[:20] for k, v in payload.items()})
    rs.add_tokens(tokens[20:], {k: v[20:].cuda() for k, v in payload.items()})
    assert len(rs) == 50 and not rs.embeddings.is_cuda and not rs.payload["row"].is_cuda
    D, I, rows = rs.query_tokens(tokens[17:18], 3)
    assert int(I[0, 0]) == 17 and float(D[0, 0]) == 0.0                        # the MLP decode is batch-invariant: the same bits alone
    assert torch.equal(rows["tok_depth"][0, 0], payload["tok_depth"][17]) and rows["row"][0].tolist() == I[0].tolist()
    assert tuple(rows["tok_depth"].shape) == (1, 3, 9)
    out_dict = {"tok_dinov2_global": {"tensor": tokens[17:18].cuda()}, "tok_depth": {"tensor": torch.zeros(1, 9)}}
    D2, I2, rows2 = rs.query(out_dict, "tok_dinov2_global", 3)
    assert torch.equal(D2, D) and torch.equal(I2, I) and torch.equal(rows2["tok_depth"], rows["tok_depth"])
    with pytest.raises(ValueError, match="tok_imagebind_global"):
        rs.query(out_dict, "tok_imagebind_global", 3)
    path = str(tmp_path / "set.pth")
    rs.save(path)
    back = RetrievalSet.load(path, tokenizer)
    D3, I3, rows3 = back.query_tokens(tokens[17:18], 3)
    assert torch.equal(D3, D) and torch.equal(I3, I) and torch.equal(rows3["row"], rows["row"])
