"""Retrieval without a GPU: the module imports, the new C symbols are declared, exported and bound (FM_ABI_VERSION stays 11), every
Python-level refusal fires before a device is touched, a CPU index says that there is no CPU path, RetrievalSet round-trips host tensors,
and the float64 yardstick of the GPU tests (tests/retrieval_util.py) is itself pinned: a hand-worked case with a tie, and the share of
queries of the two real-valued recipes whose neighbours are decided by float64 alone."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import retrieval_util as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["fm_row_sqnorms", "fm_knn_query_tile", "fm_knn_splits", "fm_knn_scratch_bytes", "fm_knn_search", "fm_knn_refine_l2"]


def test_module_imports_and_names():
    from fourm.utils import retrieval
    for name in ("FlatIndex", "IndexFlatL2", "IndexFlatIP", "RetrievalSet", "global_embeddings"):
        assert hasattr(retrieval, name), name
    assert retrieval.MAX_K >= 64
    ix = retrieval.IndexFlatL2(7)
    assert (ix.d, ix.ntotal, ix.metric) == (7, 0, "l2") and retrieval.IndexFlatIP(7).metric == "ip"


def test_new_symbols_are_declared_exported_and_bound():
    from fourm.hip import _lib
    from fourm.utils import retrieval
    header = open(os.path.join(ROOT, "include", "fourm_hip.h")).read()
    assert re.search(r"#define FM_ABI_VERSION 11\b", header) and _lib.ABI_VERSION == 11 and _lib.lib.fm_abi_version() == 11
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib.EXPORTS and hasattr(_lib.lib, name), name
        assert getattr(_lib.lib, name).restype is ctypes.c_int
    assert len(_lib.knn_search.argtypes) == 15 and len(_lib.knn_refine_l2.argtypes) == 9 and len(_lib.row_sqnorms.argtypes) == 5
    assert "knn.hip" in open(os.path.join(ROOT, "ml-4m_amd", "build_ext.py")).read()
    for macro, value in (("FM_KNN_MAX_K", _lib.KNN_MAX_K), ("FM_KNN_MAX_D", _lib.KNN_MAX_D), ("FM_KNN_MAX_MERGE", _lib.KNN_MAX_MERGE),
                         ("FM_KNN_IP", _lib.KNN_IP), ("FM_KNN_L2", _lib.KNN_L2)):
        assert int(re.search(r"#define %s (\d+)\b" % macro, header).group(1)) == value, macro
    assert retrieval.MAX_K == _lib.KNN_MAX_K >= 64 and retrieval.MAX_D == _lib.KNN_MAX_D


def test_host_functions_and_host_side_refusals():
    """The host functions compute without a GPU; null pointers and sizes out of range come back as -1 with a message."""
    from fourm.hip import _lib
    assert _lib.knn_query_tile(1) == 32 and _lib.knn_query_tile(64) == 32 and _lib.knn_query_tile(65) == 128 and _lib.knn_query_tile(0) == -1
    # one query over a long gallery is split so that it fills the chip; many queries over a short one are not split further than needed
    s1 = _lib.knn_splits(1, 1_000_000, 5, 256)
    assert 256 <= s1 and s1 * 5 <= _lib.KNN_MAX_MERGE
    assert _lib.knn_splits(1, 1_000_000, 64, 256) == 64                        # capped by the merge width
    assert _lib.knn_splits(100_000, 1000, 10, 256) == 1
    assert _lib.knn_splits(5, 100, 1, 256) == 1                                # a single tile cannot be split
    for n, s in ((4099, 7), (1000, 2), (129, 2)):
        per = R.chunk_rows(n, s)
        assert per % 128 == 0 and per * s >= n
    assert _lib.knn_splits(0, 10, 1, 256) == -1 and b"fm_knn_splits" in _lib.lib.fm_last_error()
    nbytes = ctypes.c_int64(-5)
    assert _lib.knn_scratch_bytes(130, 10, 7, ctypes.byref(nbytes)) == 0 and nbytes.value == 130 * 10 * 7 * 8
    assert _lib.knn_scratch_bytes(130, 65, 1, ctypes.byref(nbytes)) == -1 and b"fm_knn_scratch_bytes" in _lib.lib.fm_last_error()
    assert _lib.knn_scratch_bytes(130, 64, 65, ctypes.byref(nbytes)) == -1 and nbytes.value == 130 * 10 * 7 * 8
    assert _lib.row_sqnorms(None, 1, 4, None, None) == -1 and b"fm_row_sqnorms" in _lib.lib.fm_last_error()
    assert _lib.knn_search(None, 1, None, None, 1, 4, 1, 1, 1, 0, None, 0, None, None, None) == -1 and b"fm_knn_search" in _lib.lib.fm_last_error()
    assert _lib.knn_refine_l2(None, 1, None, 1, 4, 1, None, None, None) == -1 and b"fm_knn_refine_l2" in _lib.lib.fm_last_error()


def test_python_refusals_fire_before_a_device_is_touched():
    from fourm.hip import _lib
    from fourm.utils.retrieval import MAX_K, FlatIndex, RetrievalSet, global_embeddings
    before = _lib.lib.fm_last_error()
    with pytest.raises(ValueError, match="unknown metric"):
        FlatIndex(8, "manhattan")
    with pytest.raises(ValueError, match="d="):
        FlatIndex(0)
    with pytest.raises(ValueError, match="d="):
        FlatIndex(4097)
    for device in ("cpu", None):                                               # None: the GPU - still nothing is touched by a refusal
        ix = FlatIndex(8, "l2", device)
        with pytest.raises(ValueError, match=r"\(m, 8\)"):
            ix.add(torch.zeros(3, 7))
        with pytest.raises(ValueError, match=r"\(m, 8\)"):
            ix.add(np.zeros(8, dtype=np.float32))
        with pytest.raises(ValueError, match="floating"):
            ix.add(torch.zeros(3, 8, dtype=torch.int64))
        with pytest.raises(ValueError, match="floating"):
            ix.add(np.zeros((3, 8), dtype=np.int32))
        with pytest.raises(ValueError, match=r"\(m, 8\)"):
            ix.search(torch.zeros(3, 9), 1)
        with pytest.raises(ValueError, match="floating"):
            ix.search(torch.zeros(3, 8, dtype=torch.int32), 1)
        with pytest.raises(ValueError, match=">= 1"):
            ix.search(torch.zeros(3, 8), 0)
        with pytest.raises(ValueError, match=f"FM_KNN_MAX_K = {MAX_K}"):
            ix.search(torch.zeros(3, 8), MAX_K + 1)
        assert ix.ntotal == 0
    with pytest.raises(ValueError, match="unknown metric"):
        RetrievalSet(metric="dot")
    with pytest.raises(ValueError, match="without a tokenizer"):
        RetrievalSet().add_tokens(torch.zeros(2, 4, dtype=torch.int64))
    with pytest.raises(ValueError, match="integer token tensor"):
        global_embeddings(torch.zeros(2, 4), None)
    with pytest.raises(ValueError, match=r"\(B, n\)"):
        global_embeddings(torch.zeros(2, 4, 2, dtype=torch.int64), None)

    class FakeTokenizer:
        class quantize:
            heads = 4

    with pytest.raises(ValueError, match="4 heads"):
        global_embeddings(torch.zeros(2, 5, dtype=torch.int64), FakeTokenizer())
    with pytest.raises(ValueError, match="4 heads"):
        global_embeddings({"tensor": torch.zeros(2, 16, 1, 1, dtype=torch.int64)}, FakeTokenizer())
    assert _lib.lib.fm_last_error() == before


def test_cpu_index_has_no_cpu_path():
    from fourm.utils.retrieval import FlatIndex, RetrievalSet
    ix = FlatIndex(8, "ip", "cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        ix.add(torch.zeros(3, 8))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ix.search(np.zeros((1, 8), dtype=np.float32), 1)
    rs = RetrievalSet.from_tensors(torch.randn(5, 8), device="cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        rs.query_embeddings(torch.zeros(1, 8), 1)


def test_retrieval_set_round_trips_host_tensors(tmp_path):
    from fourm.utils.retrieval import RetrievalSet
    g = torch.Generator().manual_seed(0)
    emb = torch.randn(10, 24, generator=g)
    payload = {"tok_depth": torch.randint(0, 100, (10, 6), generator=g), "id": torch.arange(10)}
    rs = RetrievalSet(metric="cosine")
    rs.add_embeddings(emb[:4], {k: v[:4] for k, v in payload.items()})
    rs.add_embeddings(emb[4:].numpy(), {k: v[4:] for k, v in payload.items()})
    assert len(rs) == 10 and torch.equal(rs.embeddings, emb) and all(torch.equal(rs.payload[k], payload[k]) for k in payload)
    path = str(tmp_path / "set.pth")
    rs.save(path)
    blob = torch.load(path)
    assert sorted(blob) == ["embeddings", "metric", "payload"] and torch.equal(blob["embeddings"], emb)      # plain tensors
    back = RetrievalSet.load(path)
    assert back.metric == "cosine" and len(back) == 10 and torch.equal(back.embeddings, emb)
    assert all(torch.equal(back.payload[k], payload[k]) for k in payload)
    plain = RetrievalSet.from_tensors(emb, payload["tok_depth"])                   # upstream's pair of files: embeddings and tokens
    assert plain.metric == "l2" and torch.equal(plain.payload, payload["tok_depth"]) and RetrievalSet.from_tensors(emb).payload is None
    with pytest.raises(ValueError, match="payload rows"):
        RetrievalSet.from_tensors(emb, payload["id"][:9])
    with pytest.raises(ValueError, match="width"):
        plain.add_embeddings(torch.zeros(2, 23), torch.zeros(2, 6))
    with pytest.raises(ValueError, match="every item has a payload"):
        plain.add_embeddings(torch.zeros(2, 24))


def test_reference_on_a_hand_worked_case_with_a_tie():
    """q = (1, 0) against (0, 0), (1, 0), (0, 1), (1, 0): squared distances 1, 0, 2, 0 and products 0, 1, 0, 1.  Rows 1 and 3 tie; the lower
    index comes first under both metrics, and rows 0 and 2 tie under ip."""
    X = np.array([[0, 0], [1, 0], [0, 1], [1, 0]], dtype=np.float32)
    Q = np.array([[1, 0]], dtype=np.float32)
    D, I = R.brute_force(Q, X, 3, "l2")
    assert I.tolist() == [[1, 3, 0]] and D.tolist() == [[0.0, 0.0, 1.0]]
    D, I = R.brute_force(Q, X, 4, "ip")
    assert I.tolist() == [[1, 3, 0, 2]] and D.tolist() == [[1.0, 1.0, 0.0, 0.0]]
    D, I = R.brute_force(Q, X, 6, "l2")                                        # k > n: faiss's padding
    assert I.tolist() == [[1, 3, 0, 2, -1, -1]] and D.tolist() == [[0.0, 0.0, 1.0, 2.0, np.inf, np.inf]]
    D, I = R.brute_force(Q, X, 5, "ip")
    assert I.tolist() == [[1, 3, 0, 2, -1]] and D[0, 4] == -np.inf


def test_integer_cases_are_exact_in_fp32_and_carry_ties_at_the_boundaries():
    for nq, n, d, k in R.INTEGER_CASES:
        Q, X = R.integer_case(nq, n, d, k)
        assert Q.shape == (nq, d) and X.shape == (n, d) and d <= 1024 and np.abs(X).max() <= 3 and np.abs(Q).max() <= 3
        assert 36 * d < 2 ** 24                                               # every sum the search forms is an exact fp32 integer
        if n >= 300:
            D, I = R.brute_force(Q[:1], X, min(k, n), "l2")
            assert (D[0] == 0).sum() >= min(k, 5)                              # the first query's neighbours tie at distance 0
        if n > 8:
            for r in R.boundary_rows(n):                                       # every boundary row has a copy elsewhere
                assert (X == X[r]).all(1).sum() >= 2, (n, r)
    assert R.boundary_rows(4099) == [127, 128, 129, 639, 640, 1279, 1280, 1919, 1920, 2175, 2176, 2559, 2560, 3199, 3200, 3839, 3840]


@pytest.mark.parametrize("name,share", [("A", 0.908), ("B", 0.939)])
def test_recipes_leave_most_queries_decided_by_float64(name, share):
    """The band of the GPU test cannot hide a wrong kernel: for at least 85 % of the queries the gap between ranks k and k + 1 is above
    2 E_q, so the returned set is fixed by float64 alone (l2, the metric the shares were worked out for: 0.908 and 0.939)."""
    Q, X, k = R.recipe(name)
    val = R.scores64(Q, X, "l2")
    got = float(R.determined(val, k, R.band(Q, X, "l2"), "l2").mean())
    assert got >= 0.85, got
    assert abs(got - share) < 0.0051, got
