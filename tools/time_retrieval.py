#!/usr/bin/env python3
"""Time of the flat k-NN search (``fourm.utils.retrieval.FlatIndex``, metric l2, random fp32 rows) on one MI355X against the same search in
eager torch on the same device (``|x|^2 - 2 q X^T`` as one matmul, then ``torch.topk``), at three shapes (nq, n, d, k): one query over a
million rows, a batch over 10^5 rows, and many queries over a small gallery.

One process, one run: per shape a warm-up, then --runs searches between device events; the median is reported with the minimum and the
maximum.  From shapes: gallery bytes / time as a fraction of 6.3 TB/s and 2 nq n d / time in TFLOP/s (the fp32-MFMA peak is 157).  ``search``
is the whole call (query preparation, the chunk search, the merge, the l2 refinement); ``kernels`` the chunk search and the merge alone.
torch's peak extra memory is what its (nq, n) score matrix costs.  Nothing is asserted and no speed is required; without a GPU it fails.

    python tools/time_retrieval.py [--runs 30] [--out profiles/retrieval_bench.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ml-4m_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

SHAPES = [(1, 1_000_000, 768, 5), (256, 100_000, 768, 10), (4096, 10_000, 768, 10)]
HBM_BYTES_PER_S = 6.3e12


def timed(fn, runs, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(runs + 1)]
    ev[0].record()
    for i in range(runs):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    ms = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(runs))
    return ms[len(ms) // 2], ms[0], ms[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.runs < 20:
        raise SystemExit("time_retrieval: at least 20 runs per shape")
    if not torch.cuda.is_available():
        raise SystemExit("time_retrieval needs an MI355X: a timing taken elsewhere says nothing")
    from fourm.hip import _lib as L
    from fourm.utils.retrieval import FlatIndex, knn_search
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    res = dict(metric="l2", runs=a.runs, compute_units=cus, shapes=[])
    for nq, n, d, k in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(nq)
        X = torch.randn(n, d, device="cuda", generator=g)
        Q = torch.randn(nq, d, device="cuda", generator=g)
        ix = FlatIndex(d, "l2")
        ix.add(X)
        x, xn = ix._store[:n], ix._norms[:n]
        med, lo, hi = timed(lambda: ix.search(Q, k), a.runs)
        kmed, klo, khi = timed(lambda: knn_search(Q, x, xn, k, "l2"), a.runs)

        def eager():
            return torch.topk(torch.addmm(xn[None, :].expand(nq, n), Q, X.t(), alpha=-2.0), k, dim=1, largest=False)

        tmed, tlo, thi = timed(eager, a.runs)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = eager()
        torch.cuda.synchronize()
        extra = torch.cuda.max_memory_allocated() - base
        I = ix.search(Q, k)[1]
        agree = float((I == out[1]).float().mean())
        del out
        gbytes, flops = n * d * 4, 2.0 * nq * n * d
        res["shapes"].append(dict(
            nq=nq, n=n, d=d, k=k, splits=L.knn_splits(nq, n, k, cus), query_tile=L.knn_query_tile(nq),
            search_ms=round(med, 4), search_ms_min_max=[round(lo, 4), round(hi, 4)],
            kernels_ms=round(kmed, 4), kernels_ms_min_max=[round(klo, 4), round(khi, 4)],
            gallery_bytes=gbytes, gallery_bandwidth_fraction=round(gbytes / (kmed * 1e-3) / HBM_BYTES_PER_S, 4),
            tflops=round(flops / (kmed * 1e-3) / 1e12, 3),
            torch_ms=round(tmed, 4), torch_ms_min_max=[round(tlo, 4), round(thi, 4)], torch_extra_bytes=int(extra),
            torch_over_search=round(tmed / med, 3), indices_equal_to_torch=round(agree, 5)))
        del ix, X, Q, x, xn
        torch.cuda.empty_cache()
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
