"""What the retrieval tests share: a float64 brute-force k-NN reference (a stable sort on (distance, index): the lowest index first on equal
distances) and the seeded input recipes - integer galleries with planted duplicate rows, and the two real-valued recipes with the error
bands of the fp32 search."""
import numpy as np

U = 2.0 ** -24

# (nq, n, d, k) of the integer cases: a single row; one row short of a tile and k = 1; a tile and a row, d = 20 (the columns 20..23 of the
# padded width are live); k at its maximum over a few tiles; several query tiles, 33 gallery tiles, d = 768; two skinny query tiles at
# d = 1024, k = 64; and k > n
INTEGER_CASES = [(1, 1, 4, 1), (3, 127, 36, 1), (5, 129, 20, 7), (2, 300, 8, 64), (130, 4099, 768, 10), (33, 1000, 1024, 64), (2, 5, 8, 7)]
FORCED_SPLITS = (1, 2, 7)


def chunk_rows(n, splits):
    """Rows per chunk of the search: ceil(ceil(n / 128) / splits) tiles of 128 (include/fourm_hip.h, "Flat k-NN index")."""
    tiles = (n + 127) // 128
    return 128 * ((tiles + splits - 1) // splits)


def brute_force(Q, X, k, metric):
    """(D (nq, k) float64, I (nq, k) int64): the first k of a stable sort on (distance, index).  ``l2``: sum (q - x)^2 ascending; ``ip``:
    <q, x> descending.  Fewer than k rows: I = -1 and D = +inf (l2) / -inf (ip)."""
    Q, X = np.asarray(Q, dtype=np.float64), np.asarray(X, dtype=np.float64)
    nq, n = Q.shape[0], X.shape[0]
    if metric == "l2":
        val = key = _sqdist(Q, X)
    else:
        val = Q @ X.T
        key = -val
    order = np.argsort(key, axis=1, kind="stable")[:, :k]
    D = np.full((nq, k), np.inf if metric == "l2" else -np.inf)
    I = np.full((nq, k), -1, dtype=np.int64)
    m = min(k, n)
    I[:, :m] = order[:, :m]
    D[:, :m] = np.take_along_axis(val, order[:, :m], axis=1)
    return D, I


def _sqdist(Q, X):
    """sum (q - x)^2 in float64, summed directly (no cancellation), in row blocks."""
    out = np.empty((Q.shape[0], X.shape[0]))
    for i in range(Q.shape[0]):
        diff = X - Q[i][None, :]
        out[i] = np.einsum("nd,nd->n", diff, diff)
    return out


def boundary_rows(n):
    """Gallery positions on both sides of every chunk boundary of the forced splits, and of the first tile boundary."""
    rows = {127, 128, 129}
    for s in FORCED_SPLITS:
        per = chunk_rows(n, s)
        for c in range(1, s):
            rows.update((c * per - 1, c * per))
    return sorted(r for r in rows if 0 <= r < n)


def integer_case(nq, n, d, k, seed=0):
    """(Q (nq, d), X (n, d)) fp32 with integer entries in [-3, 3].  About 40 positions of the gallery (rows 127, 128, 129, both sides of every
    forced chunk boundary, and scattered ones) hold copies of a few source rows, and the first queries are those source rows: their nearest
    neighbours tie inside a tile, across tiles and across chunks."""
    rng = np.random.default_rng(1000 * seed + 7 * n + d)
    X = rng.integers(-3, 4, (n, d)).astype(np.float32)
    Q = rng.integers(-3, 4, (nq, d)).astype(np.float32)
    n_src = min(3, n)
    src = X[rng.choice(n, n_src, replace=False)].copy()
    spots = boundary_rows(n)
    if n > 8:
        spots = sorted(set(spots) | set(int(v) for v in rng.choice(n, min(40, n // 3), replace=False)))
    for t, r in enumerate(spots):
        X[r] = src[t % n_src]
    for i in range(min(nq, n_src)):
        Q[i] = src[i]
    return Q, X


def recipe(name):
    """(Q, X, k) of the two real-valued recipes, fp32."""
    if name == "A":
        rng = np.random.default_rng(0)
        X = rng.standard_normal((4099, 768))
        Q = rng.standard_normal((130, 768))
        return Q.astype(np.float32), X.astype(np.float32), 10
    if name == "B":
        rng = np.random.default_rng(3)
        X = rng.standard_normal((1000, 1024))
        idx = rng.integers(0, 1000, 33)
        Q = X[idx] + 0.05 * rng.standard_normal((33, 1024))
        return Q.astype(np.float32), X.astype(np.float32), 5
    raise KeyError(name)


def band(Q, X, metric):
    """E_q (nq,) of the fp32 selection key, from float64 norms: l2 (d + 2) u (|q| + max |x|)^2, ip (d + 1) u |q| max |x|."""
    Q, X = np.asarray(Q, dtype=np.float64), np.asarray(X, dtype=np.float64)
    d = Q.shape[1]
    qn, xm = np.sqrt((Q * Q).sum(1)), np.sqrt((X * X).sum(1)).max()
    return (d + 2) * U * (qn + xm) ** 2 if metric == "l2" else (d + 1) * U * qn * xm


def scores64(Q, X, metric):
    """(nq, n) float64: squared distances (l2, smaller is better) or inner products (ip, larger is better)."""
    Q, X = np.asarray(Q, dtype=np.float64), np.asarray(X, dtype=np.float64)
    return _sqdist(Q, X) if metric == "l2" else Q @ X.T


def determined(val, k, E, metric):
    """Per query: is the gap between ranks k and k + 1 above 2 E_q (the returned SET is then fixed by float64 alone)?"""
    srt = np.sort(val if metric == "l2" else -val, axis=1)
    return (srt[:, k] - srt[:, k - 1]) > 2.0 * E


def check_band(val, k, E, metric, D, I, Q, X):
    """The statements of the band test for one search result (numpy D (nq, k) f32, I (nq, k) int64); returns the worst ratios it saw."""
    nq, d = Q.shape
    key = val if metric == "l2" else -val
    T = np.sort(key, axis=1)[:, k - 1]
    assert I.min() >= 0 and I.max() < X.shape[0]
    got = np.take_along_axis(key, I, axis=1)
    assert np.all(got <= (T + E)[:, None]), "a returned row lies outside the band"
    for i in range(nq):
        must = np.nonzero(key[i] < T[i] - E[i])[0]
        assert np.isin(must, I[i]).all(), (i, "a row inside the band is missing")
        assert len(set(I[i].tolist())) == k
    Dk = D.astype(np.float64) if metric == "l2" else -D.astype(np.float64)
    assert np.all(np.diff(Dk, axis=1) >= 0), "D is not sorted"
    same = np.diff(Dk, axis=1) == 0
    assert np.all(np.diff(I, axis=1)[same] > 0), "equal values do not come in ascending index"
    ref = np.take_along_axis(val, I, axis=1)
    if metric == "l2":
        tol = (d + 3) * U * ref
    else:
        absdot = np.abs(np.asarray(Q, dtype=np.float64))[:, None, :] * np.abs(np.asarray(X, dtype=np.float64)[I])
        tol = (d + 1) * U * absdot.sum(-1)
    err = np.abs(D.astype(np.float64) - ref)
    assert np.all(err <= tol), (float((err / np.maximum(tol, 1e-300)).max()), "reported value outside its bound")
    return float((err / np.maximum(tol, 1e-300)).max())
