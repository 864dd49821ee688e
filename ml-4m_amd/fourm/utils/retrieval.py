"""Any-to-any retrieval (upstream: notebooks/retrieval_4M-21.ipynb): an exact k-nearest-neighbour index over global embeddings on the HIP
engine, in place of ``faiss.IndexFlatL2`` / ``IndexFlatIP``.

4M-21 predicts the ``tok_dinov2_global`` / ``tok_imagebind_global`` tokens from any conditioning, the MLP + Memcodes detokenizer turns them
into one embedding per sample (:func:`global_embeddings`), and the nearest neighbours of that embedding in a gallery are the retrieved items
(:class:`FlatIndex`, :class:`RetrievalSet`).

The search is DEFINED here, not by faiss ("Retrieval"; include/fourm_hip.h, "Flat k-NN index"): fp32 inner products with one
accumulation chain per (query, gallery row); ``ip`` ranks by the product, ``l2`` selects by ``|x|^2 - 2 <q, x>`` and reports the directly
summed ``sum (q - x)^2`` of the winners; a total order on (key, index) with the lowest index first on ties, so the result does not depend on
how the gallery is split or batched.  There is no CPU path."""
import ctypes as C

import numpy as np
import torch

__all__ = ["FlatIndex", "IndexFlatL2", "IndexFlatIP", "RetrievalSet", "global_embeddings", "knn_search", "knn_refine_l2", "row_sqnorms",
           "MAX_K", "chunk_rows"]

MAX_K = 64                      # FM_KNN_MAX_K
MAX_D = 4096                    # FM_KNN_MAX_D
_SCRATCH_CAP = 256 << 20        # bytes of candidate scratch per search launch; more queries are walked in blocks
_QUERY_BLOCK = 32768
_METRICS = ("l2", "ip", "cosine")


def _lib():
    from ..hip import _lib as L
    return L


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def chunk_rows(n: int, splits: int) -> int:
    """Gallery rows per chunk of a search over ``n`` rows in ``splits`` chunks: whole tiles of 128 rows (chunk c starts at c * chunk_rows)."""
    tiles = (n + 127) // 128
    return 128 * ((tiles + splits - 1) // splits)


# ---- the C entry points on tensors ----------------------------------------------------------------------------------------------------
def row_sqnorms(x, out=None):
    """|x_r|^2 (n,) f32 of contiguous f32 rows (n, d), d % 4 == 0 - fm_row_sqnorms."""
    L = _lib()
    n, d = x.shape
    assert x.dtype == torch.float32 and x.is_contiguous()
    out = torch.empty(n, dtype=torch.float32, device=x.device) if out is None else out
    assert out.dtype == torch.float32 and out.numel() == n and out.is_contiguous()
    L.check(L.row_sqnorms(_p(x), n, d, _p(out), _stream()))
    return out


def knn_search(q, x, xnorm, k, metric, splits=None, query_tile=0):
    """The keys (nq, k) f32 and indices (nq, k) int64 of the k best gallery rows per query - fm_knn_search.  q (nq, d), x (n, d) contiguous
    f32 on one GPU, d % 4 == 0; xnorm (n,) for ``l2``.  ``splits`` None: by nq, n, k and the CU count; ``query_tile`` 0: by nq."""
    L = _lib()
    nq, d = q.shape
    n = x.shape[0]
    assert q.dtype == x.dtype == torch.float32 and q.is_contiguous() and x.is_contiguous() and x.shape[1] == d and q.device == x.device
    code = {"ip": L.KNN_IP, "l2": L.KNN_L2}[metric]
    if splits is None:
        splits = L.knn_splits(nq, n, k, torch.cuda.get_device_properties(q.device).multi_processor_count)
        L.check(min(splits, 0))
    nbytes = C.c_int64(0)
    L.check(L.knn_scratch_bytes(nq, k, splits, C.byref(nbytes)))
    scratch = torch.empty(nbytes.value // 8, dtype=torch.int64, device=q.device)
    D = torch.empty(nq, k, dtype=torch.float32, device=q.device)
    I = torch.empty(nq, k, dtype=torch.int64, device=q.device)
    with torch.cuda.device(q.device):
        L.check(L.knn_search(_p(q), nq, _p(x), _p(xnorm), n, d, k, code, splits, query_tile, _p(scratch), nbytes.value, _p(D), _p(I), _stream()))
    return D, I


def knn_refine_l2(q, x, D, I):
    """In place: D = sum (q - x[I])^2 in fp32 and the k entries of every query re-ordered by (D, I) - fm_knn_refine_l2."""
    L = _lib()
    nq, d = q.shape
    assert D.shape == I.shape and D.shape[0] == nq and D.is_contiguous() and I.is_contiguous() and D.dtype == torch.float32 and I.dtype == torch.int64
    with torch.cuda.device(q.device):
        L.check(L.knn_refine_l2(_p(q), nq, _p(x), x.shape[0], d, D.shape[1], _p(D), _p(I), _stream()))
    return D, I


# ---- the index ------------------------------------------------------------------------------------------------------------------------
def _as_rows(a, d, what):
    """(tensor (m, d) as given, was_numpy) after the refusals that need no device."""
    was_numpy = isinstance(a, np.ndarray)
    if was_numpy:
        if not np.issubdtype(a.dtype, np.floating):
            raise ValueError(f"{what}: a floating-point array is expected, got {a.dtype}")
        a = torch.from_numpy(np.ascontiguousarray(a))
    elif not isinstance(a, torch.Tensor):
        raise ValueError(f"{what}: a torch tensor or a numpy array is expected, got {type(a).__name__}")
    elif not a.dtype.is_floating_point:
        raise ValueError(f"{what}: a floating-point tensor is expected, got {a.dtype}")
    if a.dim() != 2 or a.shape[1] != d:
        raise ValueError(f"{what}: shape (m, {d}) expected, got {tuple(a.shape)}")
    return a.detach(), was_numpy


class FlatIndex:
    """Exact nearest-neighbour index over fp32 rows of width ``d`` on one GPU, with faiss's ``add`` / ``search`` / ``reset`` / ``ntotal``.

    ``metric``: ``"l2"`` (squared Euclidean distance, ascending), ``"ip"`` (inner product, descending) or ``"cosine"`` (``ip`` on rows
    l2-normalised when they are added and when they are searched).  ``search`` returns ``(D, I)``: fp32 ``(nq, k)`` and int64 ``(nq, k)``,
    torch tensors on the index's device for torch queries and numpy arrays for numpy queries; with fewer than ``k`` rows the missing slots
    are ``I = -1`` and ``D = +inf`` (``l2``) / ``-inf``.  Rows are kept zero-padded to a multiple of 4 columns in one buffer that doubles."""

    def __init__(self, d, metric="l2", device=None):
        if metric not in _METRICS:
            raise ValueError(f"FlatIndex: unknown metric {metric!r} (one of {', '.join(_METRICS)})")
        if not isinstance(d, int) or d < 1 or d > MAX_D:
            raise ValueError(f"FlatIndex: d={d!r} unsupported (an integer in [1, {MAX_D}])")
        self.d, self.metric, self.ntotal = d, metric, 0
        self._dp = (d + 3) // 4 * 4
        self._device = torch.device("cuda" if device is None else device)
        self._store = self._norms = None

    # -- storage --
    @property
    def device(self):
        return self._device

    @property
    def vectors(self):
        """The stored rows, a (ntotal, d) view (normalised rows for ``cosine``)."""
        if self._store is None:
            return torch.empty(0, self.d, dtype=torch.float32, device=self._device)
        return self._store[:self.ntotal, :self.d]

    def _need_gpu(self, what):
        if self._device.type != "cuda":
            raise RuntimeError(f"FlatIndex.{what}: the index is on {self._device}; the search runs on the GPU only (no CPU path) - FlatIndex(d, device='cuda') or .to('cuda')")
        if not torch.cuda.is_available():
            raise RuntimeError(f"FlatIndex.{what}: no GPU is available; the search runs on the GPU only (no CPU path)")
        if self._device.index is None:
            self._device = torch.device("cuda", torch.cuda.current_device())

    def _reserve(self, rows):
        cap = 0 if self._store is None else self._store.shape[0]
        if rows <= cap:
            return
        cap = max(rows, 2 * cap)
        store = torch.zeros(cap, self._dp, dtype=torch.float32, device=self._device)
        norms = torch.zeros(cap, dtype=torch.float32, device=self._device)
        if self.ntotal:
            store[:self.ntotal].copy_(self._store[:self.ntotal])
            norms[:self.ntotal].copy_(self._norms[:self.ntotal])
        self._store, self._norms = store, norms

    def _prepare(self, a):
        """fp32 rows on the device, zero-padded to the stored width (normalised for ``cosine``): always a buffer of this call's own."""
        from ..hip import ops
        m = a.shape[0]
        rows = torch.zeros(m, self._dp, dtype=torch.float32, device=self._device) if self._dp != self.d else \
            torch.empty(m, self._dp, dtype=torch.float32, device=self._device)
        rows[:, :self.d].copy_(a)
        if self.metric == "cosine":
            ops.l2_normalize_rows(rows)
        return rows

    def add(self, x):
        x, _ = _as_rows(x, self.d, "FlatIndex.add")
        m = x.shape[0]
        if self.ntotal + m > 2 ** 31 - 1:
            raise ValueError(f"FlatIndex.add: {self.ntotal + m} rows exceed the limit of 2^31 - 1")
        self._need_gpu("add")
        if m == 0:
            return
        with torch.cuda.device(self._device):
            self._reserve(self.ntotal + m)
            dst = self._store[self.ntotal:self.ntotal + m]
            if self.metric == "cosine":
                dst.copy_(self._prepare(x))
            else:
                dst[:, :self.d].copy_(x)
            if self.metric == "l2":
                row_sqnorms(dst, self._norms[self.ntotal:self.ntotal + m])
        self.ntotal += m

    def reset(self):
        self.ntotal = 0
        self._store = self._norms = None

    def to(self, device):
        device = torch.device(device)
        if self._store is not None:
            self._store, self._norms = self._store.to(device), self._norms.to(device)
        self._device = device
        return self

    # -- search --
    def search(self, q, k, splits=None, query_tile=0):
        q, was_numpy = _as_rows(q, self.d, "FlatIndex.search")
        if not isinstance(k, int) or isinstance(k, bool) or k < 1:
            raise ValueError(f"FlatIndex.search: k={k!r}: an integer >= 1 is expected")
        if k > MAX_K:
            raise ValueError(f"FlatIndex.search: k={k} exceeds FM_KNN_MAX_K = {MAX_K}")
        self._need_gpu("search")
        nq, l2 = q.shape[0], self.metric == "l2"
        with torch.cuda.device(self._device):
            if nq == 0 or self.ntotal == 0:
                D = torch.full((nq, k), float("inf") if l2 else float("-inf"), dtype=torch.float32, device=self._device)
                I = torch.full((nq, k), -1, dtype=torch.int64, device=self._device)
            else:
                rows = self._prepare(q)
                x = self._store[:self.ntotal]
                xn = self._norms[:self.ntotal] if l2 else None
                out = []
                for b in range(0, nq, _QUERY_BLOCK):
                    qb = rows[b:b + _QUERY_BLOCK]
                    D, I = knn_search(qb, x, xn, k, "l2" if l2 else "ip", splits, query_tile)
                    if l2:
                        knn_refine_l2(qb, x, D, I)
                    out.append((D, I))
                D, I = out[0] if len(out) == 1 else (torch.cat([o[0] for o in out]), torch.cat([o[1] for o in out]))
        if was_numpy:
            return D.cpu().numpy(), I.cpu().numpy()
        return D, I


def IndexFlatL2(d, device=None):
    """``faiss.IndexFlatL2(d)``: squared Euclidean distances, ascending."""
    return FlatIndex(d, "l2", device)


def IndexFlatIP(d, device=None):
    """``faiss.IndexFlatIP(d)``: inner products, descending."""
    return FlatIndex(d, "ip", device)


# ---- global tokens -> embeddings ------------------------------------------------------------------------------------------------------
def global_embeddings(tokens, tokenizer):
    """The global embedding (B, C) f32 of every sample's global tokens: upstream's ``decode_tok_dinov2_global`` /
    ``decode_tok_imagebind_global`` (fourm/utils/plotting_utils.py:327-355) without the ``.squeeze()`` that loses the batch axis at B = 1.

    ``tokens``: an integer tensor (B, n) or (B, n, 1, 1), or a generation ``out_dict[key]`` (a dict with a ``'tensor'`` entry); ``n`` is the
    tokenizer's number of heads (codebooks)."""
    if isinstance(tokens, dict):
        tokens = tokens["tensor"]
    if not isinstance(tokens, torch.Tensor) or tokens.dtype.is_floating_point or tokens.dtype == torch.bool:
        raise ValueError("global_embeddings: an integer token tensor (B, n) or (B, n, 1, 1) is expected")
    if tokens.dim() == 4 and tokens.shape[2:] == (1, 1):
        tokens = tokens.reshape(tokens.shape[0], tokens.shape[1])
    if tokens.dim() != 2:
        raise ValueError(f"global_embeddings: tokens of shape (B, n) or (B, n, 1, 1) expected, got {tuple(tokens.shape)}")
    heads = getattr(getattr(tokenizer, "quantize", None), "heads", None)
    B, n = tokens.shape
    if heads is not None and n != heads:
        raise ValueError(f"global_embeddings: {n} tokens per sample, the tokenizer has {heads} heads")
    device = next(tokenizer.parameters()).device
    rec = tokenizer.decode_tokens(tokens.long().reshape(B, n, 1, 1).to(device))
    return rec.reshape(B, -1).float()


# ---- a gallery with what it retrieves -------------------------------------------------------------------------------------------------
def _payload_rows(payload):
    if isinstance(payload, dict):
        sizes = {k: _payload_rows(v) for k, v in payload.items()}
        if len(set(sizes.values())) != 1:
            raise ValueError(f"RetrievalSet: the payload entries have different numbers of rows: {sizes}")
        return next(iter(sizes.values()))
    if not isinstance(payload, torch.Tensor) or payload.dim() < 1:
        raise ValueError("RetrievalSet: a payload is a tensor with one row per item, or a dict of such tensors")
    return payload.shape[0]


def _payload_host(payload):
    return {k: _payload_host(v) for k, v in payload.items()} if isinstance(payload, dict) else payload.detach().cpu()


def _payload_cat(chunks):
    if isinstance(chunks[0], dict):
        return {k: _payload_cat([c[k] for c in chunks]) for k in chunks[0]}
    return chunks[0] if len(chunks) == 1 else torch.cat(chunks)


def _payload_take(payload, I):
    if isinstance(payload, dict):
        return {k: _payload_take(v, I) for k, v in payload.items()}
    return payload[I.clamp_min(0)]


class RetrievalSet:
    """A gallery of global embeddings and, row-aligned on the host, what each item retrieves (``payload``: a tensor with one row per item or
    a dict of such tensors - the item's ``tok_depth`` tokens, its RGB tokens, ...).

    Embeddings are kept on the host (``save`` / ``load`` / ``from_tensors`` need no GPU); the :class:`FlatIndex` is built on the first
    query.  Queries return ``(D, I, payload rows)``: the payload indexed by ``I`` (``None`` without a payload; a missing neighbour,
    ``I = -1``, shows item 0's payload - check ``I``)."""

    def __init__(self, tokenizer=None, metric="l2", device=None):
        if metric not in _METRICS:
            raise ValueError(f"RetrievalSet: unknown metric {metric!r} (one of {', '.join(_METRICS)})")
        self.tokenizer, self.metric, self._device = tokenizer, metric, device
        self._emb, self._payload, self._index, self._indexed = [], [], None, 0

    def __len__(self):
        return sum(e.shape[0] for e in self._emb)

    @property
    def embeddings(self):
        if not self._emb:
            return torch.empty(0, 0)
        if len(self._emb) > 1:
            self._emb = [torch.cat(self._emb)]
        return self._emb[0]

    @property
    def payload(self):
        if not self._payload:
            return None
        if len(self._payload) > 1:
            self._payload = [_payload_cat(self._payload)]
        return self._payload[0]

    # -- filling --
    def add_embeddings(self, emb, payload=None):
        if isinstance(emb, np.ndarray):
            emb = torch.from_numpy(emb)
        if not isinstance(emb, torch.Tensor) or emb.dim() != 2 or not emb.dtype.is_floating_point:
            raise ValueError("RetrievalSet.add_embeddings: a floating-point (m, d) tensor is expected")
        if self._emb and emb.shape[1] != self._emb[0].shape[1]:
            raise ValueError(f"RetrievalSet.add_embeddings: width {emb.shape[1]}, the set holds width {self._emb[0].shape[1]}")
        if (payload is None) != (not self._payload) and len(self):
            raise ValueError("RetrievalSet.add_embeddings: either every item has a payload or none has")
        if payload is not None and _payload_rows(payload) != emb.shape[0]:
            raise ValueError(f"RetrievalSet.add_embeddings: {emb.shape[0]} embeddings with {_payload_rows(payload)} payload rows")
        if emb.shape[0] == 0:
            return
        self._emb.append(emb.detach().float().cpu())
        if payload is not None:
            self._payload.append(_payload_host(payload))

    def add_tokens(self, tokens, payload=None):
        self.add_embeddings(global_embeddings(tokens, self._need_tokenizer("add_tokens")), payload)

    def _need_tokenizer(self, what):
        if self.tokenizer is None:
            raise ValueError(f"RetrievalSet.{what}: the set was built without a tokenizer; pass embeddings, or RetrievalSet(tokenizer=...)")
        return self.tokenizer

    # -- queries --
    @property
    def index(self):
        """The FlatIndex over the embeddings added so far (built, and extended, on demand)."""
        n = len(self)
        if n == 0:
            raise ValueError("RetrievalSet: the set is empty")
        emb = self.embeddings
        if self._index is None:
            self._index, self._indexed = FlatIndex(emb.shape[1], self.metric, self._device), 0
        if self._indexed < n:
            self._index.add(emb[self._indexed:n])
            self._indexed = n
        return self._index

    def query_embeddings(self, emb, k):
        D, I = self.index.search(emb, k)
        payload = self.payload
        rows = None if payload is None else _payload_take(payload, torch.as_tensor(I).cpu())
        return D, I, rows

    def query_tokens(self, tokens, k):
        return self.query_embeddings(global_embeddings(tokens, self._need_tokenizer("query_tokens")), k)

    def query(self, out_dict, key, k):
        """The neighbours of a generation's global tokens: ``out_dict[key]`` as the sampler returns it."""
        if key not in out_dict:
            raise ValueError(f"RetrievalSet.query: {key!r} is not in the dict (it has {sorted(out_dict)})")
        return self.query_tokens(out_dict[key], k)

    # -- files --
    def save(self, path):
        torch.save({"embeddings": self.embeddings, "payload": self.payload, "metric": self.metric}, path)

    @classmethod
    def load(cls, path, tokenizer=None, device=None):
        blob = torch.load(path, map_location="cpu")
        return cls.from_tensors(blob["embeddings"], blob.get("payload"), tokenizer=tokenizer, metric=blob.get("metric", "l2"), device=device)

    @classmethod
    def from_tensors(cls, embeddings, payload=None, tokenizer=None, metric="l2", device=None):
        """A set from an (N, d) embedding tensor and its row-aligned payload (tensors such as upstream's ``retrieval_set_*_10k.pth`` and
        ``*_tokens_10k.pth`` hold)."""
        out = cls(tokenizer, metric, device)
        out.add_embeddings(embeddings, payload)
        return out
