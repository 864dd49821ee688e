// Exact ("flat") k-nearest-neighbour search of fp32 query rows against an fp32 gallery (include/fourm_hip.h, "Flat k-NN index"): the last
// step of 4M-21's any-to-any retrieval, faiss.IndexFlatL2 / IndexFlatIP without the score matrix.
//   fm_row_sqnorms     |x_r|^2 per gallery row, once when rows are added.
//   fm_knn_search      top-k per (query, gallery chunk) with a running top-k in LDS, then one merge per query.
//   fm_knn_refine_l2   the true squared distances of the k winners and their final order.
// Scores are the tiled exact-fp32 product of vq_search_wide_kernel (csrc/vq.hip) on v_mfma_f32_32x32x2_f32: one accumulation chain over d per
// score, so a score is a function of (query row, gallery row, d) alone - not of the tile, the chunk, the tile width or the batch.  A
// candidate is ONE 64-bit word, (order-preserving image of the key) << 32 | gallery index: an unsigned compare of two words is the total
// order "better key first, lower index first", and everything below (threshold test, compaction, merge) is that compare.  The first k of a
// total order do not depend on the order of arrival, so the result cannot depend on the gallery split.  No floating-point atomics; the only
// atomic is the integer LDS counter of the append buffer (it decides the slot of a candidate, never whether it is kept).
#include <math.h>

#include "common.h"
#include "fourm_hip.h"

namespace {

typedef unsigned long long u64;
constexpr int KNN_T = 128;             // gallery rows per tile
constexpr int KNN_KS = 32;             // columns of d per staging step
constexpr int KNN_LDT = KNN_KS + 1;    // LDS row stride 33 floats: the 32 lanes of a half-wave hit 32 banks
constexpr int KNN_BUF = 32;            // append slots per query row: one phase of the epilogue offers at most 32 gallery rows
constexpr int KNN_INSERT_MAX = 4;      // up to this many appended candidates a thread inserts them; above, a wave ranks the row
constexpr u64 KNN_NONE = ~0ull;        // "no candidate": after every real one (their indices are below 2^31)

// float -> uint32 whose unsigned order is the float order (-inf lowest, +inf highest); -0 is folded onto +0 first so that equal keys have
// equal images
__device__ __forceinline__ uint32_t knn_ord(float v) {
    if (v == 0.f) v = 0.f;
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float knn_unord(uint32_t o) { return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o); }

// |x_r|^2: a wave per row, lane l adds elements 4 l .. 4 l + 3, 4 l + 256 .., in index order (fmaf), then the shuffle tree
__global__ __launch_bounds__(256) void knn_row_sqnorms_kernel(const float* __restrict__ x, int n, int D, float* __restrict__ out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long r = (long long)blockIdx.x * 4 + wave;
    if (r >= n) return;
    const float* xr = x + (size_t)r * D;
    float s = 0.f;
    for (int d = lane * 4; d < D; d += 256) {
        const float4 v = *(const float4*)(xr + d);
        s = fmaf(v.x, v.x, s); s = fmaf(v.y, v.y, s); s = fmaf(v.z, v.z, s); s = fmaf(v.w, v.w, s);
    }
    s = wave_sum(s);
    if (lane == 0) out[r] = s;
}

// The k best of the row's k kept candidates (sorted) and its c appended ones, by rank: entry e goes to slot #{entries before e}.  One wave,
// lanes own entries lane and lane + 64 (k + c <= 96).  Every lane has read the whole row before the first lane writes (one wave, in order).
__device__ __forceinline__ void knn_compact_row(u64* row, int k, int c, u64* thr) {
    const int lane = threadIdx.x & 63, m = k + c;
    const u64 e0 = lane < m ? row[lane] : KNN_NONE, e1 = lane + 64 < m ? row[lane + 64] : KNN_NONE;
    int r0 = 0, r1 = 0;
    for (int t = 0; t < m; ++t) {
        const u64 v = row[t];
        r0 += (v < e0 || (v == e0 && t < lane)) ? 1 : 0;              // equal words are "no candidate" twice: position breaks the tie
        r1 += (v < e1 || (v == e1 && t < lane + 64)) ? 1 : 0;
    }
    __builtin_amdgcn_wave_barrier();
    if (lane < m && r0 < k) row[r0] = e0;
    if (lane + 64 < m && r1 < k) row[r1] = e1;
    if (lane < m && r0 == k - 1) *thr = e0;
    if (lane + 64 < m && r1 == k - 1) *thr = e1;
}

// The same result for a few appended candidates, by one thread: each is inserted into the sorted kept ones (or dropped).
__device__ __forceinline__ void knn_insert_row(u64* row, int k, int c, u64* thr) {
    u64 last = row[k - 1];
    for (int a = 0; a < c; ++a) {
        const u64 w = row[k + a];
        if (w >= last) continue;
        int j = k - 1;
        for (; j > 0; --j) {
            const u64 v = row[j - 1];
            if (v <= w) break;
            row[j] = v;
        }
        row[j] = w;
        last = row[k - 1];
    }
    *thr = last;
}

// grid (splits, query tiles).  A workgroup owns QT query rows and the gallery tiles [chunk tiles_per_chunk, (chunk + 1) tiles_per_chunk).
// QT = 128: waves 2 x 2, each 64 gallery rows x 64 queries (the tile of vq_search_wide_kernel).  QT = 32: each wave 32 gallery rows x the 32
// queries - a quarter of the MFMA work per gallery byte, for searches with a few queries that are bound by the gallery read.  The product of
// a (query, gallery row) pair is the same instruction sequence in both.
template <int QT>
__global__ __launch_bounds__(256, 2) void knn_search_kernel(const float* __restrict__ q, int nq, const float* __restrict__ x, const float* __restrict__ xn,
                                                         int n, int D, int k, int metric, int tiles_per_chunk, u64* __restrict__ scratch) {
    constexpr int T = KNN_T, KS = KNN_KS, LDT = KNN_LDT, NI = QT == 128 ? 2 : 1, QP = QT / 32;
    __shared__ float Xs[T * LDT], Qs[QT * LDT];
    __shared__ float xns[T];
    __shared__ u64 thr[QT];
    __shared__ int cnt[QT];
    extern __shared__ __attribute__((aligned(16))) char smem[];
    u64* rows = (u64*)smem;                                            // QT x (k kept, sorted | KNN_BUF appended)
    const int stride = k + KNN_BUF;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int gbase = QT == 128 ? (wave >> 1) * 64 : wave * 32, qbase = QT == 128 ? (wave & 1) * 64 : 0;
    const int chunk = blockIdx.x, m0 = blockIdx.y * QT;
    for (int i = threadIdx.x; i < QT * stride; i += 256) rows[i] = KNN_NONE;
    if (threadIdx.x < QT) { thr[threadIdx.x] = KNN_NONE; cnt[threadIdx.x] = 0; }
    const int ntiles = (n + T - 1) / T;
    const long long tb = (long long)chunk * tiles_per_chunk;
    const int t_begin = tb < ntiles ? (int)tb : ntiles, t_end = tb + tiles_per_chunk < ntiles ? (int)(tb + tiles_per_chunk) : ntiles;
    const int lr = threadIdx.x >> 3, lc = (threadIdx.x & 7) * 4;       // staging: thread -> (row lr + 32 p, 4 floats at column lc)
    const float* qp[QP];
#pragma unroll
    for (int p = 0; p < QP; ++p) {
        const int r = m0 + lr + 32 * p;
        qp[p] = q + (size_t)(r < nq ? r : nq - 1) * D + lc;            // rows past the edge repeat the last one (never reported)
    }
    for (int tile = t_begin; tile < t_end; ++tile) {
        const int n0 = tile * T;                                       // < n <= 2^31 - 1
        const float* xp[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int r = lr + 32 * p;
            xp[p] = x + (size_t)(r < n - n0 ? n0 + r : n - 1) * D + lc;       // 64-bit element offset: a gallery passes 4 GiB
        }
        if (threadIdx.x < T) xns[threadIdx.x] = metric == FM_KNN_L2 ? xn[threadIdx.x < n - n0 ? n0 + threadIdx.x : n - 1] : 0.f;
        f32x16_t acc[NI][NI];
#pragma unroll
        for (int i = 0; i < NI; ++i)
#pragma unroll
            for (int j = 0; j < NI; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
        float4 xreg[4], qreg[QP];
        auto load = [&](int k0) {
            const bool in = k0 + lc < D;                               // D % 4 == 0: a float4 is inside or outside as a whole
#pragma unroll
            for (int p = 0; p < 4; ++p) xreg[p] = in ? *(const float4*)(xp[p] + k0) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int p = 0; p < QP; ++p) qreg[p] = in ? *(const float4*)(qp[p] + k0) : make_float4(0.f, 0.f, 0.f, 0.f);
        };
        auto stash = [&]() {
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                float* xd = Xs + (lr + 32 * p) * LDT + lc;
                xd[0] = xreg[p].x; xd[1] = xreg[p].y; xd[2] = xreg[p].z; xd[3] = xreg[p].w;
            }
#pragma unroll
            for (int p = 0; p < QP; ++p) {
                float* qd = Qs + (lr + 32 * p) * LDT + lc;
                qd[0] = qreg[p].x; qd[1] = qreg[p].y; qd[2] = qreg[p].z; qd[3] = qreg[p].w;
            }
        };
        load(0);
        for (int k0 = 0; k0 < D; k0 += KS) {
            __syncthreads();                                           // the previous step's readers (and the previous tile's epilogue) are done
            stash();
            __syncthreads();
            if (k0 + KS < D) load(k0 + KS);                            // next step in flight under the MFMAs
            const float* xb = Xs + (gbase + (lane & 31)) * LDT + (lane >> 5);
            const float* qb = Qs + (qbase + (lane & 31)) * LDT + (lane >> 5);
#pragma unroll
            for (int kk = 0; kk < KS; kk += 2) {
                if constexpr (NI == 2) {
                    const float a0 = xb[kk], a1 = xb[32 * LDT + kk], b0 = qb[kk], b1 = qb[32 * LDT + kk];
                    acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
                    acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
                    acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
                    acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
                } else {
                    acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(xb[kk], qb[kk], acc[0][0], 0, 0, 0);
                }
            }
        }
        // accumulator map: column (lane & 31) = query row, register 4 g + e = gallery row 8 g + 4 (lane >> 5) + e of the 32-row tile.
        // A lane first asks whether any of its candidates passes its row's threshold.
        const int fhi = lane >> 5;
        auto word = [&](float s, int t) -> u64 {                       // the candidate word of score s at tile row t
            const float key = metric == FM_KNN_L2 ? fmaf(-2.0f, s, xns[t]) : -s;
            return ((u64)knn_ord(key) << 32) | (uint32_t)(n0 + t);
        };
        bool any = false;
#pragma unroll
        for (int j = 0; j < NI; ++j) {
            const int qr = qbase + j * 32 + (lane & 31);
            const u64 th = m0 + qr < nq ? thr[qr] : 0;                 // a row past the edge takes no candidate (no word is below 0)
#pragma unroll
            for (int i = 0; i < NI; ++i)
#pragma unroll
                for (int g = 0; g < 4; ++g)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int t = gbase + i * 32 + 8 * g + 4 * fhi + e;
                        any |= t < n - n0 && word(acc[i][j][4 * g + e], t) < th;
                    }
        }
        if (!__syncthreads_or(any ? 1 : 0)) continue;                  // the common case once the thresholds have settled
        // Four phases of 32 gallery rows (ascending): the owners append what passes the threshold, then the appended candidates are folded
        // into the kept ones (by a thread per row, or a wave per row) and the threshold tightens.  A row receives at most 32 = KNN_BUF
        // candidates per phase.
        for (int ph = 0; ph < 4; ++ph) {
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                if ((QT == 128 ? (wave >> 1) * 2 + i : wave) != ph) continue;
#pragma unroll
                for (int j = 0; j < NI; ++j) {
                    const int qr = qbase + j * 32 + (lane & 31);
                    const u64 th = m0 + qr < nq ? thr[qr] : 0;
#pragma unroll
                    for (int g = 0; g < 4; ++g)
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const int t = gbase + i * 32 + 8 * g + 4 * fhi + e;
                            const u64 w = word(acc[i][j][4 * g + e], t);
                            if (t < n - n0 && w < th) {
                                const int slot = atomicAdd(&cnt[qr], 1);
                                if (slot < KNN_BUF) rows[qr * stride + k + slot] = w;
                            }
                        }
                }
            }
            __syncthreads();
            if (threadIdx.x < QT) {                                    // a few appended candidates (the usual case): a thread per row inserts them
                const int r = threadIdx.x, c = cnt[r];
                if (c > 0 && c <= KNN_INSERT_MAX) {
                    knn_insert_row(rows + r * stride, k, c, &thr[r]);
                    cnt[r] = 0;
                }
            }
            __syncthreads();
            for (int r = wave; r < QT; r += 4) {                       // many (the first tiles of a chunk): a wave per row ranks them
                const int c = cnt[r] < KNN_BUF ? cnt[r] : KNN_BUF;
                if (c > 0) {
                    knn_compact_row(rows + r * stride, k, c, &thr[r]);
                    if (lane == 0) cnt[r] = 0;
                }
            }
            __syncthreads();
        }
    }
    __syncthreads();
    const int S = gridDim.x;
    for (int i = threadIdx.x; i < QT * k; i += 256) {
        const int r = i / k, c = i - r * k;
        if (m0 + r < nq) scratch[((size_t)(m0 + r) * S + chunk) * k + c] = rows[r * stride + c];
    }
}

// The k best of a query's S k candidates: a bitonic sort of P = 2^p >= S k words in LDS, a workgroup per query.
__global__ __launch_bounds__(256) void knn_merge_kernel(const u64* __restrict__ scratch, int m, int k, int P, int metric, float* __restrict__ out_d,
                                                        long long* __restrict__ out_i) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    u64* a = (u64*)smem;
    const u64* src = scratch + (size_t)blockIdx.x * m;
    for (int i = threadIdx.x; i < P; i += 256) a[i] = i < m ? src[i] : KNN_NONE;
    for (int size = 2; size <= P; size <<= 1)
        for (int st = size >> 1; st > 0; st >>= 1) {
            __syncthreads();
            for (int t = threadIdx.x; t < P / 2; t += 256) {
                const int i = 2 * t - (t & (st - 1)), j = i + st;
                const u64 u = a[i], v = a[j];
                if ((u > v) == ((i & size) == 0)) { a[i] = v; a[j] = u; }
            }
        }
    __syncthreads();
    if (threadIdx.x < k) {
        const u64 w = a[threadIdx.x];
        const size_t o = (size_t)blockIdx.x * k + threadIdx.x;
        if ((uint32_t)w == 0xffffffffu) {                              // fewer than k gallery rows: faiss's padding
            out_i[o] = -1;
            out_d[o] = metric == FM_KNN_L2 ? INFINITY : -INFINITY;
        } else {
            const float key = knn_unord((uint32_t)(w >> 32));
            out_i[o] = (long long)(uint32_t)w;
            out_d[o] = metric == FM_KNN_L2 ? key : 0.f - key;
        }
    }
}

// delta = sum_i (q_i - x_i)^2 of a query's k winners (a wave per winner: lane l adds elements 4 l .., 4 l + 256 .. in index order, then the
// shuffle tree), then the k re-ordered by (delta, index) by rank.  An index outside [0, n) is padding: it stays -1 / +inf at the end.
__global__ __launch_bounds__(256) void knn_refine_l2_kernel(const float* __restrict__ q, const float* __restrict__ x, int n, int D, int k,
                                                            float* __restrict__ d_io, long long* __restrict__ i_io) {
    __shared__ float dv[FM_KNN_MAX_K];
    __shared__ long long iv[FM_KNN_MAX_K];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* qr = q + (size_t)blockIdx.x * D;
    const size_t o = (size_t)blockIdx.x * k;
    for (int c = wave; c < k; c += 4) {
        const long long idx = i_io[o + c];
        const bool ok = idx >= 0 && idx < n;
        float s = 0.f;
        if (ok) {
            const float* xr = x + (size_t)idx * D;
            for (int d = lane * 4; d < D; d += 256) {
                const float4 a = *(const float4*)(qr + d), b = *(const float4*)(xr + d);
                const float t0 = a.x - b.x, t1 = a.y - b.y, t2 = a.z - b.z, t3 = a.w - b.w;
                s = fmaf(t0, t0, s); s = fmaf(t1, t1, s); s = fmaf(t2, t2, s); s = fmaf(t3, t3, s);
            }
            s = wave_sum(s);
        }
        if (lane == 0) { dv[c] = ok ? s : INFINITY; iv[c] = ok ? idx : -1; }
    }
    __syncthreads();
    if (threadIdx.x < k) {
        const int c = threadIdx.x;
        const float dc = dv[c];
        const long long ic = iv[c];
        int rank = 0;
        for (int t = 0; t < k; ++t) {
            const float dt = dv[t];
            const long long it = iv[t];
            bool before;
            if (it < 0 || ic < 0) before = ic < 0 && (it >= 0 || t < c);      // padding goes last, in its own order
            else before = dt < dc || (dt == dc && (it < ic || (it == ic && t < c)));
            rank += before ? 1 : 0;
        }
        d_io[o + rank] = dc;
        i_io[o + rank] = ic;
    }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int fm_row_sqnorms(const void* x, int n, int d, void* out, void* stream) {
    FM_CHECK_ARG(x && out, "fm_row_sqnorms: null pointer");
    FM_CHECK_ARG(n > 0 && d > 0 && d % 4 == 0 && d <= FM_KNN_MAX_D, "fm_row_sqnorms: bad shape (n=%d d=%d: n > 0, d a multiple of 4 in [4, %d])", n, d, FM_KNN_MAX_D);
    FM_CHECK_ARG(aligned16(x) && ((uintptr_t)out & 3) == 0, "fm_row_sqnorms: x must be 16-byte aligned, out 4-byte aligned");
    hipLaunchKernelGGL(knn_row_sqnorms_kernel, dim3((unsigned)(((long long)n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (const float*)x, n, d, (float*)out);
    FM_CHECK_LAUNCH("fm_row_sqnorms");
    return 0;
}

extern "C" int fm_knn_query_tile(int nq) { return nq <= 0 ? -1 : nq <= 64 ? 32 : 128; }

extern "C" int fm_knn_splits(int nq, int n, int k, int cus) {
    FM_CHECK_ARG(nq > 0 && n > 0 && k >= 1 && k <= FM_KNN_MAX_K && cus > 0, "fm_knn_splits: bad argument (nq=%d n=%d k=%d cus=%d)", nq, n, k, cus);
    const int qt = fm_knn_query_tile(nq);
    const long long qtiles = ((long long)nq + qt - 1) / qt, ntiles = ((long long)n + KNN_T - 1) / KNN_T;
    const long long target = (long long)cus * (qt == 32 ? 4 : 2);      // workgroups that fit the chip at once at a small k
    long long S = (target + qtiles - 1) / qtiles;
    if (S > ntiles) S = ntiles;
    if (S > FM_KNN_MAX_MERGE / k) S = FM_KNN_MAX_MERGE / k;
    if (S < 1) S = 1;
    const long long per = (ntiles + S - 1) / S;
    return (int)((ntiles + per - 1) / per);                            // no empty chunk
}

extern "C" int fm_knn_scratch_bytes(int nq, int k, int splits, int64_t* bytes) {
    FM_CHECK_ARG(bytes, "fm_knn_scratch_bytes: null pointer");
    FM_CHECK_ARG(nq > 0 && k >= 1 && k <= FM_KNN_MAX_K && splits >= 1 && (long long)splits * k <= FM_KNN_MAX_MERGE,
                 "fm_knn_scratch_bytes: bad argument (nq=%d k=%d splits=%d: 1 <= k <= %d, splits k <= %d)", nq, k, splits, FM_KNN_MAX_K, FM_KNN_MAX_MERGE);
    *bytes = (int64_t)nq * splits * k * 8;
    return 0;
}

extern "C" int fm_knn_search(const void* q, int nq, const void* x, const void* xnorm, int n, int d, int k, int metric, int splits, int query_tile,
                             void* scratch, int64_t scratch_bytes, void* out_d, void* out_i, void* stream) {
    FM_CHECK_ARG(q && x && scratch && out_d && out_i, "fm_knn_search: null pointer");
    FM_CHECK_ARG(metric == FM_KNN_IP || metric == FM_KNN_L2, "fm_knn_search: unknown metric %d (FM_KNN_IP = 0, FM_KNN_L2 = 1)", metric);
    FM_CHECK_ARG(metric != FM_KNN_L2 || xnorm, "fm_knn_search: FM_KNN_L2 needs xnorm (fm_row_sqnorms)");
    FM_CHECK_ARG(nq > 0 && n > 0, "fm_knn_search: bad shape (nq=%d n=%d)", nq, n);
    FM_CHECK_ARG(d > 0 && d % 4 == 0 && d <= FM_KNN_MAX_D, "fm_knn_search: d=%d unsupported (a multiple of 4 in [4, %d])", d, FM_KNN_MAX_D);
    FM_CHECK_ARG(k >= 1 && k <= FM_KNN_MAX_K, "fm_knn_search: k=%d outside [1, FM_KNN_MAX_K = %d]", k, FM_KNN_MAX_K);
    FM_CHECK_ARG(splits >= 1 && (long long)splits * k <= FM_KNN_MAX_MERGE, "fm_knn_search: splits=%d unsupported (splits >= 1, splits k <= %d)", splits, FM_KNN_MAX_MERGE);
    FM_CHECK_ARG(query_tile == 0 || query_tile == 32 || query_tile == 128, "fm_knn_search: query_tile=%d (0 = by nq, 32 or 128)", query_tile);
    FM_CHECK_ARG(aligned16(q) && aligned16(x) && ((uintptr_t)xnorm & 3) == 0 && ((uintptr_t)scratch & 7) == 0 && ((uintptr_t)out_d & 3) == 0 && ((uintptr_t)out_i & 7) == 0,
                 "fm_knn_search: misaligned pointer (q, x 16 bytes; scratch, out_i 8; xnorm, out_d 4)");
    const int64_t need = (int64_t)nq * splits * k * 8;
    FM_CHECK_ARG(scratch_bytes >= need, "fm_knn_search: scratch_bytes=%lld, need %lld (fm_knn_scratch_bytes)", (long long)scratch_bytes, (long long)need);
    const int qt = query_tile ? query_tile : fm_knn_query_tile(nq);
    const long long qtiles = ((long long)nq + qt - 1) / qt;
    FM_CHECK_ARG(qtiles <= 65535, "fm_knn_search: nq=%d is more than 65535 query tiles of %d: search in blocks", nq, qt);
    const int ntiles = (int)(((long long)n + KNN_T - 1) / KNN_T), per = (ntiles + splits - 1) / splits;
    const size_t lds = (size_t)qt * (k + KNN_BUF) * 8;
    hipStream_t s = (hipStream_t)stream;
    if (qt == 32) {
        hipLaunchKernelGGL(knn_search_kernel<32>, dim3(splits, (unsigned)qtiles), dim3(256), lds, s, (const float*)q, nq, (const float*)x, (const float*)xnorm, n, d, k,
                           metric, per, (u64*)scratch);
    } else {
        static bool once = (hipFuncSetAttribute((const void*)knn_search_kernel<128>, hipFuncAttributeMaxDynamicSharedMemorySize, 128 * (FM_KNN_MAX_K + KNN_BUF) * 8), true);
        (void)once;
        hipLaunchKernelGGL(knn_search_kernel<128>, dim3(splits, (unsigned)qtiles), dim3(256), lds, s, (const float*)q, nq, (const float*)x, (const float*)xnorm, n, d, k,
                           metric, per, (u64*)scratch);
    }
    int P = 1;
    while (P < splits * k) P <<= 1;
    if (P < 2) P = 2;
    hipLaunchKernelGGL(knn_merge_kernel, dim3(nq), dim3(256), (size_t)P * 8, s, (const u64*)scratch, splits * k, k, P, metric, (float*)out_d, (long long*)out_i);
    FM_CHECK_LAUNCH("fm_knn_search");
    return 0;
}

extern "C" int fm_knn_refine_l2(const void* q, int nq, const void* x, int n, int d, int k, void* d_io, void* i_io, void* stream) {
    FM_CHECK_ARG(q && x && d_io && i_io, "fm_knn_refine_l2: null pointer");
    FM_CHECK_ARG(nq > 0 && n > 0, "fm_knn_refine_l2: bad shape (nq=%d n=%d)", nq, n);
    FM_CHECK_ARG(d > 0 && d % 4 == 0 && d <= FM_KNN_MAX_D, "fm_knn_refine_l2: d=%d unsupported (a multiple of 4 in [4, %d])", d, FM_KNN_MAX_D);
    FM_CHECK_ARG(k >= 1 && k <= FM_KNN_MAX_K, "fm_knn_refine_l2: k=%d outside [1, FM_KNN_MAX_K = %d]", k, FM_KNN_MAX_K);
    FM_CHECK_ARG(aligned16(q) && aligned16(x) && ((uintptr_t)d_io & 3) == 0 && ((uintptr_t)i_io & 7) == 0, "fm_knn_refine_l2: misaligned pointer (q, x 16 bytes; i_io 8; d_io 4)");
    hipLaunchKernelGGL(knn_refine_l2_kernel, dim3(nq), dim3(256), 0, (hipStream_t)stream, (const float*)q, (const float*)x, n, d, k, (float*)d_io, (long long*)i_io);
    FM_CHECK_LAUNCH("fm_knn_refine_l2");
    return 0;
}
