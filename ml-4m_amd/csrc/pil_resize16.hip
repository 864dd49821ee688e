// Pillow-exact crop + resize + flip of 16-bit ("I;16") depth images over a device job list, and upstream's truncated depth standardisation of
// the crops (include/fourm_hip.h, "Pillow-exact 16-bit depth crops"): the depth side of the data stage whose 8-bit side is pil_resize.hip.
//
// Resize: Pillow's 16bpc path.  The coefficients are the normalised doubles of pil_axis.h (fm_pil_axis_table_f64, HOST); a pass accumulates
// ss += (double)in * k tap by tap, product and sum rounded separately (__dmul_rn / __dadd_rn: never contracted, whatever the flags; the file
// is compiled with -ffp-contract=off as well), rounds half away from zero and clamps PER BYTE.  Two launches as in the 8-bit file: rows into
// a uint16 intermediate (h, S), then columns, flip, and the outputs.  A thread owns one output sample; a workgroup is 256 consecutive
// samples of one job, found by a binary search over the jobs' first workgroups.  Plain vector loads and stores.
//
// Standardisation: one workgroup of 1024 threads per crop, four sweeps over its n values (they stay in L2): a 256-bin histogram of the high
// bytes in LDS, from its prefix sums the bins that hold rank lo and rank hi - 1; histograms of the low bytes inside those two bins, from
// them the boundary values v_lo, v_hi and how many of their ties lie inside [lo, hi); the exact integer sums M1, M2 of the values strictly
// between (per-thread 64-bit partials, wave shuffles, one 64-bit LDS atomic per wave) plus the boundary shares; one thread forms mean and
// variance in 128-bit integer arithmetic; the last sweep writes (x - mean32) / sqrtf(var32 + 1e-6f).  Integer LDS atomics only: the result
// does not depend on the order in which they land.  When all values of a crop share a high byte (a narrow depth band) the histogram atomics
// of a wave hit one address and serialise (not tuned: DESIGN.md has the measured times).
#include <math.h>
#include <stdint.h>

#include "common.h"
#include "fourm_hip.h"
#include "pil_axis.h"

namespace {

constexpr int NT = 256;
constexpr int NT_STD = 1024;
constexpr long long MAX_BLOCKS = (1LL << 32) / NT - 1;          // a grid of 2^32 threads or more is rejected at launch

// ---- resize ---------------------------------------------------------------------------------------------------------------------------------
struct Pil16Args {
    const fm_pil_crop_job* jobs;
    int n_jobs;
    const uint8_t* src;
    const int32_t* tables;
    uint8_t* mid;
    int S;
    int32_t* out_i32;
    float* out_f32;
};

__device__ __forceinline__ int clip8(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

// Pillow's 16bpc store: round half away from zero, then each byte clamped on its own
__device__ __forceinline__ int round_clip16(double ss) {
    const int r = (int)(ss < 0.0 ? __dadd_rn(ss, -0.5) : __dadd_rn(ss, 0.5));
    return clip8(r % 256) | (clip8(r >> 8) << 8);
}

__device__ __forceinline__ float unit_f32(int v) { return (float)__ddiv_rn((double)v, 65535.0); }

template <bool COLS>
__device__ __forceinline__ int find_job(const fm_pil_crop_job* __restrict__ jobs, int n_jobs, long long bid) {
    int lo = 0, hi = n_jobs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((COLS ? jobs[mid].blk_cols : jobs[mid].blk_rows) <= bid) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// one sample of a pass: p[i * ld], i < cnt, against k[i]
__device__ __forceinline__ int filter16(const uint16_t* __restrict__ p, long long ld, const double* __restrict__ k, int cnt) {
    if (cnt == 1 && k[0] == 1.0) return p[0];          // an axis that keeps its size, or nearest: the sample itself
    double ss = 0.0;
    for (int i = 0; i < cnt; ++i) ss = __dadd_rn(ss, __dmul_rn((double)p[i * ld], k[i]));
    return round_clip16(ss);
}

__global__ __launch_bounds__(NT) void pil16_rows_kernel(const Pil16Args a) {
    const long long bid = blockIdx.x;
    const fm_pil_crop_job j = a.jobs[find_job<false>(a.jobs, a.n_jobs, bid)];
    const int S = a.S;
    const long long local = (bid - j.blk_rows) * NT + threadIdx.x;
    if (bid < j.blk_rows || local >= (long long)j.h * S) return;
    const int r = (int)(local / S), o = (int)(local - (long long)r * S);
    const int32_t* __restrict__ tab = a.tables + j.tab_w;
    const int s = tab[o], cnt = tab[S + o];
    const double* __restrict__ k = (const double*)(tab + 2 * S) + (long long)o * j.taps_w;
    const bool ok = s >= 0 && cnt >= 1 && cnt <= j.taps_w && s <= j.w - cnt;
    int v = 0;
    if (ok) v = filter16((const uint16_t*)(a.src + j.src_off) + (long long)(j.top + r) * j.W + j.left + s, 1, k, cnt);
    ((uint16_t*)(a.mid + j.mid_off))[local] = (uint16_t)v;
}

__global__ __launch_bounds__(NT) void pil16_cols_kernel(const Pil16Args a) {
    const long long bid = blockIdx.x;
    const fm_pil_crop_job j = a.jobs[find_job<true>(a.jobs, a.n_jobs, bid)];
    const int S = a.S;
    const long long local = (bid - j.blk_cols) * NT + threadIdx.x;
    if (bid < j.blk_cols || local >= (long long)S * S) return;
    const int oy = (int)(local / S), ox = (int)(local - (long long)oy * S);
    const int32_t* __restrict__ tab = a.tables + j.tab_h;
    const int s = tab[oy], cnt = tab[S + oy];
    const double* __restrict__ k = (const double*)(tab + 2 * S) + (long long)oy * j.taps_h;
    const bool ok = s >= 0 && cnt >= 1 && cnt <= j.taps_h && s <= j.h - cnt;
    int v = 0;
    if (ok) v = filter16((const uint16_t*)(a.mid + j.mid_off) + (long long)s * S + ox, S, k, cnt);
    const int dx = j.flip ? S - 1 - ox : ox;
    const long long pix = ((long long)j.out_slot * S + oy) * S + dx;
    if (a.out_i32) a.out_i32[pix] = v;
    if (a.out_f32) a.out_f32[pix] = unit_f32(v);
}

// ---- standardisation ------------------------------------------------------------------------------------------------------------------------
struct U128 {
    unsigned long long hi, lo;
};

__device__ __forceinline__ U128 mul64(unsigned long long a, unsigned long long b) { return {__umul64hi(a, b), a * b}; }

__device__ __forceinline__ U128 sub128(U128 a, U128 b) { return {a.hi - b.hi - (a.lo < b.lo ? 1ULL : 0ULL), a.lo - b.lo}; }

// a (< 2^64) times b (< 2^64 after the product's high word is known to fit): (a.hi, a.lo) * b, a.hi * b < 2^64 assumed
__device__ __forceinline__ U128 mul128_64(U128 a, unsigned long long b) {
    U128 p = mul64(a.lo, b);
    p.hi += a.hi * b;
    return p;
}

// the double nearest to a 128-bit integer: one rounding.  Above 64 bits the value is shifted right until it fits, the bits shifted out
// ORed into the last bit (sticky: it lies below the rounding position, the top bit of the 64 being set), converted and scaled back.
__device__ __forceinline__ double to_double(U128 a) {
    if (a.hi == 0) return (double)a.lo;          // u64 -> f64 rounds to nearest even
    const int s = 64 - __clzll((long long)a.hi);
    unsigned long long v = (a.hi << (64 - s)) | (a.lo >> s);
    if (a.lo & ((1ULL << s) - 1ULL)) v |= 1ULL;
    return ldexp((double)v, s);
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

struct StdArgs {
    const int32_t* values;
    long long n, lo, hi;
    float* out;
    float* stats;
};

// the bin that holds rank `rank` of a 256-bin histogram whose bins start at rank `base`: (bin, number of elements before the bin)
__device__ __forceinline__ void select_bin(const unsigned* __restrict__ hist, long long base, long long rank, int* bin, long long* before) {
    long long c = base;
    int b = 0;
    for (; b < 255; ++b) {
        if (c + hist[b] > rank) break;
        c += hist[b];
    }
    *bin = b;
    *before = c;
}

__global__ __launch_bounds__(NT_STD) void depth_standardize_kernel(const StdArgs a) {
    __shared__ unsigned hist[2][256];
    __shared__ unsigned long long sums[2];
    __shared__ int sel[2];          // high bytes of the bins of rank lo and rank hi - 1, then v_lo and v_hi
    __shared__ long long before[2];          // elements in front of those bins, then in front of v_lo and v_hi
    __shared__ float ms[2];
    const int t = threadIdx.x;
    const long long n = a.n;
    const int32_t* __restrict__ x = a.values + (long long)blockIdx.x * n;
    if (t < 256) hist[0][t] = hist[1][t] = 0;
    if (t < 2) sums[t] = 0;
    __syncthreads();
    for (long long i = t; i < n; i += NT_STD) atomicAdd(&hist[0][(x[i] >> 8) & 255], 1u);
    __syncthreads();
    if (t < 2) select_bin(hist[0], 0, t == 0 ? a.lo : a.hi - 1, &sel[t], &before[t]);
    __syncthreads();
    const int b_lo = sel[0], b_hi = sel[1];
    for (long long i = t; i < n; i += NT_STD) {
        const int v = x[i] & 0xffff;
        if ((v >> 8) == b_lo) atomicAdd(&hist[1][v & 255], 1u);          // hist[1]: low bytes inside the bin of rank lo
    }
    __syncthreads();
    if (t < 256) hist[0][t] = 0;          // hist[0] again: low bytes inside the bin of rank hi - 1
    __syncthreads();
    for (long long i = t; i < n; i += NT_STD) {
        const int v = x[i] & 0xffff;
        if ((v >> 8) == b_hi) atomicAdd(&hist[0][v & 255], 1u);
    }
    __syncthreads();
    long long c_lt = 0;
    int vb = 0;
    unsigned ties = 0;
    if (t < 2) {
        int low;
        select_bin(hist[1 - t], before[t], t == 0 ? a.lo : a.hi - 1, &low, &c_lt);
        vb = (sel[t] << 8) | low;
        ties = hist[1 - t][low];
    }
    __syncthreads();
    if (t < 2) {
        sel[t] = vb;
        before[t] = c_lt;
        // the ties of the boundary value inside [lo, hi): v_lo's ranks are [c_lt, c_lt + ties), v_hi's likewise
        long long share;
        if (t == 0) {
            const long long end = c_lt + ties < a.hi ? c_lt + ties : a.hi;
            share = end - a.lo;
        } else {
            share = a.hi - (c_lt > a.lo ? c_lt : a.lo);
        }
        hist[1][t] = (unsigned)share;          // share <= n <= 2^28
    }
    __syncthreads();
    const int v_lo = sel[0], v_hi = sel[1];
    unsigned long long m1 = 0, m2 = 0;
    for (long long i = t; i < n; i += NT_STD) {
        const unsigned long long v = (unsigned)(x[i] & 0xffff);
        if ((int)v > v_lo && (int)v < v_hi) {
            m1 += v;
            m2 += v * v;
        }
    }
    m1 = wave_sum(m1);
    m2 = wave_sum(m2);
    if ((t & 63) == 0) {
        atomicAdd(&sums[0], m1);
        atomicAdd(&sums[1], m2);
    }
    __syncthreads();
    if (t == 0) {
        unsigned long long M1 = sums[0], M2 = sums[1];
        const unsigned long long s_lo = hist[1][0], s_hi = v_hi == v_lo ? 0 : hist[1][1];          // one value: its share is counted once
        M1 += s_lo * (unsigned long long)v_lo + s_hi * (unsigned long long)v_hi;
        M2 += s_lo * (unsigned long long)v_lo * v_lo + s_hi * (unsigned long long)v_hi * v_hi;
        const unsigned long long m = (unsigned long long)(a.hi - a.lo);
        const double mean = __ddiv_rn((double)M1, (double)(m * 65535ULL));          // both below 2^53: exact conversions
        const U128 num = sub128(mul64(m, M2), mul64(M1, M1));          // >= 0 (Cauchy-Schwarz), exact
        const U128 den = mul128_64(mul64(m * (m - 1), 65535ULL), 65535ULL);
        const double var = __ddiv_rn(to_double(num), to_double(den));
        ms[0] = (float)mean;
        ms[1] = (float)var;
        if (a.stats) {
            a.stats[2 * (long long)blockIdx.x] = ms[0];
            a.stats[2 * (long long)blockIdx.x + 1] = ms[1];
        }
    }
    __syncthreads();
    if (!a.out) return;
    const float mean32 = ms[0];
    // sqrtf correctly rounded: the fp32 square root instruction alone is good to one ulp only; the double root of an fp32 value rounds to
    // the nearest fp32 of the exact root (53 >= 2 * 24 + 2 bits: the second rounding cannot change the result)
    const float sd = (float)sqrt((double)__fadd_rn(ms[1], 1e-6f));
    float* __restrict__ y = a.out + (long long)blockIdx.x * n;
    for (long long i = t; i < n; i += NT_STD) y[i] = __fdiv_rn(__fsub_rn(unit_f32(x[i] & 0xffff), mean32), sd);
}

inline bool aligned(const void* p, uintptr_t a) { return (((uintptr_t)p) & (a - 1)) == 0; }

inline double identity(double k) { return k; }

}  // namespace

extern "C" int fm_pil_axis_table_f64(int n_in, int n_out, int filter, int32_t* start, int32_t* count, double* coef) {
    return pil_axis::table("fm_pil_axis_table_f64", n_in, n_out, filter, true, start, count, coef, identity);
}

extern "C" int fm_pil_crop_resize16(const fm_pil_crop_job* jobs_host, const void* jobs_dev, int n_jobs, const void* src, int64_t src_bytes, const void* tables,
                                    int64_t table_words, void* scratch, int64_t scratch_bytes, int S, void* out_i32, void* out_f32, int64_t n_slots, void* stream) {
    FM_CHECK_ARG(jobs_host && jobs_dev && src && tables && scratch && n_jobs > 0 && aligned(jobs_dev, 8) && aligned(tables, 8) && aligned(src, 2) && aligned(scratch, 2),
                 "fm_pil_crop_resize16: no job list, source, tables or scratch (or one of them misaligned)");
    FM_CHECK_ARG(S >= 1 && S <= 16384 && n_slots > 0 && src_bytes > 0 && table_words > 0 && scratch_bytes > 0, "fm_pil_crop_resize16: S=%d (1 .. 16384) slots=%lld", S,
                 (long long)n_slots);
    FM_CHECK_ARG(out_i32 || out_f32, "fm_pil_crop_resize16: no output");
    FM_CHECK_ARG(aligned(out_i32, 4) && aligned(out_f32, 4), "fm_pil_crop_resize16: misaligned output");
    FM_CHECK_ARG((double)n_slots * S * (double)S <= 1.0e12, "fm_pil_crop_resize16: output too large");
    long long blocks_rows = 0, blocks_cols = 0;
    const long long per_cols = ((long long)S * S + NT - 1) / NT;
    for (int i = 0; i < n_jobs; ++i) {
        const fm_pil_crop_job& j = jobs_host[i];
        FM_CHECK_ARG(j.H > 0 && j.W > 0 && j.H <= (1 << 24) && j.W <= (1 << 24) && j.src_off >= 0 && (j.src_off & 1) == 0 && j.src_off <= src_bytes &&
                         2LL * j.H * j.W <= src_bytes - j.src_off,
                     "fm_pil_crop_resize16: job %d: image %d x %d at byte %lld outside the source buffer", i, j.H, j.W, (long long)j.src_off);
        FM_CHECK_ARG(j.h >= 1 && j.w >= 1 && j.top >= 0 && j.left >= 0 && j.h <= j.H - j.top && j.w <= j.W - j.left,
                     "fm_pil_crop_resize16: job %d: box (top %d, left %d, h %d, w %d) leaves the %d x %d image", i, j.top, j.left, j.h, j.w, j.H, j.W);
        FM_CHECK_ARG(j.flip == 0 || j.flip == 1, "fm_pil_crop_resize16: job %d: flip %d", i, j.flip);
        FM_CHECK_ARG(j.taps_w >= 1 && j.taps_w <= FM_PIL_MAX_TAPS && j.taps_h >= 1 && j.taps_h <= FM_PIL_MAX_TAPS && j.tab_w >= 0 && j.tab_h >= 0 &&
                         (j.tab_w & 1) == 0 && (j.tab_h & 1) == 0 && j.tab_w + (long long)S * (2 + 2 * j.taps_w) <= table_words &&
                         j.tab_h + (long long)S * (2 + 2 * j.taps_h) <= table_words,
                     "fm_pil_crop_resize16: job %d: tables outside the table buffer", i);
        FM_CHECK_ARG(j.mid_off >= 0 && (j.mid_off & 1) == 0 && j.mid_off <= scratch_bytes && 2LL * j.h * S <= scratch_bytes - j.mid_off,
                     "fm_pil_crop_resize16: job %d: intermediate outside the scratch (%lld bytes)", i, (long long)scratch_bytes);
        FM_CHECK_ARG(j.out_slot >= 0 && j.out_slot < n_slots, "fm_pil_crop_resize16: job %d: output slot %lld of %lld", i, (long long)j.out_slot, (long long)n_slots);
        FM_CHECK_ARG(j.blk_rows == blocks_rows && j.blk_cols == blocks_cols, "fm_pil_crop_resize16: job %d: first workgroups (%lld, %lld), expected (%lld, %lld)", i,
                     (long long)j.blk_rows, (long long)j.blk_cols, blocks_rows, blocks_cols);
        blocks_rows += ((long long)j.h * S + NT - 1) / NT;
        blocks_cols += per_cols;
        FM_CHECK_ARG(blocks_rows <= MAX_BLOCKS && blocks_cols <= MAX_BLOCKS, "fm_pil_crop_resize16: more than %lld workgroups in a launch (split the call)", MAX_BLOCKS);
    }
    Pil16Args a = {};
    a.jobs = (const fm_pil_crop_job*)jobs_dev; a.n_jobs = n_jobs;
    a.src = (const uint8_t*)src; a.tables = (const int32_t*)tables; a.mid = (uint8_t*)scratch;
    a.S = S; a.out_i32 = (int32_t*)out_i32; a.out_f32 = (float*)out_f32;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(pil16_rows_kernel, dim3((unsigned)blocks_rows), dim3(NT), 0, st, a);
    hipLaunchKernelGGL(pil16_cols_kernel, dim3((unsigned)blocks_cols), dim3(NT), 0, st, a);
    FM_CHECK_LAUNCH("fm_pil_crop_resize16");
    return 0;
}

extern "C" int fm_depth_standardize(const void* values_i32, int n_crops, int64_t n, int64_t lo, int64_t hi, void* out_f32, void* stats, void* stream) {
    FM_CHECK_ARG(values_i32 && n_crops > 0 && aligned(values_i32, 4) && aligned(out_f32, 4) && aligned(stats, 4), "fm_depth_standardize: no values (or a misaligned pointer)");
    FM_CHECK_ARG(out_f32 || stats, "fm_depth_standardize: no output");
    FM_CHECK_ARG(n >= 2 && n <= (1LL << 28), "fm_depth_standardize: %lld values per crop (2 .. 2^28)", (long long)n);
    FM_CHECK_ARG(lo >= 0 && hi <= n && hi - lo >= 2, "fm_depth_standardize: rank range [%lld, %lld) of %lld values: at least two elements inside the crop are needed",
                 (long long)lo, (long long)hi, (long long)n);
    StdArgs a = {};
    a.values = (const int32_t*)values_i32; a.n = n; a.lo = lo; a.hi = hi; a.out = (float*)out_f32; a.stats = (float*)stats;
    hipLaunchKernelGGL(depth_standardize_kernel, dim3((unsigned)n_crops), dim3(NT_STD), 0, (hipStream_t)stream, a);
    FM_CHECK_LAUNCH("fm_depth_standardize");
    return 0;
}
