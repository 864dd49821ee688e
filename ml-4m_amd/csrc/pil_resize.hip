// Pillow-exact crop + resize + flip of 8-bit images over a device job list (include/fourm_hip.h, "Pillow-exact crops"): the data stage of
// dataset pre-tokenization.  One job is one crop of one source image; many images of different sizes and all their crops go in one call.
//
// The arithmetic is Pillow's 8-bit path, integer from the coefficient tables on: fm_pil_axis_table (HOST, pil_axis.h) makes the table of one axis
// in double in Pillow's operation order - this file is compiled with -ffp-contract=off so that no multiply-add is contracted - and rounds
// it to the 22-bit fixed-point coefficients Pillow uses.  The device side is two launches:
//   rows:    every row of the crop is filtered along its columns into a uint8 intermediate (h, S, C) - Pillow's horizontal pass, its rounding
//            to 8 bits included;
//   columns: the intermediate is filtered along its rows, then flipped, inverted where asked, and written as HWC uint8, and / or NCHW fp32
//            through a C x 256 lookup table, or as an int64 class map.
// A thread owns one output pixel with all its channels (C <= 4 accumulators in registers); a workgroup is 256 consecutive pixels of one job,
// found by a binary search over the jobs' first workgroups (the pattern of fm_ema_update).  In the rows pass consecutive lanes read source
// pixels a scale factor apart and write consecutive bytes; in the columns pass they read and write consecutive pixels.  The tables are a few
// KiB per axis and are read through the caches.  Every job is validated on the host before the first launch; a table entry is used as an
// index only after a check against the crop (a pixel whose table row is inconsistent is written as 0).  Plain vector loads and stores, no
// atomics: two calls give the same bytes.
#include <math.h>
#include <stdint.h>

#include <vector>

#include "common.h"
#include "fourm_hip.h"
#include "pil_axis.h"

namespace {

constexpr int NT = 256;
constexpr long long MAX_BLOCKS = (1LL << 32) / NT - 1;          // a grid of 2^32 threads or more is rejected at launch
constexpr int PRECISION_BITS = 22;          // Pillow's 32 - 8 - 2

// ---- host: the table of one axis (pil_axis.h; shared with the 16-bit path) -----------------------------------------------------------------------
inline int32_t fixed_point(double k) {
    return k < 0 ? (int32_t)(-0.5 + k * (1 << PRECISION_BITS)) : (int32_t)(0.5 + k * (1 << PRECISION_BITS));
}

// ---- device ---------------------------------------------------------------------------------------------------------------------------------
struct PilArgs {
    const fm_pil_crop_job* jobs;
    int n_jobs;
    const uint8_t* src;
    const int32_t* tables;
    uint8_t* mid;
    int S;
    int invert;
    const float* lut;
    uint8_t* out_u8;
    float* out_f32;
    long long* out_i64;
};

__device__ __forceinline__ int clip8(int acc) {
    const int v = acc >> PRECISION_BITS;          // arithmetic shift
    return v < 0 ? 0 : v > 255 ? 255 : v;
}

// the last job whose first workgroup of this pass is <= bid
template <bool COLS>
__device__ __forceinline__ int find_job(const fm_pil_crop_job* __restrict__ jobs, int n_jobs, long long bid) {
    int lo = 0, hi = n_jobs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((COLS ? jobs[mid].blk_cols : jobs[mid].blk_rows) <= bid) lo = mid; else hi = mid - 1;
    }
    return lo;
}

template <int C>
__global__ __launch_bounds__(NT) void pil_rows_kernel(const PilArgs a) {
    const long long bid = blockIdx.x;
    const fm_pil_crop_job j = a.jobs[find_job<false>(a.jobs, a.n_jobs, bid)];
    const int S = a.S;
    const long long local = (bid - j.blk_rows) * NT + threadIdx.x;
    if (bid < j.blk_rows || local >= (long long)j.h * S) return;
    const int r = (int)(local / S), o = (int)(local - (long long)r * S);
    const int32_t* __restrict__ tab = a.tables + j.tab_w;
    const int s = tab[o], cnt = tab[S + o];
    const int32_t* __restrict__ k = tab + 2 * S + (long long)o * j.taps_w;
    const bool ok = s >= 0 && cnt >= 0 && cnt <= j.taps_w && s <= j.w - cnt;
    int acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = 1 << (PRECISION_BITS - 1);
    if (ok) {
        const uint8_t* __restrict__ p = a.src + j.src_off + ((long long)(j.top + r) * j.W + j.left + s) * C;
        for (int i = 0; i < cnt; ++i) {
            const int kk = k[i];
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] += (int)p[i * C + c] * kk;
        }
    }
    uint8_t* __restrict__ m = a.mid + j.mid_off + local * C;
#pragma unroll
    for (int c = 0; c < C; ++c) m[c] = ok ? (uint8_t)clip8(acc[c]) : (uint8_t)0;
}

template <int C>
__global__ __launch_bounds__(NT) void pil_cols_kernel(const PilArgs a) {
    const long long bid = blockIdx.x;
    const fm_pil_crop_job j = a.jobs[find_job<true>(a.jobs, a.n_jobs, bid)];
    const int S = a.S;
    const long long local = (bid - j.blk_cols) * NT + threadIdx.x;
    if (bid < j.blk_cols || local >= (long long)S * S) return;
    const int oy = (int)(local / S), ox = (int)(local - (long long)oy * S);
    const int32_t* __restrict__ tab = a.tables + j.tab_h;
    const int s = tab[oy], cnt = tab[S + oy];
    const int32_t* __restrict__ k = tab + 2 * S + (long long)oy * j.taps_h;
    const bool ok = s >= 0 && cnt >= 0 && cnt <= j.taps_h && s <= j.h - cnt;
    int acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = 1 << (PRECISION_BITS - 1);
    if (ok) {
        const uint8_t* __restrict__ p = a.mid + j.mid_off + ((long long)s * S + ox) * C;
        const long long ld = (long long)S * C;
        for (int i = 0; i < cnt; ++i) {
            const int kk = k[i];
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] += (int)p[i * ld + c] * kk;
        }
    }
    const int dx = j.flip ? S - 1 - ox : ox;
    const long long pix = ((long long)j.out_slot * S + oy) * S + dx;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        int v = ok ? clip8(acc[c]) : 0;
        if (j.flip && ((a.invert >> c) & 1)) v = 255 - v;
        if (a.out_u8) a.out_u8[pix * C + c] = (uint8_t)v;
        if (a.out_f32) a.out_f32[(((long long)j.out_slot * C + c) * S + oy) * S + dx] = a.lut[c * 256 + v];
        if (C == 1 && a.out_i64) a.out_i64[pix] = v;
    }
}

template <int C>
void launch_both(const PilArgs& a, long long blocks_rows, long long blocks_cols, hipStream_t st) {
    hipLaunchKernelGGL(pil_rows_kernel<C>, dim3((unsigned)blocks_rows), dim3(NT), 0, st, a);
    hipLaunchKernelGGL(pil_cols_kernel<C>, dim3((unsigned)blocks_cols), dim3(NT), 0, st, a);
}

inline bool aligned(const void* p, uintptr_t a) { return (((uintptr_t)p) & (a - 1)) == 0; }

}  // namespace

extern "C" int fm_pil_axis_table(int n_in, int n_out, int filter, int32_t* start, int32_t* count, int32_t* coef) {
    return pil_axis::table("fm_pil_axis_table", n_in, n_out, filter, false, start, count, coef, fixed_point);
}

extern "C" int fm_pil_crop_resize(const fm_pil_crop_job* jobs_host, const void* jobs_dev, int n_jobs, const void* src, int64_t src_bytes, const void* tables,
                                  int64_t table_words, void* scratch, int64_t scratch_bytes, int C, int S, int invert_mask, const void* lut, void* out_u8,
                                  void* out_f32, void* out_i64, int64_t n_slots, void* stream) {
    FM_CHECK_ARG(jobs_host && jobs_dev && src && tables && scratch && n_jobs > 0 && aligned(jobs_dev, 8) && aligned(tables, 4), "fm_pil_crop_resize: no job list, source, tables or scratch");
    FM_CHECK_ARG(C >= 1 && C <= 4 && S >= 1 && S <= 16384 && n_slots > 0 && src_bytes > 0 && table_words > 0 && scratch_bytes > 0,
                 "fm_pil_crop_resize: C=%d (1 .. 4) S=%d (1 .. 16384) slots=%lld", C, S, (long long)n_slots);
    FM_CHECK_ARG(out_u8 || out_f32 || out_i64, "fm_pil_crop_resize: no output");
    FM_CHECK_ARG(!out_f32 || (lut && aligned(lut, 4) && aligned(out_f32, 4)), "fm_pil_crop_resize: the fp32 output needs the lookup table (C x 256 f32)");
    FM_CHECK_ARG(!out_i64 || (C == 1 && aligned(out_i64, 8)), "fm_pil_crop_resize: the int64 output is for one-channel maps");
    FM_CHECK_ARG((invert_mask & ~((1 << C) - 1)) == 0, "fm_pil_crop_resize: invert_mask 0x%x names channels outside C=%d", invert_mask, C);
    FM_CHECK_ARG((double)n_slots * S * (double)S * C <= 4.0e12, "fm_pil_crop_resize: output too large");
    long long blocks_rows = 0, blocks_cols = 0;
    const long long per_cols = ((long long)S * S + NT - 1) / NT;
    for (int i = 0; i < n_jobs; ++i) {
        const fm_pil_crop_job& j = jobs_host[i];
        FM_CHECK_ARG(j.H > 0 && j.W > 0 && j.H <= (1 << 24) && j.W <= (1 << 24) && j.src_off >= 0 && j.src_off <= src_bytes &&
                         (long long)j.H * j.W * C <= src_bytes - j.src_off,
                     "fm_pil_crop_resize: job %d: image %d x %d at byte %lld outside the source buffer", i, j.H, j.W, (long long)j.src_off);
        FM_CHECK_ARG(j.h >= 1 && j.w >= 1 && j.top >= 0 && j.left >= 0 && j.h <= j.H - j.top && j.w <= j.W - j.left,
                     "fm_pil_crop_resize: job %d: box (top %d, left %d, h %d, w %d) leaves the %d x %d image", i, j.top, j.left, j.h, j.w, j.H, j.W);
        FM_CHECK_ARG(j.flip == 0 || j.flip == 1, "fm_pil_crop_resize: job %d: flip %d", i, j.flip);
        FM_CHECK_ARG(j.taps_w >= 1 && j.taps_w <= FM_PIL_MAX_TAPS && j.taps_h >= 1 && j.taps_h <= FM_PIL_MAX_TAPS && j.tab_w >= 0 && j.tab_h >= 0 &&
                         j.tab_w + (long long)S * (2 + j.taps_w) <= table_words && j.tab_h + (long long)S * (2 + j.taps_h) <= table_words,
                     "fm_pil_crop_resize: job %d: tables outside the table buffer", i);
        FM_CHECK_ARG(j.mid_off >= 0 && j.mid_off <= scratch_bytes && (long long)j.h * S * C <= scratch_bytes - j.mid_off,
                     "fm_pil_crop_resize: job %d: intermediate outside the scratch (%lld bytes)", i, (long long)scratch_bytes);
        FM_CHECK_ARG(j.out_slot >= 0 && j.out_slot < n_slots, "fm_pil_crop_resize: job %d: output slot %lld of %lld", i, (long long)j.out_slot, (long long)n_slots);
        FM_CHECK_ARG(j.blk_rows == blocks_rows && j.blk_cols == blocks_cols, "fm_pil_crop_resize: job %d: first workgroups (%lld, %lld), expected (%lld, %lld)", i,
                     (long long)j.blk_rows, (long long)j.blk_cols, blocks_rows, blocks_cols);
        blocks_rows += ((long long)j.h * S + NT - 1) / NT;
        blocks_cols += per_cols;
        FM_CHECK_ARG(blocks_rows <= MAX_BLOCKS && blocks_cols <= MAX_BLOCKS, "fm_pil_crop_resize: more than %lld workgroups in a launch (split the call)", MAX_BLOCKS);
    }
    PilArgs a = {};
    a.jobs = (const fm_pil_crop_job*)jobs_dev; a.n_jobs = n_jobs;
    a.src = (const uint8_t*)src; a.tables = (const int32_t*)tables; a.mid = (uint8_t*)scratch;
    a.S = S; a.invert = invert_mask; a.lut = (const float*)lut;
    a.out_u8 = (uint8_t*)out_u8; a.out_f32 = (float*)out_f32; a.out_i64 = (long long*)out_i64;
    hipStream_t st = (hipStream_t)stream;
    switch (C) {
        case 1: launch_both<1>(a, blocks_rows, blocks_cols, st); break;
        case 2: launch_both<2>(a, blocks_rows, blocks_cols, st); break;
        case 3: launch_both<3>(a, blocks_rows, blocks_cols, st); break;
        default: launch_both<4>(a, blocks_rows, blocks_cols, st); break;
    }
    FM_CHECK_LAUNCH("fm_pil_crop_resize");
    return 0;
}
