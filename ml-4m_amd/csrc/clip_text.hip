// CLIP's text tower and the CLIP score: the two ends that the trunk's kernels do not cover (include/fourm_hip.h, "CLIP text tower").
//   fm_clip_text_embed     token rows + position rows -> the fp32 residual stream, and the end-of-text row of every sample (first maximum of
//                          its ids, as torch.argmax).  Ids are range-checked before they index the table.
//   fm_clip_pair_score     100 cos(img_b, txt_b) per pair and the sum of the scores in double.
//   fm_l2_normalize_rows   x / |x| (times a factor) per row, the operands of CLIP's logits.
// Everything is fp32 and row-local.  One wavefront owns a row (pair): lane l accumulates elements l, l + 64, ... in index order, then the
// shuffle tree - a fixed order, no floating-point atomics, two calls give the same bits.  The normalisation of a finished fp32 sum (the
// square roots and the division) is done in double and rounded to fp32 once.
#include <math.h>

#include "common.h"
#include "fourm_hip.h"

namespace {

constexpr int EMBED_ROWS = 8;          // token rows per workgroup of the embedding kernel
constexpr int PAIRS = 4;               // rows (pairs) per workgroup of the two reductions: one per wavefront

// grid (ceil(Lc / EMBED_ROWS), B).  The first workgroup of a sample also finds its end-of-text row (wavefront 0).
__global__ __launch_bounds__(256) void clip_text_embed_kernel(const long long* __restrict__ ids, const float* __restrict__ tok, const float* __restrict__ pos,
                                                              float* __restrict__ out, int ldo, int* __restrict__ eot_row, int* __restrict__ eot_map,
                                                              int* __restrict__ bad, int Lc, int D, int V) {
    __shared__ int eot_s;
    const int b = blockIdx.y, t0 = blockIdx.x * EMBED_ROWS;
    const long long* idb = ids + (long long)b * Lc;
    if (threadIdx.x < 64) {                                            // (every workgroup of the sample: its rows of eot_map need the position)
        long long best = idb[0];
        int at = 0;
        for (int t = threadIdx.x; t < Lc; t += 64) {                   // (t ascending: a lane keeps the first of its equal values)
            const long long v = idb[t];
            if (v > best || (v == best && t < at)) { best = v; at = t; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const long long ov = __shfl_xor(best, o, 64);
            const int oa = __shfl_xor(at, o, 64);
            if (ov > best || (ov == best && oa < at)) { best = ov; at = oa; }
        }
        if (threadIdx.x == 0) {
            eot_s = at;
            if (blockIdx.x == 0) eot_row[b] = b * Lc + at;
        }
    }
    __syncthreads();
    const int D4 = D >> 2;
    const int rows = min(EMBED_ROWS, Lc - t0);
    if (eot_map && threadIdx.x < rows) eot_map[b * Lc + t0 + threadIdx.x] = t0 + (int)threadIdx.x == eot_s ? b : -1;
    for (int i = threadIdx.x; i < rows * D4; i += 256) {
        const int r = i / D4, c = i - r * D4;
        const int t = t0 + r;
        const long long id = idb[t];
        f32x4_t v = {0.f, 0.f, 0.f, 0.f};
        if (id >= 0 && id < V) {
            const f32x4_t a = *(const f32x4_t*)(tok + id * D + 4 * c);
            const f32x4_t p = *(const f32x4_t*)(pos + (long long)t * D + 4 * c);
            v = a + p;
        } else if (c == 0) atomicAdd(bad, 1);
        *(f32x4_t*)(out + ((long long)b * Lc + t) * ldo + 4 * c) = v;
    }
}

// one wavefront per pair; the workgroup's (up to) four scores leave as one double partial, added in pair order
__global__ __launch_bounds__(256) void clip_pair_score_kernel(const float* __restrict__ img, int ldi, const float* __restrict__ txt, int ldt,
                                                              float* __restrict__ score, double* __restrict__ scratch, int B, int E) {
    __shared__ double part[PAIRS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.x * PAIRS + wave;
    double s = 0.0;
    if (b < B) {
        const float* x = img + (long long)b * ldi;
        const float* y = txt + (long long)b * ldt;
        float dot = 0.f, nx = 0.f, ny = 0.f;
        for (int e = lane; e < E; e += 64) {
            const float a = x[e], c = y[e];
            dot += a * c; nx += a * a; ny += c * c;
        }
        dot = wave_sum(dot); nx = wave_sum(nx); ny = wave_sum(ny);
        const double den = sqrt((double)nx) * sqrt((double)ny);
        const float sc = den > 0.0 ? (float)(100.0 * (double)dot / den) : 0.f;      // (a zero-norm row: 0, not 0 / 0)
        if (lane == 0) score[b] = sc;
        s = (double)sc;
    }
    if (lane == 0) part[wave] = s;
    __syncthreads();
    if (threadIdx.x == 0) scratch[blockIdx.x] = ((part[0] + part[1]) + part[2]) + part[3];
}

// the workgroups' partials in index order (thread i takes partials i, i + 256, ...; the shuffle tree; the four wavefronts in order)
__global__ __launch_bounds__(256) void clip_pair_score_finish_kernel(const double* __restrict__ scratch, int parts, int B, double* __restrict__ sum,
                                                                     long long* __restrict__ count) {
    __shared__ double part[4];
    double a = 0.0;
    for (int i = threadIdx.x; i < parts; i += 256) a += scratch[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) {
        sum[0] += ((part[0] + part[1]) + part[2]) + part[3];
        if (count) count[0] += B;
    }
}

// one wavefront per row; a lane writes only the elements it has read itself, after the row's sum is complete (x == y, in place, is allowed)
__global__ __launch_bounds__(256) void l2_normalize_rows_kernel(const float* x, int ldx, float* y, int ldy, int R, int E,
                                                                const float* __restrict__ factor_dev, float factor) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * PAIRS + (threadIdx.x >> 6);
    if (r >= R) return;
    const float* xr = x + (long long)r * ldx;
    float* yr = y + (long long)r * ldy;
    float ss = 0.f;
    for (int e = lane; e < E; e += 64) { const float a = xr[e]; ss += a * a; }
    ss = wave_sum(ss);
    const double f = (double)factor * (factor_dev ? (double)factor_dev[0] : 1.0);
    const float inv = ss > 0.f ? (float)(f / sqrt((double)ss)) : 0.f;                // (a zero row stays zero)
    for (int e = lane; e < E; e += 64) yr[e] = xr[e] * inv;
}

inline bool aligned(const void* p, uintptr_t a) { return (((uintptr_t)p) & (a - 1)) == 0; }

}  // namespace

extern "C" int fm_clip_text_embed(const void* ids, const void* token_embedding, const void* positional_embedding, void* out, int ldo, void* eot_row,
                                  void* eot_map, void* bad, int B, int Lc, int D, int V, void* stream) {
    FM_CHECK_ARG(ids && token_embedding && positional_embedding && out && eot_row && bad, "fm_clip_text_embed: null pointer");
    FM_CHECK_ARG(B > 0 && Lc > 0 && D > 0 && V > 0, "fm_clip_text_embed: bad shape (B=%d Lc=%d D=%d V=%d)", B, Lc, D, V);
    FM_CHECK_ARG(D % 4 == 0 && ldo % 4 == 0 && ldo >= D, "fm_clip_text_embed: D=%d and ldo=%d must be multiples of 4, ldo >= D", D, ldo);
    FM_CHECK_ARG((double)B * Lc <= (double)0x7fffffff && B <= 65535, "fm_clip_text_embed: B=%d x Lc=%d rows are too many", B, Lc);
    FM_CHECK_ARG(aligned(ids, 8) && aligned(token_embedding, 16) && aligned(positional_embedding, 16) && aligned(out, 16) && aligned(eot_row, 4) && aligned(eot_map, 4) && aligned(bad, 4),
                 "fm_clip_text_embed: misaligned pointer");
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(bad, 0, sizeof(int), st) != hipSuccess) { fm_set_error("fm_clip_text_embed: hipMemsetAsync failed"); return -2; }
    hipLaunchKernelGGL(clip_text_embed_kernel, dim3((Lc + EMBED_ROWS - 1) / EMBED_ROWS, B), dim3(256), 0, st, (const long long*)ids, (const float*)token_embedding,
                       (const float*)positional_embedding, (float*)out, ldo, (int*)eot_row, (int*)eot_map, (int*)bad, Lc, D, V);
    FM_CHECK_LAUNCH("fm_clip_text_embed");
    return 0;
}

extern "C" int fm_clip_pair_score_scratch(int B) {
    FM_CHECK_ARG(B > 0, "fm_clip_pair_score_scratch: B=%d", B);
    return (B + PAIRS - 1) / PAIRS;
}

extern "C" int fm_clip_pair_score(const void* img, int ldi, const void* txt, int ldt, void* score, void* scratch, void* sum, void* count, int B, int E,
                                  void* stream) {
    FM_CHECK_ARG(img && txt && score && scratch && sum, "fm_clip_pair_score: null pointer");
    FM_CHECK_ARG(B > 0 && E > 0 && ldi >= E && ldt >= E, "fm_clip_pair_score: bad shape (B=%d E=%d ldi=%d ldt=%d)", B, E, ldi, ldt);
    FM_CHECK_ARG(aligned(img, 4) && aligned(txt, 4) && aligned(score, 4) && aligned(scratch, 8) && aligned(sum, 8) && aligned(count, 8),
                 "fm_clip_pair_score: misaligned pointer");
    hipStream_t st = (hipStream_t)stream;
    const int parts = (B + PAIRS - 1) / PAIRS;
    hipLaunchKernelGGL(clip_pair_score_kernel, dim3(parts), dim3(256), 0, st, (const float*)img, ldi, (const float*)txt, ldt, (float*)score, (double*)scratch, B, E);
    FM_CHECK_LAUNCH("fm_clip_pair_score");
    hipLaunchKernelGGL(clip_pair_score_finish_kernel, dim3(1), dim3(256), 0, st, (const double*)scratch, parts, B, (double*)sum, (long long*)count);
    FM_CHECK_LAUNCH("fm_clip_pair_score (finish)");
    return 0;
}

extern "C" int fm_l2_normalize_rows(const void* x, int ldx, void* y, int ldy, int R, int E, const void* factor_dev, float factor, void* stream) {
    FM_CHECK_ARG(x && y, "fm_l2_normalize_rows: null pointer");
    FM_CHECK_ARG(R > 0 && E > 0 && ldx >= E && ldy >= E, "fm_l2_normalize_rows: bad shape (R=%d E=%d ldx=%d ldy=%d)", R, E, ldx, ldy);
    FM_CHECK_ARG(aligned(x, 4) && aligned(y, 4) && aligned(factor_dev, 4), "fm_l2_normalize_rows: misaligned pointer");
    hipLaunchKernelGGL(l2_normalize_rows_kernel, dim3((R + PAIRS - 1) / PAIRS), dim3(256), 0, (hipStream_t)stream, (const float*)x, ldx, (float*)y, ldy, R, E,
                       (const float*)factor_dev, factor);
    FM_CHECK_LAUNCH("fm_l2_normalize_rows");
    return 0;
}
