// Tokenizer validation metrics: what upstream's eval_metrics (run_training_vqvae.py:1427-1632) gets from torchmetrics, as kernels
// (include/fourm_hip.h, "tokenizer validation metrics").  The inputs are fp32 images (B, C, H, W) of which the first C_use channels are read in
// place (no slice copy); the conversion of upstream's domain table - the denormalisation (v + 1) / 2, the sigmoid of a mask prediction - happens
// in the loads.  Per-element and per-position arithmetic is fp32, compiled with -ffp-contract=off so that every operation is rounded on its own
// (the denormalisation is one fp32 add and an exact halving, as TF.normalize with mean -1 and std 2 computes it).  Sums over elements, positions
// and tiles are carried in double: per thread, then the shuffle tree, the four wavefronts in order, per-workgroup partials in caller-owned
// scratch and a second launch that adds those in index order.  No floating-point atomics: two calls on the same inputs give the same bits.  The
// integer atomics (IoU counts, the token histogram) do not depend on the order.
//
// SSIM at one scale: one workgroup per (plane, 32 x 32 tile of window positions).  The haloed tile of both images (at most 42 x 42 each) is
// staged in LDS, the five moments x, y, x^2, y^2, xy are filtered along the rows into LDS (42 x 32 each), then along the columns in registers.
// In both passes the 32 lanes of a half wavefront read consecutive words of one LDS row: no bank conflicts.
#include <math.h>

#include "common.h"
#include "fourm_hip.h"

namespace {

constexpr int T = FM_SSIM_TILE;                     // window positions per tile edge
constexpr int KM = FM_SSIM_MAX_KERNEL;              // taps of the longest window
constexpr int IN = T + KM - 1;                      // input rows / columns of a tile with the longest window

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// workgroup (256 threads) sum in a fixed order: the lanes by the shuffle tree, then the 4 wavefronts in order
__device__ __forceinline__ double block_sum_d(double v, double* part) {
    v = wave_sum_d(v);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    const double s = ((part[0] + part[1]) + part[2]) + part[3];
    __syncthreads();                                                                // (part is free for the next sum)
    return s;
}

__device__ __forceinline__ float conv_pred(float v, int transform) {
    if (transform == FM_METRIC_DENORM) return (v + 1.0f) * 0.5f;
    if (transform == FM_METRIC_SIGMOID_PRED) return 1.0f / (1.0f + expf(-v));
    return v;
}
__device__ __forceinline__ float conv_target(float v, int transform) { return transform == FM_METRIC_DENORM ? (v + 1.0f) * 0.5f : v; }

// ---- sum d^2, sum |d| and the IoU counts ------------------------------------------------------------------------------------------------------
// Element e of the B C_use HW that are read is (b, c, hw) in that order; workgroup w owns elements [w, w + 1) FM_METRIC_CHUNK, thread t of it
// elements t, t + 256, ...: the partition depends on the three sizes only, not on the channel strides.
__global__ __launch_bounds__(256) void metric_sums_kernel(const float* __restrict__ pred, const float* __restrict__ target, int Cp, int Ct, int C_use, long long HW,
                                                          long long n, int transform, int iou, float threshold, double* __restrict__ scratch,
                                                          unsigned long long* __restrict__ counts) {
    __shared__ double part[4];
    const long long base = (long long)blockIdx.x * FM_METRIC_CHUNK;
    double ssq = 0.0, sab = 0.0;
    int tp = 0, fp = 0, fn = 0, bad = 0;
    for (int it = 0; it < FM_METRIC_CHUNK / 256; ++it) {
        const long long e = base + it * 256 + threadIdx.x;
        if (e >= n) break;
        const long long row = e / HW, hw = e - row * HW;
        const long long b = row / C_use, c = row - b * C_use;
        const float p = conv_pred(pred[(b * Cp + c) * HW + hw], transform);
        const float t = conv_target(target[(b * Ct + c) * HW + hw], transform);
        const float d = p - t;
        ssq += (double)(d * d);
        sab += (double)fabsf(d);
        if (iou) {
            const bool pp = fminf(fmaxf(p, 0.0f), 1.0f) > threshold;                // (a NaN prediction is clamped to 0)
            const bool tpos = t == 1.0f;
            tp += pp && tpos; fp += pp && !tpos; fn += !pp && tpos;
            bad += !(tpos || t == 0.0f);
        }
    }
    const double s0 = block_sum_d(ssq, part), s1 = block_sum_d(sab, part);
    if (threadIdx.x == 0) { scratch[2 * (long long)blockIdx.x] = s0; scratch[2 * (long long)blockIdx.x + 1] = s1; }
    if (iou) {
        tp = wave_sum_i(tp); fp = wave_sum_i(fp); fn = wave_sum_i(fn); bad = wave_sum_i(bad);
        if ((threadIdx.x & 63) == 0) {
            if (tp) atomicAdd(counts + 0, (unsigned long long)tp);
            if (fp) atomicAdd(counts + 1, (unsigned long long)fp);
            if (fn) atomicAdd(counts + 2, (unsigned long long)fn);
            if (bad) atomicAdd(counts + 4, (unsigned long long)bad);
        }
    }
}

// the workgroups' partials in index order (thread i takes partials i, i + 256, ...; then the tree) onto the accumulators
__global__ __launch_bounds__(256) void metric_sums_finish_kernel(const double* __restrict__ scratch, long long parts, long long n, double* __restrict__ sums,
                                                                 long long* __restrict__ counts) {
    __shared__ double part[4];
    double a = 0.0, b = 0.0;
    for (long long i = threadIdx.x; i < parts; i += 256) { a += scratch[2 * i]; b += scratch[2 * i + 1]; }
    a = block_sum_d(a, part);
    b = block_sum_d(b, part);
    if (threadIdx.x == 0) { sums[0] += a; sums[1] += b; counts[3] += n; }
}

// ---- SSIM at one scale ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ssim_scale_kernel(const float* __restrict__ x, const float* __restrict__ y, int Cx, int Cy, int C_use, int H, int W, int transform,
                                                         const float* __restrict__ window, int k, float c1, float c2, int tiles_x, int tiles,
                                                         double* __restrict__ scratch) {
    __shared__ float sx[IN * IN], sy[IN * IN];
    __shared__ float rf[5][IN * T];
    __shared__ float g[KM];
    __shared__ double part[4];
    const int tid = threadIdx.x;
    const long long wg = blockIdx.x, plane = wg / tiles;
    const int tile = (int)(wg - plane * tiles);
    const int b = (int)(plane / C_use), c = (int)(plane - (long long)b * C_use);
    const int ty0 = (tile / tiles_x) * T, tx0 = (tile % tiles_x) * T;
    const int in = T + k - 1;                                                       // rows and columns of the haloed tile
    const float* xp = x + ((long long)b * Cx + c) * H * W;
    const float* yp = y + ((long long)b * Cy + c) * H * W;
    if (tid < k) g[tid] = window[tid];
    for (int idx = tid; idx < in * in; idx += 256) {
        const int r = idx / in, cc = idx - r * in;
        const int gr = ty0 + r, gc = tx0 + cc;
        float a = 0.f, bv = 0.f;                                                    // (outside the image: feeds no window position that is counted)
        if (gr < H && gc < W) {
            a = conv_pred(xp[(long long)gr * W + gc], transform);
            bv = conv_target(yp[(long long)gr * W + gc], transform);
        }
        sx[r * IN + cc] = a;
        sy[r * IN + cc] = bv;
    }
    __syncthreads();
    for (int idx = tid; idx < in * T; idx += 256) {                                 // along the rows: cc + j <= T - 1 + k - 1 < IN
        const int r = idx / T, cc = idx - r * T;
        float m0 = 0.f, m1 = 0.f, m2 = 0.f, m3 = 0.f, m4 = 0.f;
        for (int j = 0; j < k; ++j) {
            const float a = sx[r * IN + cc + j], bv = sy[r * IN + cc + j], w = g[j];
            m0 += w * a; m1 += w * bv; m2 += w * (a * a); m3 += w * (bv * bv); m4 += w * (a * bv);
        }
        rf[0][idx] = m0; rf[1][idx] = m1; rf[2][idx] = m2; rf[3][idx] = m3; rf[4][idx] = m4;
    }
    __syncthreads();
    const int Ho = H - k + 1, Wo = W - k + 1;
    double ss = 0.0, sc = 0.0;
    for (int idx = tid; idx < T * T; idx += 256) {                                  // along the columns: r + i <= T - 1 + k - 1 < IN
        const int r = idx / T, cc = idx - r * T;
        if (ty0 + r >= Ho || tx0 + cc >= Wo) continue;
        float mx = 0.f, my = 0.f, exx = 0.f, eyy = 0.f, exy = 0.f;
        for (int i = 0; i < k; ++i) {
            const int o = (r + i) * T + cc;
            const float w = g[i];
            mx += w * rf[0][o]; my += w * rf[1][o]; exx += w * rf[2][o]; eyy += w * rf[3][o]; exy += w * rf[4][o];
        }
        const float mxx = mx * mx, myy = my * my, mxy = mx * my;
        const float vx = exx - mxx, vy = eyy - myy, vxy = exy - mxy;
        const float cs = (2.0f * vxy + c2) / (vx + vy + c2);
        const float s = ((2.0f * mxy + c1) / (mxx + myy + c1)) * cs;
        ss += (double)s;
        sc += (double)cs;
    }
    ss = block_sum_d(ss, part);
    sc = block_sum_d(sc, part);
    if (tid == 0) { scratch[2 * wg] = ss; scratch[2 * wg + 1] = sc; }
}

// image b: its C_use * tiles partials in index order, over the number of window positions
__global__ __launch_bounds__(256) void ssim_finish_kernel(const double* __restrict__ scratch, long long per_image, double count, double* __restrict__ ssim,
                                                          double* __restrict__ cs) {
    __shared__ double part[4];
    const double* s = scratch + 2 * per_image * blockIdx.x;
    double a = 0.0, b = 0.0;
    for (long long i = threadIdx.x; i < per_image; i += 256) { a += s[2 * i]; b += s[2 * i + 1]; }
    a = block_sum_d(a, part);
    b = block_sum_d(b, part);
    if (threadIdx.x == 0) { ssim[blockIdx.x] = a / count; cs[blockIdx.x] = b / count; }
}

// ---- 2 x 2 mean, stride 2, of both images (an odd last row / column is dropped) ---------------------------------------------------------------
__global__ __launch_bounds__(256) void avgpool2x2_pair_kernel(const float* __restrict__ x, const float* __restrict__ y, int Cx, int Cy, int C_use, int H, int W, int transform,
                                                              float* __restrict__ xo, float* __restrict__ yo, long long total) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int Ho = H >> 1, Wo = W >> 1;
    const long long plane = i / ((long long)Ho * Wo), rem = i - plane * Ho * Wo;
    const int oh = (int)(rem / Wo), ow = (int)(rem - (long long)oh * Wo);
    const long long b = plane / C_use, c = plane - b * C_use;
    const long long at = (long long)(2 * oh) * W + 2 * ow;                          // 2 oh + 1 < H and 2 ow + 1 < W
    const float* xp = x + (b * Cx + c) * H * W + at;
    const float* yp = y + (b * Cy + c) * H * W + at;
    xo[i] = ((conv_pred(xp[0], transform) + conv_pred(xp[1], transform)) + (conv_pred(xp[W], transform) + conv_pred(xp[W + 1], transform))) * 0.25f;
    yo[i] = ((conv_target(yp[0], transform) + conv_target(yp[1], transform)) + (conv_target(yp[W], transform) + conv_target(yp[W + 1], transform))) * 0.25f;
}

// ---- token histogram -------------------------------------------------------------------------------------------------------------------------------
template <typename Tok>
__global__ __launch_bounds__(256) void token_histogram_kernel(const Tok* __restrict__ tokens, long long n, int K, unsigned long long* __restrict__ hist, int* __restrict__ bad) {
    int nbad = 0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const long long v = (long long)tokens[i];
        if (v >= 0 && v < K) atomicAdd(hist + v, 1ULL);
        else ++nbad;
    }
    nbad = wave_sum_i(nbad);
    if ((threadIdx.x & 63) == 0 && nbad) atomicAdd(bad, nbad);
}

inline bool aligned(const void* p, uintptr_t a) { return (((uintptr_t)p) & (a - 1)) == 0; }
inline bool transform_ok(int t) { return t == FM_METRIC_RAW || t == FM_METRIC_DENORM || t == FM_METRIC_SIGMOID_PRED; }

// workgroups of the main launch of fm_metric_sums; 0: bad arguments
long long sums_parts(int B, int C_use, long long HW) {
    if (B <= 0 || C_use <= 0 || HW <= 0 || (double)B * C_use * (double)HW > 4.0e12) return 0;
    const long long parts = ((long long)B * C_use * HW + FM_METRIC_CHUNK - 1) / FM_METRIC_CHUNK;
    return parts <= 0x3fffffffLL ? parts : 0;
}

// tiles per plane of fm_ssim_scale (0: bad arguments); workgroups = B * C_use * tiles
long long ssim_tiles(int B, int C_use, int H, int W, int k, int* tiles_x) {
    if (B <= 0 || C_use <= 0 || k < 1 || k > KM || !(k & 1) || H < k || W < k) return 0;
    const long long tx = (W - k + 1 + T - 1) / T, ty = (H - k + 1 + T - 1) / T;
    if ((double)B * C_use * (double)H * (double)W > 4.0e12 || (double)B * C_use * (double)(tx * ty) > (double)0x3fffffff) return 0;
    if (tiles_x) *tiles_x = (int)tx;
    return tx * ty;
}

}  // namespace

extern "C" int fm_metric_sums_scratch(int B, int C_use, int64_t HW) {
    const long long parts = sums_parts(B, C_use, HW);
    FM_CHECK_ARG(parts > 0, "fm_metric_sums_scratch: bad shape (B=%d C_use=%d HW=%lld)", B, C_use, (long long)HW);
    return (int)(2 * parts);
}

extern "C" int fm_metric_sums(const void* pred, const void* target, int B, int Cp, int Ct, int C_use, int64_t HW, int transform, int iou, float threshold,
                              void* scratch, void* sums, void* counts, void* stream) {
    FM_CHECK_ARG(pred && target && scratch && sums && counts, "fm_metric_sums: null pointer");
    const long long parts = sums_parts(B, C_use, HW);
    FM_CHECK_ARG(parts > 0 && C_use <= Cp && C_use <= Ct && (double)B * (Cp > Ct ? Cp : Ct) * (double)HW <= 4.0e12,
                 "fm_metric_sums: bad shape (B=%d Cp=%d Ct=%d C_use=%d HW=%lld)", B, Cp, Ct, C_use, (long long)HW);
    FM_CHECK_ARG(transform_ok(transform), "fm_metric_sums: transform %d", transform);
    FM_CHECK_ARG(aligned(pred, 4) && aligned(target, 4) && aligned(scratch, 8) && aligned(sums, 8) && aligned(counts, 8), "fm_metric_sums: misaligned pointer");
    hipStream_t st = (hipStream_t)stream;
    const long long n = (long long)B * C_use * HW;
    hipLaunchKernelGGL(metric_sums_kernel, dim3((unsigned)parts), dim3(256), 0, st, (const float*)pred, (const float*)target, Cp, Ct, C_use, (long long)HW, n, transform,
                       iou ? 1 : 0, threshold, (double*)scratch, (unsigned long long*)counts);
    FM_CHECK_LAUNCH("fm_metric_sums");
    hipLaunchKernelGGL(metric_sums_finish_kernel, dim3(1), dim3(256), 0, st, (const double*)scratch, parts, n, (double*)sums, (long long*)counts);
    FM_CHECK_LAUNCH("fm_metric_sums (finish)");
    return 0;
}

extern "C" int fm_ssim_scale_scratch(int B, int C_use, int H, int W, int ksize) {
    const long long tiles = ssim_tiles(B, C_use, H, W, ksize, nullptr);
    FM_CHECK_ARG(tiles > 0, "fm_ssim_scale_scratch: bad shape (B=%d C_use=%d H=%d W=%d ksize=%d; ksize odd, <= %d, <= H and W)", B, C_use, H, W, ksize, KM);
    return (int)(2 * tiles * B * C_use);
}

extern "C" int fm_ssim_scale(const void* x, const void* y, int B, int Cx, int Cy, int C_use, int H, int W, int transform, const void* window, int ksize, float c1,
                             float c2, void* scratch, void* ssim, void* cs, void* stream) {
    FM_CHECK_ARG(x && y && window && scratch && ssim && cs, "fm_ssim_scale: null pointer");
    int tiles_x = 0;
    const long long tiles = ssim_tiles(B, C_use, H, W, ksize, &tiles_x);
    FM_CHECK_ARG(tiles > 0 && C_use <= Cx && C_use <= Cy && (double)B * (Cx > Cy ? Cx : Cy) * (double)H * (double)W <= 4.0e12,
                 "fm_ssim_scale: bad shape (B=%d Cx=%d Cy=%d C_use=%d H=%d W=%d ksize=%d; ksize odd, <= %d, <= H and W)", B, Cx, Cy, C_use, H, W, ksize, KM);
    FM_CHECK_ARG(transform_ok(transform), "fm_ssim_scale: transform %d", transform);
    FM_CHECK_ARG(aligned(x, 4) && aligned(y, 4) && aligned(window, 4) && aligned(scratch, 8) && aligned(ssim, 8) && aligned(cs, 8), "fm_ssim_scale: misaligned pointer");
    hipStream_t st = (hipStream_t)stream;
    const long long per_image = tiles * C_use;
    hipLaunchKernelGGL(ssim_scale_kernel, dim3((unsigned)(per_image * B)), dim3(256), 0, st, (const float*)x, (const float*)y, Cx, Cy, C_use, H, W, transform,
                       (const float*)window, ksize, c1, c2, tiles_x, (int)tiles, (double*)scratch);
    FM_CHECK_LAUNCH("fm_ssim_scale");
    const double count = (double)C_use * (double)(H - ksize + 1) * (double)(W - ksize + 1);
    hipLaunchKernelGGL(ssim_finish_kernel, dim3((unsigned)B), dim3(256), 0, st, (const double*)scratch, per_image, count, (double*)ssim, (double*)cs);
    FM_CHECK_LAUNCH("fm_ssim_scale (finish)");
    return 0;
}

extern "C" int fm_avgpool2x2_pair(const void* x, const void* y, int B, int Cx, int Cy, int C_use, int H, int W, int transform, void* xo, void* yo, void* stream) {
    FM_CHECK_ARG(x && y && xo && yo, "fm_avgpool2x2_pair: null pointer");
    FM_CHECK_ARG(B > 0 && C_use > 0 && C_use <= Cx && C_use <= Cy && H >= 2 && W >= 2 && (double)B * (Cx > Cy ? Cx : Cy) * (double)H * (double)W <= 4.0e12,
                 "fm_avgpool2x2_pair: bad shape (B=%d Cx=%d Cy=%d C_use=%d H=%d W=%d)", B, Cx, Cy, C_use, H, W);
    FM_CHECK_ARG(transform_ok(transform), "fm_avgpool2x2_pair: transform %d", transform);
    FM_CHECK_ARG(aligned(x, 4) && aligned(y, 4) && aligned(xo, 4) && aligned(yo, 4), "fm_avgpool2x2_pair: misaligned pointer");
    const long long total = (long long)B * C_use * (H >> 1) * (W >> 1), blocks = (total + 255) / 256;
    FM_CHECK_ARG(blocks <= 0x7fffffffLL, "fm_avgpool2x2_pair: too many elements");
    hipLaunchKernelGGL(avgpool2x2_pair_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const float*)x, (const float*)y, Cx, Cy, C_use, H, W, transform,
                       (float*)xo, (float*)yo, total);
    FM_CHECK_LAUNCH("fm_avgpool2x2_pair");
    return 0;
}

extern "C" int fm_token_histogram(const void* tokens, int elem_size, int64_t n, int K, void* hist, void* bad, void* stream) {
    FM_CHECK_ARG(tokens && hist && bad, "fm_token_histogram: null pointer");
    FM_CHECK_ARG(elem_size == 2 || elem_size == 4 || elem_size == 8, "fm_token_histogram: tokens of %d bytes (int16, int32 or int64)", elem_size);
    FM_CHECK_ARG(K > 0 && n > 0, "fm_token_histogram: K=%d, n=%lld", K, (long long)n);
    FM_CHECK_ARG(aligned(tokens, elem_size) && aligned(hist, 8) && aligned(bad, 4), "fm_token_histogram: misaligned pointer");
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(bad, 0, sizeof(int), st) != hipSuccess) { fm_set_error("fm_token_histogram: hipMemsetAsync failed"); return -2; }
    const long long want = (n + 255) / 256;
    const dim3 grid((unsigned)(want > 1024 ? 1024 : want)), blk(256);
    if (elem_size == 8) hipLaunchKernelGGL(token_histogram_kernel<long long>, grid, blk, 0, st, (const long long*)tokens, (long long)n, K, (unsigned long long*)hist, (int*)bad);
    else if (elem_size == 4) hipLaunchKernelGGL(token_histogram_kernel<int>, grid, blk, 0, st, (const int*)tokens, (long long)n, K, (unsigned long long*)hist, (int*)bad);
    else hipLaunchKernelGGL(token_histogram_kernel<short>, grid, blk, 0, st, (const short*)tokens, (long long)n, K, (unsigned long long*)hist, (int*)bad);
    FM_CHECK_LAUNCH("fm_token_histogram");
    return 0;
}
