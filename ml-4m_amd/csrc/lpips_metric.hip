// The kernels of the LPIPS (AlexNet) validation metric (include/fourm_hip.h, "LPIPS validation metric"; fourm/vq/percept_losses/lpips_alex.py):
//   fm_conv2d_stem_f32   an image stem: few input channels (1..4), a large kernel (up to 11 x 11) and a large stride (up to 4), read straight from
//                        NCHW pixels with an optional clamp and a per-channel affine in the gather; NHWC rows out.  AlexNet's first convolution.
//   fm_lpips_score       the metric's per-layer distance, forward only: unit-normalised features (sqrt(eps + sum a^2)), weighted squared
//                        difference, mean over the pixels, accumulated onto score (B).
// Everything fp32, no floating-point atomics, one summation order per output element: two calls give the same bits.
//
// The stem is the implicit GEMM of csrc/inception.hip (v_mfma_f32_32x32x2_f32: exact fp32, an fmaf chain over k) with another gather: a
// workgroup of 4 waves owns 64 output pixels x 64 output channels (128 x 32 for Cout <= 32: by Cout alone), a wave one 32 x 32 accumulator.  Per
// step of 32 k each thread gathers 4 consecutive k of 2 (4) pixels - bounds-checked against the image, clamped, scaled - and 4 k of 2 (1)
// weight rows into registers, then LDS; the next step's loads are in flight under this step's 16 MFMAs.  No im2col or space-to-depth copy
// goes to memory.
// What bounds it: the gather, not the matrix pipe.  Measured (tools/time_lpips_metric.py, profiles/lpips_metric_bench.json, one MI355X):
// AlexNet's stem on 64 images of 224 x 224 (9.0 GFLOP, 38.5 MB in, 49.6 MB out) takes 0.198 ms per launch = 45.5 TFLOP/s, 29 % of the
// 157 TFLOP/s f32 MFMA rate and 3.5 x the 57 us that rate would allow; HBM traffic is 0.45 TB/s, far from its limit.  Per step of 32 k a
// wave issues 16 MFMAs of 64 cycles (1024 cycles) and every thread 16 four-byte global loads, each with its own (c, ky, kx) address, a
// clamp and an fmaf: with Cin = 3 the 4 consecutive k of a thread lie in 3 different channel planes, and the 8 pixels a wave covers per
// load are `stride` floats apart, so one load instruction touches dozens of cache lines where a row-contiguous layout would touch one.
// No counters were taken: that the cache-line rate of these loads, and not LDS or the two barriers per step, is what the MFMAs wait for
// is a reading of these counts, not a measurement.  What was measured: taking the 64-bit index arithmetic and the two integer divisions
// per step out of the gather (32-bit offsets, a tap state advanced by 32 k) moved a launch from 0.205 to 0.198 ms, so the VALU work of the
// addresses is not the bound.  k is padded from K to the next multiple of 32 (AlexNet: 363 -> 384, 5.8 % idle MFMA
// columns).  Not done: staging the image rows a tile needs into LDS with row-contiguous 16-byte loads and gathering from there.
#include <math.h>

#include "common.h"
#include "fourm_hip.h"

namespace {

constexpr int ST_KS = 32;              // k per staging step
constexpr int ST_LDT = ST_KS + 1;      // LDS row stride 33 floats: the 32 lanes of a half-wave hit 32 banks (the tile layout of csrc/inception.hip)

struct StemP {
    const float* img; const float* w; const float* bias; const float* mul; const float* add; float* out;
    int B, Cin, H, W, Cout, KH, KW, stride, pad, ldw, ldo, relu, clamp, Ho, Wo, K, M, ntn;
    float lo, hi;
};

template <int WM, int WN>
__global__ __launch_bounds__(256) void conv2d_stem_f32_kernel(const StemP p) {
    constexpr int TM = 32 * WM, TN = 32 * WN, KS = ST_KS, LDT = ST_LDT, PA = TM / 32, PW = TN / 32;
    __shared__ float As[TM * LDT], Ws[TN * LDT];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave / WN, wn = wave - wm * WN;
    const int mt = blockIdx.x / p.ntn, nt = blockIdx.x - mt * p.ntn;
    const int m0 = mt * TM, n0 = nt * TN;                              // m0 < M < 2^31, n0 < Cout
    const int lr = threadIdx.x >> 3, lc = (threadIdx.x & 7) * 4;
    int iy0[PA], ix0[PA], base[PA];
    const float* xb[PA];
    bool rv[PA];
    const int HoWo = p.Ho * p.Wo;
    const int plane = p.H * p.W;                                       // 32-bit offsets inside an image: Cin (H + 2 pad) (W + 2 pad) < 2^31 (checked by the host)
#pragma unroll
    for (int q = 0; q < PA; ++q) {
        const int m = m0 + lr + 32 * q;
        rv[q] = m < p.M;
        const int mm = rv[q] ? m : 0;
        const int b = mm / HoWo, rem = mm - b * HoWo, oy = rem / p.Wo, ox = rem - oy * p.Wo;
        iy0[q] = oy * p.stride - p.pad;
        ix0[q] = ox * p.stride - p.pad;
        base[q] = iy0[q] * p.W + ix0[q];
        xb[q] = p.img + (size_t)b * p.Cin * (size_t)plane;
    }
    const float* wp[PW];
    bool wv[PW];
#pragma unroll
    for (int q = 0; q < PW; ++q) {
        const int n = n0 + lr + 32 * q;
        wv[q] = n < p.Cout;
        wp[q] = p.w + (size_t)(wv[q] ? n : 0) * p.ldw;
    }
    float areg[PA][4], wreg[PW][4];
    // (c0, ky0, kx0) of this thread's first k of the step, found by division once and then advanced by 32 k per step
    int c0, ky0, kx0;
    {
        const int tap = lc / p.Cin;
        c0 = lc - tap * p.Cin;
        ky0 = tap / p.KW;
        kx0 = tap - ky0 * p.KW;
    }
    const int adv_t = KS / p.Cin, adv_c = KS - adv_t * p.Cin;
    auto advance = [&]() {
        int t = adv_t;
        c0 += adv_c;
        if (c0 >= p.Cin) { c0 -= p.Cin; ++t; }
        kx0 += t;
        while (kx0 >= p.KW) { kx0 -= p.KW; ++ky0; }
    };
    auto load = [&](int k0) {
        const int k = k0 + lc;
        int c = c0, ky = ky0, kx = kx0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool kin = k + j < p.K;                              // (c < Cin always; ky < KH follows from kin)
            // the offset comes from the same (c, ky, kx) as the bounds checks below: base + koff = c plane + iy W + ix
            const int koff = (int)((unsigned)c * (unsigned)plane + (unsigned)ky * (unsigned)p.W + (unsigned)kx);
            const float mc = (kin && p.mul) ? p.mul[c] : 1.f, ac = (kin && p.mul) ? p.add[c] : 0.f;
#pragma unroll
            for (int q = 0; q < PA; ++q) {
                const int iy = iy0[q] + ky, ix = ix0[q] + kx;
                const bool ok = rv[q] && kin && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
                float s = 0.f;                                         // zero padding applies to s: outside the image 0, not add[c]
                if (ok) {
                    float v = xb[q][base[q] + koff];
                    if (p.clamp) v = fminf(fmaxf(v, p.lo), p.hi);
                    s = p.mul ? __fmaf_rn(v, mc, ac) : v;
                }
                areg[q][j] = s;
            }
#pragma unroll
            for (int q = 0; q < PW; ++q) wreg[q][j] = (wv[q] && kin) ? wp[q][k + j] : 0.f;
            if (++c == p.Cin) {
                c = 0;
                if (++kx == p.KW) { kx = 0; ++ky; }
            }
        }
    };
    auto stash = [&]() {
#pragma unroll
        for (int q = 0; q < PA; ++q) {
            float* d = As + (lr + 32 * q) * LDT + lc;
            d[0] = areg[q][0]; d[1] = areg[q][1]; d[2] = areg[q][2]; d[3] = areg[q][3];
        }
#pragma unroll
        for (int q = 0; q < PW; ++q) {
            float* d = Ws + (lr + 32 * q) * LDT + lc;
            d[0] = wreg[q][0]; d[1] = wreg[q][1]; d[2] = wreg[q][2]; d[3] = wreg[q][3];
        }
    };
    f32x16_t acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    load(0);
    advance();
    for (int k0 = 0; k0 < p.K; k0 += KS) {
        __syncthreads();                                               // the previous step's readers are done
        stash();
        __syncthreads();
        if (k0 + KS < p.K) {                                           // next step in flight under the MFMAs
            load(k0 + KS);
            advance();
        }
        const float* ab = As + (wm * 32 + (lane & 31)) * LDT + (lane >> 5);
        const float* bb = Ws + (wn * 32 + (lane & 31)) * LDT + (lane >> 5);
#pragma unroll
        for (int kk = 0; kk < KS; kk += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ab[kk], bb[kk], acc, 0, 0, 0);
    }
    // accumulator map: column (lane & 31) = output channel, register 4 g + e = output pixel 8 g + 4 (lane >> 5) + e of the wave's 32
    const int n = n0 + wn * 32 + (lane & 31);
    if (n >= p.Cout) return;
    const float bias = p.bias ? p.bias[n] : 0.f;
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int m = m0 + wm * 32 + 8 * g + 4 * (lane >> 5) + e;
            if (m < p.M) {
                float v = bias + acc[4 * g + e];
                if (p.relu) v = v > 0.f ? v : 0.f;
                p.out[(size_t)m * p.ldo + n] = v;
            }
        }
}

// ---- per-layer distance ----------------------------------------------------------------------------------------------------------------
// One workgroup (4 wavefronts) per (sample, chunk of FM_LPIPS_SCORE_CHUNK pixels).  LP lanes share a pixel (16 for C <= 64, 32 for C <= 128,
// else 64), a lane holds channels [4 (l + LP j), + 4) of it, j < J; a wavefront takes 64 / LP pixels at a time.  Partial sums: a lane
// group's pixels in order, the groups of a wavefront by a fixed shuffle tree, then the 4 wavefronts in order -> scratch[b * chunks + chunk].
// a and b go through the same instructions, the difference enters as (w d) d: swapping them changes no bit, and a against itself is 0.
template <int LP>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
    for (int o = LP / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <int LP>
__global__ __launch_bounds__(256) void lpips_score_kernel(const float* __restrict__ a, int lda, const float* __restrict__ b, int ldb, const float* __restrict__ w,
                                                          int P, int C, int chunks, float eps, float* __restrict__ scratch) {
    constexpr int PPW = 64 / LP, J = LP == 64 ? 2 : 1, CH = FM_LPIPS_SCORE_CHUNK;
    __shared__ float part[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane / LP, sl = lane % LP;
    const int smp = blockIdx.x / chunks, chunk = blockIdx.x - smp * chunks;
    float wv[J][4];
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const int c = 4 * (sl + LP * j);
#pragma unroll
        for (int e = 0; e < 4; ++e) wv[j][e] = c < C ? w[c + e] : 0.f;
    }
    float sum = 0.f;
    for (int i0 = wave * PPW; i0 < CH; i0 += 4 * PPW) {
        if (chunk * CH + i0 >= P) break;                                // (uniform over the wavefront)
        const int px = chunk * CH + i0 + sub;
        const bool valid = px < P;
        const long long row = (long long)smp * P + (valid ? px : P - 1);   // (a dead lane group re-reads the last pixel and contributes nothing)
        float x[J][4], y[J][4];
        float sx = 0.f, sy = 0.f;
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const int c = 4 * (sl + LP * j);
            float4 vx = make_float4(0.f, 0.f, 0.f, 0.f), vy = vx;
            if (c < C) {
                vx = *(const float4*)(a + row * lda + c);
                vy = *(const float4*)(b + row * ldb + c);
            }
            x[j][0] = vx.x; x[j][1] = vx.y; x[j][2] = vx.z; x[j][3] = vx.w;
            y[j][0] = vy.x; y[j][1] = vy.y; y[j][2] = vy.z; y[j][3] = vy.w;
#pragma unroll
            for (int e = 0; e < 4; ++e) { sx = __fmaf_rn(x[j][e], x[j][e], sx); sy = __fmaf_rn(y[j][e], y[j][e], sy); }
        }
        sx = group_sum<LP>(sx); sy = group_sum<LP>(sy);
        const float nx = sqrtf(eps + sx), ny = sqrtf(eps + sy);
        float val = 0.f;
#pragma unroll
        for (int j = 0; j < J; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float diff = x[j][e] / nx - y[j][e] / ny;
                const float wd = wv[j][e] * diff;
                val = __fmaf_rn(wd, diff, val);
            }
        val = group_sum<LP>(val);
        sum += valid ? val : 0.f;
    }
#pragma unroll
    for (int o = LP; o < 64; o <<= 1) sum += __shfl_xor(sum, o, 64);    // the lane groups of this wavefront
    if (lane == 0) part[wave] = sum;
    __syncthreads();
    if (threadIdx.x == 0) scratch[blockIdx.x] = ((part[0] + part[1]) + part[2]) + part[3];
}

// score[b] += (the chunks' partial sums, added in chunk order) / P: one wavefront per sample, lane l takes chunks l, l + 64, ... in order
__global__ __launch_bounds__(64) void lpips_score_sum_kernel(const float* __restrict__ scratch, int chunks, int P, float* __restrict__ score) {
    const int b = blockIdx.x, lane = threadIdx.x;
    float s = 0.f;
    for (int i = lane; i < chunks; i += 64) s += scratch[(long long)b * chunks + i];
    s = wave_sum(s);
    if (lane == 0) score[b] += s / (float)P;
}

inline bool aligned(const void* p, int a) { return ((uintptr_t)p & (uintptr_t)(a - 1)) == 0; }

template <int WM, int WN>
void launch_stem(const StemP& p, hipStream_t s) {
    const long long mtiles = ((long long)p.M + 32 * WM - 1) / (32 * WM);
    hipLaunchKernelGGL((conv2d_stem_f32_kernel<WM, WN>), dim3((unsigned)(mtiles * p.ntn)), dim3(256), 0, s, p);
}

}  // namespace

extern "C" int fm_conv2d_stem_f32(const fm_conv2d_stem_args* a, void* stream) {
    FM_CHECK_ARG(a, "fm_conv2d_stem_f32: null args");
    FM_CHECK_ARG(a->img && a->w && a->out, "fm_conv2d_stem_f32: null pointer (img, w and out are required; bias may be NULL = zeros)");
    FM_CHECK_ARG((a->mul == nullptr) == (a->add == nullptr), "fm_conv2d_stem_f32: mul and add are given together, or both NULL (the identity)");
    FM_CHECK_ARG(aligned(a->img, 4) && aligned(a->w, 4) && aligned(a->out, 4) && aligned(a->bias, 4) && aligned(a->mul, 4) && aligned(a->add, 4),
                 "fm_conv2d_stem_f32: pointers must be 4-byte aligned");
    FM_CHECK_ARG(a->Cin >= 1 && a->Cin <= FM_STEM_MAX_CIN && a->Cout >= 1 && a->Cout <= FM_STEM_MAX_COUT, "fm_conv2d_stem_f32: Cin=%d Cout=%d unsupported (Cin 1..%d, Cout 1..%d)",
                 a->Cin, a->Cout, FM_STEM_MAX_CIN, FM_STEM_MAX_COUT);
    FM_CHECK_ARG(a->KH >= 1 && a->KH <= FM_STEM_MAX_K && a->KW >= 1 && a->KW <= FM_STEM_MAX_K, "fm_conv2d_stem_f32: kernel %d x %d unsupported (1..%d each)", a->KH, a->KW, FM_STEM_MAX_K);
    FM_CHECK_ARG(a->stride >= 1 && a->stride <= FM_STEM_MAX_STRIDE, "fm_conv2d_stem_f32: stride=%d unsupported (1..%d)", a->stride, FM_STEM_MAX_STRIDE);
    FM_CHECK_ARG(a->pad >= 0 && a->pad <= FM_STEM_MAX_PAD, "fm_conv2d_stem_f32: padding %d unsupported (0..%d)", a->pad, FM_STEM_MAX_PAD);
    FM_CHECK_ARG(a->B >= 1 && a->H >= 1 && a->W >= 1, "fm_conv2d_stem_f32: bad shape (B=%d H=%d W=%d)", a->B, a->H, a->W);
    FM_CHECK_ARG((long long)a->H + 2 * a->pad >= a->KH && (long long)a->W + 2 * a->pad >= a->KW, "fm_conv2d_stem_f32: the %d x %d kernel does not fit the padded %d x %d image",
                 a->KH, a->KW, a->H + 2 * a->pad, a->W + 2 * a->pad);
    const int K = a->KH * a->KW * a->Cin;
    FM_CHECK_ARG(a->ldw >= K && a->ldo >= a->Cout, "fm_conv2d_stem_f32: row strides too small (ldw=%d >= K=%d, ldo=%d >= Cout=%d)", a->ldw, K, a->ldo, a->Cout);
    FM_CHECK_ARG((long long)a->Cin * (a->H + 2ll * a->pad) * (a->W + 2ll * a->pad) < (1ll << 31) && (long long)a->B * a->Cin * a->H * a->W < (1ll << 40),
                 "fm_conv2d_stem_f32: images too large (Cin (H + 2 pad) (W + 2 pad) < 2^31 per image): convolve in blocks");
    StemP p;
    p.img = (const float*)a->img; p.w = (const float*)a->w; p.bias = (const float*)a->bias; p.mul = (const float*)a->mul; p.add = (const float*)a->add; p.out = (float*)a->out;
    p.B = a->B; p.Cin = a->Cin; p.H = a->H; p.W = a->W; p.Cout = a->Cout; p.KH = a->KH; p.KW = a->KW; p.stride = a->stride; p.pad = a->pad;
    p.ldw = a->ldw; p.ldo = a->ldo; p.relu = a->relu ? 1 : 0; p.clamp = a->clamp ? 1 : 0; p.lo = a->lo; p.hi = a->hi;
    p.Ho = (a->H + 2 * a->pad - a->KH) / a->stride + 1;
    p.Wo = (a->W + 2 * a->pad - a->KW) / a->stride + 1;
    p.K = K;
    const long long M = (long long)a->B * p.Ho * p.Wo;
    FM_CHECK_ARG(M < (1ll << 31) - 256, "fm_conv2d_stem_f32: more than 2^31 output rows (B=%d): convolve in blocks", a->B);
    p.M = (int)M;
    const bool narrow = a->Cout <= 32;                                 // by Cout alone: never by B
    p.ntn = narrow ? 1 : (a->Cout + 63) / 64;
    if (narrow) launch_stem<4, 1>(p, (hipStream_t)stream);
    else launch_stem<2, 2>(p, (hipStream_t)stream);
    FM_CHECK_LAUNCH("fm_conv2d_stem_f32");
    return 0;
}

extern "C" int fm_lpips_score_scratch(int B, int P) {
    FM_CHECK_ARG(B >= 1 && P >= 1, "fm_lpips_score_scratch: bad shape B=%d P=%d", B, P);
    const long long n = (long long)B * ((P + FM_LPIPS_SCORE_CHUNK - 1) / FM_LPIPS_SCORE_CHUNK);
    FM_CHECK_ARG(n < (1ll << 31) && (long long)B * P < (1ll << 31), "fm_lpips_score_scratch: B=%d P=%d: too many pixels, score in blocks", B, P);
    return (int)n;
}

extern "C" int fm_lpips_score(const void* a, int lda, const void* b, int ldb, const void* w, int B, int P, int C, float eps, void* score, void* scratch, void* stream) {
    FM_CHECK_ARG(a && b && w && score && scratch, "fm_lpips_score: null pointer");
    FM_CHECK_ARG(B >= 1 && P >= 1 && C >= 4 && C % 4 == 0 && C <= FM_LPIPS_SCORE_MAX_C, "fm_lpips_score: bad shape B=%d P=%d C=%d (C %% 4 == 0, C <= %d)", B, P, C, FM_LPIPS_SCORE_MAX_C);
    FM_CHECK_ARG(lda >= C && ldb >= C && lda % 4 == 0 && ldb % 4 == 0, "fm_lpips_score: leading dimensions %d / %d (>= C, %% 4 == 0)", lda, ldb);
    FM_CHECK_ARG(aligned(a, 16) && aligned(b, 16) && aligned(w, 16) && aligned(score, 16) && aligned(scratch, 16), "fm_lpips_score: pointers must be 16-byte aligned");
    FM_CHECK_ARG(eps >= 0.f, "fm_lpips_score: eps=%g (>= 0 expected)", (double)eps);
    const int n = fm_lpips_score_scratch(B, P);
    if (n < 0) return -1;
    const int chunks = n / B;
    hipStream_t st = (hipStream_t)stream;
#define FM_LPIPS_SCORE(LP) hipLaunchKernelGGL((lpips_score_kernel<LP>), dim3((unsigned)n), dim3(256), 0, st, (const float*)a, lda, (const float*)b, ldb, (const float*)w, P, C, chunks, eps, (float*)scratch)
    if (C <= 64) FM_LPIPS_SCORE(16);
    else if (C <= 128) FM_LPIPS_SCORE(32);
    else FM_LPIPS_SCORE(64);
#undef FM_LPIPS_SCORE
    FM_CHECK_LAUNCH("fm_lpips_score");
    hipLaunchKernelGGL(lpips_score_sum_kernel, dim3((unsigned)B), dim3(64), 0, st, (const float*)scratch, chunks, P, (float*)score);
    FM_CHECK_LAUNCH("fm_lpips_score (sum)");
    return 0;
}
