// The kernels of the FID / Inception-score tower (include/fourm_hip.h, "Inception tower"; fourm/utils/inception): everything fp32, NHWC rows.
//   fm_conv2d_nhwc_f32       general implicit-GEMM convolution on v_mfma_f32_32x32x2_f32 (KH, KW in 1..7, stride 1 | 2, zero padding 0..3,
//                            any Cin / Cout, bias, optional ReLU, channel-slice output).  The 1 x 1 convolutions and the final fc run here too.
//   fm_pool2d_nhwc_f32       the four pools of the graph.
//   fm_inception_preprocess  uint8 / [0, 1] images (B, 3, H, W) -> TF1-style bilinear 299 x 299 -> (v - 128) / 128 as NHWC rows.
//   fm_feature_moments       float64 sum, outer product and count of feature rows.
// No floating-point atomics anywhere: every output element is written once by one thread, in a summation order that is a function of the
// element alone.  A convolution output is ONE fp32 accumulation chain over k = (ky KW + kx) Cin + c ascending (the MFMA is an fmaf chain over
// k, MI355X_MICROARCH "Matrix cores"), whatever tile the element falls into - so it does not depend on the batch or the position in it.
#include <math.h>

#include "common.h"
#include "fourm_hip.h"

namespace {

constexpr int CV_KS = 32;              // k per staging step
constexpr int CV_LDT = CV_KS + 1;      // LDS row stride 33 floats (the tile layout of csrc/knn.hip: the 32 lanes of a half-wave hit 32 banks)

struct ConvP {
    const float* x; const float* w; const float* bias; float* out;
    int B, H, W, Cin, Cout, KH, KW, stride, ph, pw, ldx, ldw, ldo, relu, Ho, Wo, K, M, ntn;
};

// A workgroup of WM x WN waves owns 32 WM output pixels x 32 WN output channels; a wave one 32 x 32 accumulator (the 32x32x2 MFMA issues
// every 64 cycles and its dependent latency is 64 cycles: one chain per wave keeps the pipe full).  Per step of 32 k the activation tile is
// GATHERED into LDS with bounds checks (thread -> row lr + 32 p, 4 consecutive k at lc): no im2col row ever goes to memory.  VEC: Cin, ldx and
// ldw are multiples of 4 and the pointers 16-byte aligned, so 4 consecutive k are one tap and one float4.  Both forms stage the same values.
template <int WM, int WN, bool VEC>
__global__ __launch_bounds__(256) void conv2d_nhwc_f32_kernel(const ConvP p) {
    constexpr int TM = 32 * WM, TN = 32 * WN, KS = CV_KS, LDT = CV_LDT, PA = TM / 32, PW = TN / 32;
    __shared__ float As[TM * LDT], Ws[TN * LDT];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave / WN, wn = wave - wm * WN;
    const int mt = blockIdx.x / p.ntn, nt = blockIdx.x - mt * p.ntn;
    const int m0 = mt * TM, n0 = nt * TN;                              // m0 < M < 2^31, n0 < Cout
    const int lr = threadIdx.x >> 3, lc = (threadIdx.x & 7) * 4;
    int iy0[PA], ix0[PA];
    const float* xb[PA];
    bool rv[PA];
    const int HoWo = p.Ho * p.Wo;
#pragma unroll
    for (int q = 0; q < PA; ++q) {
        const int m = m0 + lr + 32 * q;
        rv[q] = m < p.M;
        const int mm = rv[q] ? m : 0;
        const int b = mm / HoWo, rem = mm - b * HoWo, oy = rem / p.Wo, ox = rem - oy * p.Wo;
        iy0[q] = oy * p.stride - p.ph;
        ix0[q] = ox * p.stride - p.pw;
        xb[q] = p.x + (size_t)b * p.H * p.W * p.ldx;
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
    auto load = [&](int k0) {
        const int k = k0 + lc;
        int tap = k / p.Cin, c = k - tap * p.Cin, ky = tap / p.KW, kx = tap - ky * p.KW;
        if constexpr (VEC) {
            const bool kin = k < p.K;                                  // K % 4 == 0: the 4 are inside or outside together, and in one tap
#pragma unroll
            for (int q = 0; q < PA; ++q) {
                const int iy = iy0[q] + ky, ix = ix0[q] + kx;
                const bool ok = rv[q] && kin && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
                const float4 v = ok ? *(const float4*)(xb[q] + ((size_t)iy * p.W + ix) * p.ldx + c) : make_float4(0.f, 0.f, 0.f, 0.f);
                areg[q][0] = v.x; areg[q][1] = v.y; areg[q][2] = v.z; areg[q][3] = v.w;
            }
#pragma unroll
            for (int q = 0; q < PW; ++q) {
                const float4 v = (wv[q] && kin) ? *(const float4*)(wp[q] + k) : make_float4(0.f, 0.f, 0.f, 0.f);
                wreg[q][0] = v.x; wreg[q][1] = v.y; wreg[q][2] = v.z; wreg[q][3] = v.w;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool kin = k + j < p.K;
#pragma unroll
                for (int q = 0; q < PA; ++q) {
                    const int iy = iy0[q] + ky, ix = ix0[q] + kx;
                    const bool ok = rv[q] && kin && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
                    areg[q][j] = ok ? xb[q][((size_t)iy * p.W + ix) * p.ldx + c] : 0.f;
                }
#pragma unroll
                for (int q = 0; q < PW; ++q) wreg[q][j] = (wv[q] && kin) ? wp[q][k + j] : 0.f;
                if (++c == p.Cin) {
                    c = 0;
                    if (++kx == p.KW) { kx = 0; ++ky; }
                }
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
    for (int k0 = 0; k0 < p.K; k0 += KS) {
        __syncthreads();                                               // the previous step's readers are done
        stash();
        __syncthreads();
        if (k0 + KS < p.K) load(k0 + KS);                              // next step in flight under the MFMAs
        const float* ab = As + (wm * 32 + (lane & 31)) * LDT + (lane >> 5);
        const float* bb = Ws + (wn * 32 + (lane & 31)) * LDT + (lane >> 5);
#pragma unroll
        for (int kk = 0; kk < KS; kk += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ab[kk], bb[kk], acc, 0, 0, 0);
    }
    // accumulator map: column (lane & 31) = output channel, register 4 g + e = output pixel 8 g + 4 (lane >> 5) + e of the wave's 32: a
    // store instruction writes 32 consecutive channels of two rows
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

// 3 x 3 windows: a thread per (output pixel, channel), channels fastest.  The taps are visited ky, kx ascending.
__global__ __launch_bounds__(256) void pool3x3_kernel(const float* __restrict__ x, int ldx, float* __restrict__ out, int ldo, int H, int W, int C, int Ho, int Wo,
                                                      int stride, int pad, int avg, long long total) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int c = (int)(idx % C);
    const long long pix = idx / C;
    const int ox = (int)(pix % Wo);
    const long long t = pix / Wo;
    const int oy = (int)(t % Ho);
    const long long b = t / Ho;
    float s = 0.f, m = -INFINITY;
    int cnt = 0;
    for (int ky = 0; ky < 3; ++ky) {
        const int iy = oy * stride - pad + ky;
        if ((unsigned)iy >= (unsigned)H) continue;
        for (int kx = 0; kx < 3; ++kx) {
            const int ix = ox * stride - pad + kx;
            if ((unsigned)ix >= (unsigned)W) continue;
            const float v = x[(size_t)((b * H + iy) * W + ix) * ldx + c];
            s += v;
            m = fmaxf(m, v);
            ++cnt;
        }
    }
    out[(size_t)pix * ldo + c] = avg ? s * (1.0f / (float)cnt) : m;
}

// mean over the H W rows of an image in row order: a thread per (image, channel)
__global__ __launch_bounds__(256) void global_avg_kernel(const float* __restrict__ x, int ldx, float* __restrict__ out, int ldo, int HW, int C, long long total) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int c = (int)(idx % C);
    const long long b = idx / C;
    const float* xp = x + (size_t)b * HW * ldx + c;
    float s = 0.f;
    for (int r = 0; r < HW; ++r) s += xp[(size_t)r * ldx];
    out[(size_t)b * ldo + c] = s / (float)HW;
}

// a thread per output element (b, oy, ox, c), c fastest.  idx (4, 299) int32: y0, y1, x0, x1;  wt (2, 299) f32: wy, wx.  The table indices are
// clamped to the image, so a wrong table cannot make the kernel read outside the input.
template <bool F32>
__global__ __launch_bounds__(256) void inception_preprocess_kernel(const void* __restrict__ in, int H, int W, const int* __restrict__ idx,
                                                                  const float* __restrict__ wt, float* __restrict__ out, long long total) {
    constexpr int S = FM_INCEPTION_SIZE;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % 3);
    long long t = i / 3;
    const int ox = (int)(t % S);
    t /= S;
    const int oy = (int)(t % S);
    const long long b = t / S;
    auto clampi = [](int v, int hi) { return v < 0 ? 0 : v > hi ? hi : v; };
    const int y0 = clampi(idx[oy], H - 1), y1 = clampi(idx[S + oy], H - 1), x0 = clampi(idx[2 * S + ox], W - 1), x1 = clampi(idx[3 * S + ox], W - 1);
    const float wy = wt[oy], wx = wt[S + ox];
    const size_t plane = (size_t)(b * 3 + c) * H * W;
    auto px = [&](int y, int xx) -> float {
        const size_t o = plane + (size_t)y * W + xx;
        if constexpr (F32) {
            const float v = truncf(255.0f * ((const float*)in)[o]);    // torchmetrics' (imgs * 255).byte(); the clamp is ours (NaN -> 0)
            return fminf(fmaxf(v, 0.f), 255.f);
        } else {
            return (float)((const uint8_t*)in)[o];
        }
    };
    const float tl = px(y0, x0), tr = px(y0, x1), bl = px(y1, x0), br = px(y1, x1);
    const float top = __fmaf_rn(tr - tl, wx, tl), bot = __fmaf_rn(br - bl, wx, bl);
    const float v = __fmaf_rn(bot - top, wy, top);
    out[i] = (v - 128.0f) / 128.0f;
}

// outer (d, d) += X^T X in float64: a workgroup owns 64 x 64 elements, a thread 4 x 4; the rows are added in ascending order (the product of
// two floats is exact in double, so fma(x_i, x_j, acc) is the sequential float64 sum bit for bit)
__global__ __launch_bounds__(256) void moments_outer_kernel(const float* __restrict__ f, int ld, int n, int d, double* __restrict__ outer) {
    constexpr int T = 64, RC = 16;
    __shared__ float Xi[RC][T], Xj[RC][T];
    const int i0 = blockIdx.y * T, j0 = blockIdx.x * T;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    double acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int i = i0 + ty * 4 + a, j = j0 + tx * 4 + b;
            acc[a][b] = (i < d && j < d) ? outer[(size_t)i * d + j] : 0.0;
        }
    for (int r0 = 0; r0 < n; r0 += RC) {
        __syncthreads();
        for (int e = threadIdx.x; e < RC * T; e += 256) {
            const int r = e / T, col = e - r * T;
            const bool rin = r0 + r < n;
            Xi[r][col] = (rin && i0 + col < d) ? f[(size_t)(r0 + r) * ld + i0 + col] : 0.f;
            Xj[r][col] = (rin && j0 + col < d) ? f[(size_t)(r0 + r) * ld + j0 + col] : 0.f;
        }
        __syncthreads();
        const int rows = n - r0 < RC ? n - r0 : RC;
        for (int r = 0; r < rows; ++r) {
            double xi[4], xj[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) { xi[a] = (double)Xi[r][ty * 4 + a]; xj[a] = (double)Xj[r][tx * 4 + a]; }
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) acc[a][b] = fma(xi[a], xj[b], acc[a][b]);
        }
    }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int i = i0 + ty * 4 + a, j = j0 + tx * 4 + b;
            if (i < d && j < d) outer[(size_t)i * d + j] = acc[a][b];
        }
}

// sum (d) += column sums in float64, rows ascending, a thread per column; thread 0 adds n to the count
__global__ __launch_bounds__(256) void moments_sum_kernel(const float* __restrict__ f, int ld, int n, int d, double* __restrict__ sum, long long* __restrict__ count) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j == 0) *count += n;
    if (j >= d) return;
    double s = sum[j];
    for (int r = 0; r < n; ++r) s += (double)f[(size_t)r * ld + j];
    sum[j] = s;
}

inline bool aligned(const void* p, int a) { return ((uintptr_t)p & (uintptr_t)(a - 1)) == 0; }

template <int WM, int WN>
void launch_conv(const ConvP& p, bool vec, hipStream_t s) {
    const long long mtiles = ((long long)p.M + 32 * WM - 1) / (32 * WM);
    const dim3 grid((unsigned)(mtiles * p.ntn));
    if (vec) hipLaunchKernelGGL((conv2d_nhwc_f32_kernel<WM, WN, true>), grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL((conv2d_nhwc_f32_kernel<WM, WN, false>), grid, dim3(256), 0, s, p);
}

}  // namespace

extern "C" int fm_conv2d_nhwc_f32(const fm_conv2d_args* a, void* stream) {
    FM_CHECK_ARG(a, "fm_conv2d_nhwc_f32: null args");
    FM_CHECK_ARG(a->x && a->w && a->out, "fm_conv2d_nhwc_f32: null pointer (x, w and out are required; bias may be NULL = zeros)");
    FM_CHECK_ARG(aligned(a->x, 4) && aligned(a->w, 4) && aligned(a->out, 4) && aligned(a->bias, 4), "fm_conv2d_nhwc_f32: pointers must be 4-byte aligned");
    FM_CHECK_ARG(a->KH >= 1 && a->KH <= FM_CONV2D_MAX_K && a->KW >= 1 && a->KW <= FM_CONV2D_MAX_K, "fm_conv2d_nhwc_f32: kernel %d x %d unsupported (1..%d each)", a->KH, a->KW, FM_CONV2D_MAX_K);
    FM_CHECK_ARG(a->stride == 1 || a->stride == 2, "fm_conv2d_nhwc_f32: stride=%d unsupported (1 | 2)", a->stride);
    FM_CHECK_ARG(a->pad_h >= 0 && a->pad_h <= FM_CONV2D_MAX_PAD && a->pad_w >= 0 && a->pad_w <= FM_CONV2D_MAX_PAD, "fm_conv2d_nhwc_f32: padding (%d, %d) unsupported (0..%d each)", a->pad_h, a->pad_w, FM_CONV2D_MAX_PAD);
    FM_CHECK_ARG(a->B >= 1 && a->H >= 1 && a->W >= 1 && a->Cin >= 1 && a->Cout >= 1, "fm_conv2d_nhwc_f32: bad shape (B=%d H=%d W=%d Cin=%d Cout=%d)", a->B, a->H, a->W, a->Cin, a->Cout);
    FM_CHECK_ARG(a->H + 2 * a->pad_h >= a->KH && a->W + 2 * a->pad_w >= a->KW, "fm_conv2d_nhwc_f32: the %d x %d kernel does not fit the padded %d x %d map", a->KH, a->KW, a->H + 2 * a->pad_h, a->W + 2 * a->pad_w);
    const long long K = (long long)a->KH * a->KW * a->Cin;
    FM_CHECK_ARG(K < (1ll << 30), "fm_conv2d_nhwc_f32: KH KW Cin = %lld too large", K);
    FM_CHECK_ARG(a->ldx >= a->Cin && a->ldw >= K && a->ldo >= a->Cout, "fm_conv2d_nhwc_f32: row strides too small (ldx=%d >= Cin=%d, ldw=%d >= K=%lld, ldo=%d >= Cout=%d)", a->ldx, a->Cin, a->ldw, K, a->ldo, a->Cout);
    ConvP p;
    p.x = (const float*)a->x; p.w = (const float*)a->w; p.bias = (const float*)a->bias; p.out = (float*)a->out;
    p.B = a->B; p.H = a->H; p.W = a->W; p.Cin = a->Cin; p.Cout = a->Cout; p.KH = a->KH; p.KW = a->KW; p.stride = a->stride; p.ph = a->pad_h; p.pw = a->pad_w;
    p.ldx = a->ldx; p.ldw = a->ldw; p.ldo = a->ldo; p.relu = a->relu ? 1 : 0;
    p.Ho = (a->H + 2 * a->pad_h - a->KH) / a->stride + 1;
    p.Wo = (a->W + 2 * a->pad_w - a->KW) / a->stride + 1;
    p.K = (int)K;
    const long long M = (long long)a->B * p.Ho * p.Wo;
    FM_CHECK_ARG(M < (1ll << 31) - 256 && (long long)a->B * a->H * a->W < (1ll << 31), "fm_conv2d_nhwc_f32: more than 2^31 rows (B=%d): convolve in blocks", a->B);
    p.M = (int)M;
    const bool narrow = a->Cout <= 32;                                 // by Cout alone: never by B
    const int TN = narrow ? 32 : 64, TM = narrow ? 128 : 64;
    p.ntn = (a->Cout + TN - 1) / TN;
    FM_CHECK_ARG(((M + TM - 1) / TM) * p.ntn < (1ll << 31), "fm_conv2d_nhwc_f32: too many tiles: convolve in blocks");
    const bool vec = a->Cin % 4 == 0 && a->ldx % 4 == 0 && a->ldw % 4 == 0 && aligned(a->x, 16) && aligned(a->w, 16);
    if (narrow) launch_conv<4, 1>(p, vec, (hipStream_t)stream);
    else launch_conv<2, 2>(p, vec, (hipStream_t)stream);
    FM_CHECK_LAUNCH("fm_conv2d_nhwc_f32");
    return 0;
}

extern "C" int fm_pool2d_nhwc_f32(const void* x, int ldx, void* out, int ldo, int B, int H, int W, int C, int mode, void* stream) {
    FM_CHECK_ARG(x && out, "fm_pool2d_nhwc_f32: null pointer");
    FM_CHECK_ARG(aligned(x, 4) && aligned(out, 4), "fm_pool2d_nhwc_f32: pointers must be 4-byte aligned");
    FM_CHECK_ARG(mode >= FM_POOL_MAX_3X3_S2 && mode <= FM_POOL_GLOBAL_AVG, "fm_pool2d_nhwc_f32: unknown mode %d", mode);
    FM_CHECK_ARG(B >= 1 && H >= 1 && W >= 1 && C >= 1 && ldx >= C && ldo >= C, "fm_pool2d_nhwc_f32: bad shape (B=%d H=%d W=%d C=%d ldx=%d ldo=%d)", B, H, W, C, ldx, ldo);
    FM_CHECK_ARG((long long)B * H * W < (1ll << 31), "fm_pool2d_nhwc_f32: more than 2^31 rows: pool in blocks");
    hipStream_t s = (hipStream_t)stream;
    if (mode == FM_POOL_GLOBAL_AVG) {
        const long long total = (long long)B * C;
        hipLaunchKernelGGL(global_avg_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (const float*)x, ldx, (float*)out, ldo, H * W, C, total);
    } else {
        const bool s2 = mode == FM_POOL_MAX_3X3_S2;
        FM_CHECK_ARG(!s2 || (H >= 3 && W >= 3), "fm_pool2d_nhwc_f32: the valid 3 x 3 window does not fit a %d x %d map", H, W);
        const int Ho = s2 ? (H - 3) / 2 + 1 : H, Wo = s2 ? (W - 3) / 2 + 1 : W;
        const long long total = (long long)B * Ho * Wo * C;
        FM_CHECK_ARG((total + 255) / 256 < (1ll << 31), "fm_pool2d_nhwc_f32: too many elements: pool in blocks");
        hipLaunchKernelGGL(pool3x3_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, (const float*)x, ldx, (float*)out, ldo, H, W, C, Ho, Wo, s2 ? 2 : 1,
                           s2 ? 0 : 1, mode == FM_POOL_AVG_3X3_S1P1 ? 1 : 0, total);
    }
    FM_CHECK_LAUNCH("fm_pool2d_nhwc_f32");
    return 0;
}

extern "C" int fm_inception_preprocess(const void* in, int is_f32, int B, int H, int W, const void* idx, const void* wt, void* out, void* stream) {
    FM_CHECK_ARG(in && idx && wt && out, "fm_inception_preprocess: null pointer");
    FM_CHECK_ARG(aligned(idx, 4) && aligned(wt, 4) && aligned(out, 4) && (!is_f32 || aligned(in, 4)), "fm_inception_preprocess: misaligned pointer");
    FM_CHECK_ARG(B >= 1 && H >= 1 && W >= 1, "fm_inception_preprocess: bad shape (B=%d H=%d W=%d)", B, H, W);
    const long long total = (long long)B * FM_INCEPTION_SIZE * FM_INCEPTION_SIZE * 3;
    FM_CHECK_ARG((total + 255) / 256 < (1ll << 31) && (long long)B * 3 * H * W < (1ll << 40), "fm_inception_preprocess: batch too large: preprocess in blocks");
    const dim3 grid((unsigned)((total + 255) / 256));
    if (is_f32) hipLaunchKernelGGL(inception_preprocess_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, in, H, W, (const int*)idx, (const float*)wt, (float*)out, total);
    else hipLaunchKernelGGL(inception_preprocess_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, in, H, W, (const int*)idx, (const float*)wt, (float*)out, total);
    FM_CHECK_LAUNCH("fm_inception_preprocess");
    return 0;
}

extern "C" int fm_feature_moments(const void* feats, int ld, int n, int d, void* sum, void* outer, void* count, void* stream) {
    FM_CHECK_ARG(feats && sum && outer && count, "fm_feature_moments: null pointer");
    FM_CHECK_ARG(aligned(feats, 4) && aligned(sum, 8) && aligned(outer, 8) && aligned(count, 8), "fm_feature_moments: misaligned pointer (feats 4 bytes; sum, outer, count 8)");
    FM_CHECK_ARG(n >= 1 && d >= 1 && d <= FM_MOMENTS_MAX_D && ld >= d, "fm_feature_moments: bad shape (n=%d d=%d ld=%d: n >= 1, 1 <= d <= %d, ld >= d)", n, d, ld, FM_MOMENTS_MAX_D);
    hipStream_t s = (hipStream_t)stream;
    const unsigned t = (unsigned)((d + 63) / 64);
    hipLaunchKernelGGL(moments_outer_kernel, dim3(t, t), dim3(256), 0, s, (const float*)feats, ld, n, d, (double*)outer);
    hipLaunchKernelGGL(moments_sum_kernel, dim3((unsigned)((d + 255) / 256)), dim3(256), 0, s, (const float*)feats, ld, n, d, (double*)sum, (long long*)count);
    FM_CHECK_LAUNCH("fm_feature_moments");
    return 0;
}
