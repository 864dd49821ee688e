// LPIPS perceptual loss: the kernels around the 3 x 3 implicit-GEMM convolutions of the frozen VGG16 (include/fourm_hip.h, "LPIPS perceptual
// loss"; upstream fourm/vq/percept_losses/lpips.py:96-177).  Feature maps are rows (B * H * W, C), bf16 or f32 (F32 template argument: the
// fp32 verification mode, nothing rounded).  Every kernel is a streaming kernel: 16-byte accesses per lane, fixed summation orders, no atomics.
//
// |p| = 0 in fm_lpips_distance: d p^ / d p = I / (|p| + eps) - p p^T / ((|p| + eps)^2 |p|); the second term divides by the norm and is taken
// as 0 there (torch's autograd yields NaN).  p = 0 after a ReLU means every channel of that pixel is masked, so the tap layer's ReLU mask
// (fm_lpips_tap_bwd) zeroes that pixel's gradient whatever the rule; the rule only keeps NaN out of the rows.
#include "common.h"
#include "fourm_hip.h"

namespace {

template <bool F32> struct RowT { using type = bf16_t; };
template <> struct RowT<true> { using type = float; };

// 8 consecutive channels of a row -> floats / back (16 bytes of bf16, 32 bytes of f32)
template <bool F32>
__device__ __forceinline__ void load8(const void* row, int c, float (&v)[8]) {
    if constexpr (F32) {
        const float4 a = *(const float4*)((const float*)row + c), b = *(const float4*)((const float*)row + c + 4);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    } else {
        const uint4 t = *(const uint4*)((const bf16_t*)row + c);
        const uint32_t u[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) { v[2 * i] = bf2f((bf16_t)(u[i] & 0xffff)); v[2 * i + 1] = bf2f((bf16_t)(u[i] >> 16)); }
    }
}
template <bool F32>
__device__ __forceinline__ void store8(void* row, int c, const float (&v)[8]) {
    if constexpr (F32) {
        *(float4*)((float*)row + c) = make_float4(v[0], v[1], v[2], v[3]);
        *(float4*)((float*)row + c + 4) = make_float4(v[4], v[5], v[6], v[7]);
    } else {
        *(uint4*)((bf16_t*)row + c) = make_uint4(pack2bf(v[0], v[1]), pack2bf(v[2], v[3]), pack2bf(v[4], v[5]), pack2bf(v[6], v[7]));
    }
}
// 4 consecutive channels
template <bool F32>
__device__ __forceinline__ void load4(const void* row, int c, float (&v)[4]) {
    if constexpr (F32) {
        const float4 a = *(const float4*)((const float*)row + c);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    } else {
        unpack_bf4(*(const uint2*)((const bf16_t*)row + c), v);
    }
}
template <bool F32>
__device__ __forceinline__ void store4(void* row, int c, const float (&v)[4]) {
    if constexpr (F32) *(float4*)((float*)row + c) = make_float4(v[0], v[1], v[2], v[3]);
    else *(uint2*)((bf16_t*)row + c) = make_uint2(pack2bf(v[0], v[1]), pack2bf(v[2], v[3]));
}

// ---- stem: ScalingLayer + conv1_1 + bias + ReLU --------------------------------------------------------------------------------------
// 8 lanes per pixel, 8 output channels per lane: a wavefront writes 8 consecutive rows (1 KiB of bf16) with one 16-byte store per lane.
// The 27 x 64 weights are staged in LDS ([k][64]) once per workgroup, which then walks its share of the pixels; the 8 lanes of a pixel read
// the same 27 input values (one address per 8 lanes), all requested before the first is used.
template <bool F32>
__global__ __launch_bounds__(256) void lpips_stem_kernel(const float* __restrict__ img, const float* __restrict__ mul, const float* __restrict__ add,
                                                         const float* __restrict__ w, const float* __restrict__ bias, void* __restrict__ out, int ldo,
                                                         int B, int H, int W) {
    __shared__ __attribute__((aligned(16))) float ws[27 * 64];
    __shared__ __attribute__((aligned(16))) float bs[64];
    for (int i = threadIdx.x; i < 27 * 64; i += 256) {
        const int n = i & 63, k = i >> 6;
        const float v = w[n * 27 + k];
        ws[i] = F32 ? v : bfround(v);
    }
    if (threadIdx.x < 64) bs[threadIdx.x] = F32 ? bias[threadIdx.x] : bfround(bias[threadIdx.x]);
    __syncthreads();
    const int cg = (threadIdx.x & 7) * 8;
    float br[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) br[e] = bs[cg + e];
    const float m0 = mul[0], m1 = mul[1], m2 = mul[2], a0 = add[0], a1 = add[1], a2 = add[2];
    const long long total = (long long)B * H * W;
    const int hw = H * W;
    for (long long pix = (long long)blockIdx.x * 32 + (threadIdx.x >> 3); pix < total; pix += (long long)gridDim.x * 32) {
        const int b = (int)(pix / hw), r = (int)(pix - (long long)b * hw), y = r / W, x = r - y * W;
        // all 27 inputs first, from clamped (always valid) addresses: the loads are in flight together, the padding is a select afterwards
        float s[27];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float m = c == 0 ? m0 : c == 1 ? m1 : m2, a = c == 0 ? a0 : c == 1 ? a1 : a2;
            const float* plane = img + ((long long)b * 3 + c) * hw;
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const int yy = y + ky - 1, xx = x + kx - 1;
                    const bool in = (unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W;
                    float v = fmaf(plane[min(max(yy, 0), H - 1) * W + min(max(xx, 0), W - 1)], m, a);
                    if (!F32) v = bfround(v);
                    s[c * 9 + ky * 3 + kx] = in ? v : 0.f;                           // zero padding in the SCALED space
                }
        }
        float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        // (the weights are re-read from LDS for every pixel: hoisted out of the loop they take 216 registers and leave one wavefront per SIMD)
        asm volatile("" ::: "memory");
#pragma unroll
        for (int k = 0; k < 27; ++k) {
            const float4 w0 = *(const float4*)(ws + k * 64 + cg), w1 = *(const float4*)(ws + k * 64 + cg + 4);
            acc[0] = fmaf(s[k], w0.x, acc[0]); acc[1] = fmaf(s[k], w0.y, acc[1]); acc[2] = fmaf(s[k], w0.z, acc[2]); acc[3] = fmaf(s[k], w0.w, acc[3]);
            acc[4] = fmaf(s[k], w1.x, acc[4]); acc[5] = fmaf(s[k], w1.y, acc[5]); acc[6] = fmaf(s[k], w1.z, acc[6]); acc[7] = fmaf(s[k], w1.w, acc[7]);
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float v = acc[e] + br[e];
            acc[e] = fmaxf(F32 ? v : bfround(v), 0.f);
        }
        typename RowT<F32>::type* orow = (typename RowT<F32>::type*)out + pix * ldo;
        store8<F32>(orow, cg, acc);
    }
}

// ---- stem backward: one thread per pixel, its three channels; taps (ky, kx) outermost, the 64 output channels in order ------------------
template <bool F32>
__global__ __launch_bounds__(256) void lpips_stem_bwd_kernel(const void* __restrict__ d, int ldd, const float* __restrict__ w, const float* __restrict__ mul,
                                                             const float* __restrict__ row_scale, float* __restrict__ dimg, int B, int H, int W) {
    __shared__ __attribute__((aligned(16))) float ws[9 * 64 * 4];                   // [tap][n][c (padded to 4)]
    for (int i = threadIdx.x; i < 9 * 64 * 4; i += 256) {
        const int c = i & 3, n = (i >> 2) & 63, tap = i >> 8;
        float v = 0.f;
        if (c < 3) { v = w[n * 27 + c * 9 + tap]; if (!F32) v = bfround(v); }
        ws[i] = v;
    }
    __syncthreads();
    const long long total = (long long)B * H * W;
    const long long pix = (long long)blockIdx.x * 256 + threadIdx.x;
    if (pix >= total) return;
    const int hw = H * W;
    const int b = (int)(pix / hw), r = (int)(pix - (long long)b * hw), y = r / W, x = r - y * W;
    const typename RowT<F32>::type* base = (const typename RowT<F32>::type*)d;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    for (int ky = 0; ky < 3; ++ky)
        for (int kx = 0; kx < 3; ++kx) {
            const int oy = y + 1 - ky, ox = x + 1 - kx;                               // the output pixel whose tap (ky, kx) read this pixel
            if ((unsigned)oy >= (unsigned)H || (unsigned)ox >= (unsigned)W) continue;
            const typename RowT<F32>::type* row = base + ((long long)b * hw + (long long)oy * W + ox) * ldd;
            const float* wt = ws + (ky * 3 + kx) * 256;
#pragma unroll
            for (int n0 = 0; n0 < 64; n0 += 8) {
                float v[8];
                load8<F32>(row, n0, v);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float4 wv = *(const float4*)(wt + (n0 + e) * 4);
                    a0 = fmaf(v[e], wv.x, a0); a1 = fmaf(v[e], wv.y, a1); a2 = fmaf(v[e], wv.z, a2);
                }
            }
        }
    const float rs = row_scale ? row_scale[b] : 1.0f;
    float* o = dimg + (long long)b * 3 * hw + r;
    o[0] = (a0 * mul[0]) * rs;
    o[hw] = (a1 * mul[1]) * rs;
    o[2 * hw] = (a2 * mul[2]) * rs;
}

// ---- 2 x 2 max-pool on rows: one thread per 8 output channels ----------------------------------------------------------------------------
template <bool F32>
__global__ __launch_bounds__(256) void maxpool2x2_kernel(const void* __restrict__ x, int ldx, void* __restrict__ y, int ldy, int B, int H, int W, int C) {
    const int C8 = C >> 3, Ho = H >> 1, Wo = W >> 1;
    const long long total = (long long)B * Ho * Wo * C8;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % C8) * 8;
    const long long op = i / C8;
    const int ox = (int)(op % Wo), oy = (int)((op / Wo) % Ho), b = (int)(op / ((long long)Wo * Ho));
    using T = typename RowT<F32>::type;
    const T* r00 = (const T*)x + ((long long)b * H * W + (long long)(2 * oy) * W + 2 * ox) * ldx;
    float m[8], v[8];
    load8<F32>(r00, c, m);
    load8<F32>(r00 + ldx, c, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) m[e] = fmaxf(m[e], v[e]);
    load8<F32>(r00 + (long long)W * ldx, c, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) m[e] = fmaxf(m[e], v[e]);
    load8<F32>(r00 + (long long)(W + 1) * ldx, c, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) m[e] = fmaxf(m[e], v[e]);
    store8<F32>((T*)y + op * ldy, c, m);
}

// ---- per-tap distance ----------------------------------------------------------------------------------------------------------------------
// grid (chunks, B), 4 wavefronts.  LP lanes share a pixel (16 for C <= 64, 32 for C <= 128, else 64: no idle lanes at the wide, shallow
// taps), a lane holds channels [4 (l + LP j), + 4) of it, j < J; a wavefront takes 64 / LP pixels at a time.  Partial sums: a lane group's
// pixels in order, the groups of a wavefront by a fixed shuffle tree, then the 4 wavefronts in order -> scratch[b * chunks + chunk].
template <int LP>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
    for (int o = LP / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
template <bool F32, int LP>
__global__ __launch_bounds__(256) void lpips_distance_kernel(const void* __restrict__ pred, int ldp, const void* __restrict__ tgt, int ldt,
                                                             const float* __restrict__ w, int P, int C, float* __restrict__ dpred, int lddp,
                                                             float* __restrict__ scratch) {
    constexpr int PPW = 64 / LP, J = LP == 64 ? 2 : 1;
    __shared__ float part[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane / LP, sl = lane % LP;
    const int b = blockIdx.y, chunk = blockIdx.x;
    using T = typename RowT<F32>::type;
    float wv[J][4];
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const int c = 4 * (sl + LP * j);
#pragma unroll
        for (int e = 0; e < 4; ++e) wv[j][e] = c < C ? w[c + e] : 0.f;
    }
    const float inv_p = 1.0f / (float)P;
    float sum = 0.f;
    for (int i0 = wave * PPW; i0 < FM_LPIPS_CHUNK; i0 += 4 * PPW) {
        if (chunk * FM_LPIPS_CHUNK + i0 >= P) break;                               // (uniform over the wavefront)
        const int px = chunk * FM_LPIPS_CHUNK + i0 + sub;
        const bool valid = px < P;
        const long long row = (long long)b * P + (valid ? px : P - 1);            // (a dead lane group re-reads the last pixel and contributes nothing)
        float p[J][4], t[J][4];
        float sp = 0.f, st = 0.f;
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const int c = 4 * (sl + LP * j);
            if (c < C) {
                load4<F32>((const T*)pred + row * ldp, c, p[j]);
                load4<F32>((const T*)tgt + row * ldt, c, t[j]);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) p[j][e] = t[j][e] = 0.f;
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) { sp = fmaf(p[j][e], p[j][e], sp); st = fmaf(t[j][e], t[j][e], st); }
        }
        sp = group_sum<LP>(sp); st = group_sum<LP>(st);
        const float np = sqrtf(sp), dp = np + 1e-10f, dt = sqrtf(st) + 1e-10f;
        float val = 0.f, gp = 0.f;
        float g[J][4];
#pragma unroll
        for (int j = 0; j < J; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float diff = p[j][e] / dp - t[j][e] / dt;
                const float wd = wv[j][e] * diff;
                val = fmaf(wd, diff, val);
                g[j][e] = 2.0f * wd * inv_p;
                gp = fmaf(g[j][e], p[j][e], gp);
            }
        val = group_sum<LP>(val);
        sum += valid ? val : 0.f;
        if (dpred) {
            gp = group_sum<LP>(gp);
            const float k = np > 0.f ? gp / (dp * dp * np) : 0.f;                  // |p| = 0: the term that divides by the norm is 0
#pragma unroll
            for (int j = 0; j < J; ++j) {
                const int c = 4 * (sl + LP * j);
                if (valid && c < C)
                    *(float4*)(dpred + row * lddp + c) = make_float4(g[j][0] / dp - p[j][0] * k, g[j][1] / dp - p[j][1] * k,
                                                                     g[j][2] / dp - p[j][2] * k, g[j][3] / dp - p[j][3] * k);
            }
        }
    }
#pragma unroll
    for (int o = LP; o < 64; o <<= 1) sum += __shfl_xor(sum, o, 64);               // the lane groups of this wavefront
    if (lane == 0) part[wave] = sum;
    __syncthreads();
    if (threadIdx.x == 0) scratch[(long long)b * gridDim.x + chunk] = ((part[0] + part[1]) + part[2]) + part[3];
}
// loss[b] += (the chunks' partial sums, added in chunk order) / P: one wavefront per sample, lane l takes chunks l, l + 64, ... in order
__global__ __launch_bounds__(64) void lpips_distance_sum_kernel(const float* __restrict__ scratch, int chunks, int P, float* __restrict__ loss) {
    const int b = blockIdx.x, lane = threadIdx.x;
    float s = 0.f;
    for (int i = lane; i < chunks; i += 64) s += scratch[(long long)b * chunks + i];
    s = wave_sum(s);
    if (lane == 0) loss[b] += s * (1.0f / (float)P);
}

// ---- tap layer backward / ReLU mask: one thread per 4 channels of a pixel ---------------------------------------------------------------
template <bool F32>
__global__ __launch_bounds__(256) void lpips_tap_bwd_kernel(const void* __restrict__ act, int lda, const void* din, int ldi, const float* __restrict__ dtap, int ldt,
                                                            const void* __restrict__ dpool, int ldp, void* d, int ldd, int B, int H, int W, int C) {
    const int C4 = C >> 2;
    const long long total = (long long)B * H * W * C4;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % C4) * 4;
    const long long pix = i / C4;
    using T = typename RowT<F32>::type;
    float a[4], v[4] = {0.f, 0.f, 0.f, 0.f};
    load4<F32>((const T*)act + pix * lda, c, a);
    if (din) load4<F32>((const T*)din + pix * ldi, c, v);
    if (dtap) {
        const float4 t = *(const float4*)(dtap + pix * ldt + c);
        v[0] += t.x; v[1] += t.y; v[2] += t.z; v[3] += t.w;
    }
    if (dpool) {
        const int x = (int)(pix % W), y = (int)((pix / W) % H), b = (int)(pix / ((long long)W * H));
        const int pos = (y & 1) * 2 + (x & 1);
        const long long win = (long long)b * H * W + (long long)(y & ~1) * W + (x & ~1);
        bool first[4] = {true, true, true, true};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (q == pos) continue;
            float o[4];
            load4<F32>((const T*)act + (win + (q >> 1) * W + (q & 1)) * lda, c, o);
#pragma unroll
            for (int e = 0; e < 4; ++e) first[e] = first[e] && (q < pos ? a[e] > o[e] : a[e] >= o[e]);
        }
        float g[4];
        load4<F32>((const T*)dpool + ((long long)b * (H >> 1) * (W >> 1) + (long long)(y >> 1) * (W >> 1) + (x >> 1)) * ldp, c, g);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] += first[e] ? g[e] : 0.f;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = a[e] > 0.f ? v[e] : 0.f;
    store4<F32>((T*)d + pix * ldd, c, v);
}

inline bool aligned(const void* p, uintptr_t a) { return (((uintptr_t)p) & (a - 1)) == 0; }
inline bool fits_grid(long long blocks) { return blocks > 0 && blocks <= 0x7fffffffLL; }

}  // namespace

extern "C" int fm_lpips_stem(const void* img, const void* mul, const void* add, const void* w, const void* bias, void* out, int ldo, int is_f32, int B, int H,
                             int W, void* stream) {
    FM_CHECK_ARG(img && mul && add && w && bias && out, "fm_lpips_stem: null pointer");
    FM_CHECK_ARG(B > 0 && H > 0 && W > 0 && (long long)H * W <= 0x7fffffffLL, "fm_lpips_stem: bad shape B=%d H=%d W=%d", B, H, W);
    FM_CHECK_ARG(ldo >= 64 && ldo % 8 == 0 && aligned(out, 16) && aligned(img, 4), "fm_lpips_stem: ldo=%d must be >= 64 and a multiple of 8, out 16-byte aligned", ldo);
    long long blocks = ((long long)B * H * W + 31) / 32;
    FM_CHECK_ARG(fits_grid(blocks), "fm_lpips_stem: too many pixels");
    if (blocks > 2048) blocks = 2048;          // a workgroup walks pixel groups blockIdx.x, + gridDim.x, ...: its weights are staged once
    if (is_f32) hipLaunchKernelGGL(lpips_stem_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const float*)img, (const float*)mul, (const float*)add,
                                   (const float*)w, (const float*)bias, out, ldo, B, H, W);
    else hipLaunchKernelGGL(lpips_stem_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const float*)img, (const float*)mul, (const float*)add,
                            (const float*)w, (const float*)bias, out, ldo, B, H, W);
    FM_CHECK_LAUNCH("fm_lpips_stem");
    return 0;
}

extern "C" int fm_lpips_stem_bwd(const void* d, int ldd, int is_f32, const void* w, const void* mul, const void* row_scale, void* dimg, int B, int H, int W,
                                 void* stream) {
    FM_CHECK_ARG(d && w && mul && dimg, "fm_lpips_stem_bwd: null pointer");
    FM_CHECK_ARG(B > 0 && H > 0 && W > 0 && (long long)H * W <= 0x7fffffffLL, "fm_lpips_stem_bwd: bad shape B=%d H=%d W=%d", B, H, W);
    FM_CHECK_ARG(ldd >= 64 && ldd % 8 == 0 && aligned(d, 16) && aligned(dimg, 4), "fm_lpips_stem_bwd: ldd=%d must be >= 64 and a multiple of 8, d 16-byte aligned", ldd);
    const long long blocks = ((long long)B * H * W + 255) / 256;
    FM_CHECK_ARG(fits_grid(blocks), "fm_lpips_stem_bwd: too many pixels");
    if (is_f32) hipLaunchKernelGGL(lpips_stem_bwd_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, d, ldd, (const float*)w, (const float*)mul,
                                   (const float*)row_scale, (float*)dimg, B, H, W);
    else hipLaunchKernelGGL(lpips_stem_bwd_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, d, ldd, (const float*)w, (const float*)mul,
                            (const float*)row_scale, (float*)dimg, B, H, W);
    FM_CHECK_LAUNCH("fm_lpips_stem_bwd");
    return 0;
}

extern "C" int fm_maxpool2x2_nhwc(const void* x, int ldx, void* y, int ldy, int is_f32, int B, int H, int W, int C, void* stream) {
    FM_CHECK_ARG(x && y, "fm_maxpool2x2_nhwc: null pointer");
    FM_CHECK_ARG(B > 0 && H > 0 && W > 0 && C > 0 && H % 2 == 0 && W % 2 == 0 && C % 8 == 0, "fm_maxpool2x2_nhwc: bad shape B=%d H=%d W=%d C=%d (H, W even, C %% 8 == 0)", B, H, W, C);
    FM_CHECK_ARG(ldx >= C && ldy >= C && ldx % 8 == 0 && ldy % 8 == 0 && aligned(x, 16) && aligned(y, 16), "fm_maxpool2x2_nhwc: leading dimensions %d / %d (>= C, %% 8 == 0) and 16-byte aligned pointers", ldx, ldy);
    const long long blocks = ((long long)B * (H / 2) * (W / 2) * (C / 8) + 255) / 256;
    FM_CHECK_ARG(fits_grid(blocks), "fm_maxpool2x2_nhwc: too many elements");
    if (is_f32) hipLaunchKernelGGL(maxpool2x2_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, ldx, y, ldy, B, H, W, C);
    else hipLaunchKernelGGL(maxpool2x2_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, ldx, y, ldy, B, H, W, C);
    FM_CHECK_LAUNCH("fm_maxpool2x2_nhwc");
    return 0;
}

extern "C" int fm_lpips_distance(const void* pred, int ldp, const void* tgt, int ldt, int is_f32, const void* w, int B, int P, int C, void* loss, void* dpred,
                                 int lddp, void* scratch, void* stream) {
    FM_CHECK_ARG(pred && tgt && w && loss && scratch, "fm_lpips_distance: null pointer");
    FM_CHECK_ARG(B > 0 && B <= 65535 && P > 0 && C > 0 && C % 4 == 0 && C <= 512, "fm_lpips_distance: bad shape B=%d P=%d C=%d (C %% 4 == 0, C <= 512, B <= 65535)", B, P, C);
    FM_CHECK_ARG(ldp >= C && ldt >= C && ldp % 4 == 0 && ldt % 4 == 0 && (!dpred || (lddp >= C && lddp % 4 == 0)), "fm_lpips_distance: leading dimensions %d / %d / %d (>= C, %% 4 == 0)", ldp, ldt, lddp);
    FM_CHECK_ARG(aligned(pred, 16) && aligned(tgt, 16) && aligned(w, 16) && aligned(loss, 4) && aligned(scratch, 4) && aligned(dpred, 16), "fm_lpips_distance: pointers must be 16-byte aligned");
    const int chunks = (P + FM_LPIPS_CHUNK - 1) / FM_LPIPS_CHUNK;
    const dim3 grid(chunks, B);
    hipStream_t st = (hipStream_t)stream;
#define FM_LPIPS_DIST(F, LP) hipLaunchKernelGGL((lpips_distance_kernel<F, LP>), grid, dim3(256), 0, st, pred, ldp, tgt, ldt, (const float*)w, P, C, (float*)dpred, lddp, (float*)scratch)
    if (is_f32) { if (C <= 64) FM_LPIPS_DIST(true, 16); else if (C <= 128) FM_LPIPS_DIST(true, 32); else FM_LPIPS_DIST(true, 64); }
    else { if (C <= 64) FM_LPIPS_DIST(false, 16); else if (C <= 128) FM_LPIPS_DIST(false, 32); else FM_LPIPS_DIST(false, 64); }
#undef FM_LPIPS_DIST
    FM_CHECK_LAUNCH("fm_lpips_distance");
    hipLaunchKernelGGL(lpips_distance_sum_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, (const float*)scratch, chunks, P, (float*)loss);
    FM_CHECK_LAUNCH("fm_lpips_distance (sum)");
    return 0;
}

extern "C" int fm_lpips_tap_bwd(const void* act, int lda, const void* din, int ldi, const void* dtap, int ldt, const void* dpool, int ldp, void* d, int ldd,
                                int is_f32, int B, int H, int W, int C, void* stream) {
    FM_CHECK_ARG(act && d, "fm_lpips_tap_bwd: null pointer");
    FM_CHECK_ARG(B > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0 && (!dpool || (H % 2 == 0 && W % 2 == 0)), "fm_lpips_tap_bwd: bad shape B=%d H=%d W=%d C=%d (C %% 4 == 0; H, W even with dpool)", B, H, W, C);
    FM_CHECK_ARG(lda >= C && lda % 4 == 0 && ldd >= C && ldd % 4 == 0 && (!din || (ldi >= C && ldi % 4 == 0)) && (!dtap || (ldt >= C && ldt % 4 == 0)) && (!dpool || (ldp >= C && ldp % 4 == 0)),
                 "fm_lpips_tap_bwd: leading dimensions must be >= C and multiples of 4");
    const uintptr_t al = is_f32 ? 16 : 8;
    FM_CHECK_ARG(aligned(act, al) && aligned(din, al) && aligned(dpool, al) && aligned(d, al) && aligned(dtap, 16), "fm_lpips_tap_bwd: misaligned pointer");
    const long long blocks = ((long long)B * H * W * (C / 4) + 255) / 256;
    FM_CHECK_ARG(fits_grid(blocks), "fm_lpips_tap_bwd: too many elements");
    if (is_f32) hipLaunchKernelGGL(lpips_tap_bwd_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, act, lda, din, ldi, (const float*)dtap, ldt, dpool, ldp, d, ldd, B, H, W, C);
    else hipLaunchKernelGGL(lpips_tap_bwd_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, act, lda, din, ldi, (const float*)dtap, ldt, dpool, ldp, d, ldd, B, H, W, C);
    FM_CHECK_LAUNCH("fm_lpips_tap_bwd");
    return 0;
}
