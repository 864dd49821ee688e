// LayerScale on the residual stream (DINOv2's blocks: x = x + gamma * branch(norm(x)), a learned per-channel gamma):
//     fm_layernorm_fwd_res_ls   x_out = x + gamma[c] * float(delta),  y = LN(x_out)   - fm_layernorm_fwd_res with the scale in front of the add
//     fm_layerscale_add         x_out = x + gamma[c] * float(delta)                    - the same sum where no norm follows (bf16 or f32 delta)
// The arithmetic is eager torch's: the product is rounded to fp32, then the sum is rounded to fp32 (under autocast bf16 * fp32 promotes to
// fp32).  ls_add() below keeps the two roundings apart (no fused multiply-add), so x_out is checkable bit for bit against the CPU; everything
// behind it - the LayerNorm statistics and the affine store - is the text of ln_fwd_kernel (layernorm.hip), compiled the same way, so that
// y / mean / rstd carry the bits fm_layernorm_fwd gives on that x_out.
//
// HBM-bound like the kernels they extend: one wavefront per row with the row in registers (<= 2048 columns), 16-byte accesses; gamma (D floats)
// is read per chunk and stays in cache.
#include "common.h"
#include "fourm_hip.h"

namespace {

constexpr int LS_MAXC_LIMIT = 8;   // float4 chunks per lane  ->  D <= 64 * 4 * 8 = 2048 (as fm_layernorm_fwd)

// x + gamma * d with the product and the sum rounded separately
__device__ __forceinline__ float ls_add(float x, float g, float d) {
#pragma clang fp contract(off)
    const float p = g * d;
    return x + p;
}

template <typename T> __device__ __forceinline__ void ls_store4(T* p, float a, float b, float c, float d);
template <> __device__ __forceinline__ void ls_store4<float>(float* p, float a, float b, float c, float d) {
    *(float4*)p = make_float4(a, b, c, d);
}
template <> __device__ __forceinline__ void ls_store4<bf16_t>(bf16_t* p, float a, float b, float c, float d) {
    *(uint2*)p = make_uint2(pack2bf(a, b), pack2bf(c, d));
}

template <typename OutT, int MAXC>
__global__ __launch_bounds__(256) void ln_fwd_ls_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ w,
                                                        const float* __restrict__ b, OutT* __restrict__ y, int ldy,
                                                        float* __restrict__ mean, float* __restrict__ rstd,
                                                        const int* __restrict__ row_map, int R, int D, float eps,
                                                        const bf16_t* __restrict__ delta, int ldd, const float* __restrict__ gamma,
                                                        float* __restrict__ xo, int ldxo) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nch = D >> 2;
    float4 ww[MAXC], bb[MAXC];
#pragma unroll
    for (int c = 0; c < MAXC; ++c) {
        const int ch = lane + 64 * c;
        ww[c] = ch < nch ? *(const float4*)(w + ch * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
        bb[c] = (b && ch < nch) ? *(const float4*)(b + ch * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    constexpr int NR = 2;
    for (int r0 = blockIdx.x * 4 + wave; r0 < R; r0 += gridDim.x * 4 * NR) {
        float4 v[NR][MAXC];
        uint2 dl[NR][MAXC];
#pragma unroll
        for (int q = 0; q < NR; ++q) {
            const int r = r0 + q * gridDim.x * 4;
#pragma unroll
            for (int c = 0; c < MAXC; ++c) {
                const int ch = lane + 64 * c;
                const bool in = ch < nch && r < R;
                v[q][c] = in ? *(const float4*)(x + (size_t)r * ldx + ch * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
                dl[q][c] = in ? *(const uint2*)(delta + (size_t)r * ldd + ch * 4) : make_uint2(0u, 0u);
            }
        }
#pragma unroll
        for (int c = 0; c < MAXC; ++c) {
            const int ch = lane + 64 * c;
            const float4 g = ch < nch ? *(const float4*)(gamma + ch * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int q = 0; q < NR; ++q) {
                const int r = r0 + q * gridDim.x * 4;
                float d4[4];
                unpack_bf4(dl[q][c], d4);
                v[q][c].x = ls_add(v[q][c].x, g.x, d4[0]); v[q][c].y = ls_add(v[q][c].y, g.y, d4[1]);
                v[q][c].z = ls_add(v[q][c].z, g.z, d4[2]); v[q][c].w = ls_add(v[q][c].w, g.w, d4[3]);
                if (ch < nch && r < R) *(float4*)(xo + (size_t)r * ldxo + ch * 4) = v[q][c];
            }
        }
#pragma unroll
        for (int q = 0; q < NR; ++q) {
            const int r = r0 + q * gridDim.x * 4;
            if (r >= R) continue;
            float s = 0.f;
#pragma unroll
            for (int c = 0; c < MAXC; ++c) s += (v[q][c].x + v[q][c].y) + (v[q][c].z + v[q][c].w);
            const float mu = wave_sum(s) / (float)D;
            float sq = 0.f;
#pragma unroll
            for (int c = 0; c < MAXC; ++c) {
                const int ch = lane + 64 * c;
                if (ch < nch) {
                    const float a0 = v[q][c].x - mu, a1 = v[q][c].y - mu, a2 = v[q][c].z - mu, a3 = v[q][c].w - mu;
                    sq += (a0 * a0 + a1 * a1) + (a2 * a2 + a3 * a3);
                }
            }
            const float rs = rsqrtf(wave_sum(sq) / (float)D + eps);
            if (lane == 0) {
                if (mean) mean[r] = mu;
                if (rstd) rstd[r] = rs;
            }
            const int dst = row_map ? row_map[r] : r;
            if (dst < 0) continue;
            OutT* yr = y + (size_t)dst * ldy;
#pragma unroll
            for (int c = 0; c < MAXC; ++c) {
                const int ch = lane + 64 * c;
                if (ch < nch)
                    ls_store4<OutT>(yr + ch * 4, (v[q][c].x - mu) * rs * ww[c].x + bb[c].x, (v[q][c].y - mu) * rs * ww[c].y + bb[c].y,
                                    (v[q][c].z - mu) * rs * ww[c].z + bb[c].z, (v[q][c].w - mu) * rs * ww[c].w + bb[c].w);
            }
        }
    }
}

// one thread per 4 columns of a row; x_out may be x itself (every element is read before it is written, by the thread that writes it)
template <bool F32>
__global__ __launch_bounds__(256) void layerscale_add_kernel(const float* x, int ldx, const void* __restrict__ delta, int ldd,
                                                             const float* __restrict__ gamma, float* xo, int ldxo, int R, int nch) {
    const long long total = (long long)R * nch;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int r = (int)(i / nch), ch = (int)(i - (long long)r * nch);
        const float4 a = *(const float4*)(x + (size_t)r * ldx + ch * 4);
        const float4 g = *(const float4*)(gamma + ch * 4);
        float d4[4];
        if constexpr (F32) {
            const float4 d = *(const float4*)((const float*)delta + (size_t)r * ldd + ch * 4);
            d4[0] = d.x; d4[1] = d.y; d4[2] = d.z; d4[3] = d.w;
        } else {
            unpack_bf4(*(const uint2*)((const bf16_t*)delta + (size_t)r * ldd + ch * 4), d4);
        }
        *(float4*)(xo + (size_t)r * ldxo + ch * 4) = make_float4(ls_add(a.x, g.x, d4[0]), ls_add(a.y, g.y, d4[1]), ls_add(a.z, g.z, d4[2]), ls_add(a.w, g.w, d4[3]));
    }
}

}  // namespace

static int ls_chunks_for(int D) { const int c = (D / 4 + 63) / 64; return c <= 2 ? 2 : c <= 3 ? 3 : c <= 4 ? 4 : 8; }

extern "C" int fm_layernorm_fwd_res_ls(const void* x, int ldx, const void* delta, int ldd, const void* gamma, void* x_out, int ldxo, const void* w,
                                       const void* b, void* y, int ldy, int y_is_f32, void* mean, void* rstd, const int32_t* row_map, int R, int D,
                                       float eps, void* stream) {
    FM_CHECK_ARG(x && delta && gamma && x_out && w && y, "fm_layernorm_fwd_res_ls: null pointer");
    FM_CHECK_ARG(R > 0 && D > 0 && D % 4 == 0 && D <= 64 * 4 * LS_MAXC_LIMIT, "fm_layernorm_fwd_res_ls: D=%d must be a multiple of 4 and <= %d", D, 64 * 4 * LS_MAXC_LIMIT);
    FM_CHECK_ARG(ldx % 4 == 0 && ldy % 4 == 0 && ldd % 4 == 0 && ldxo % 4 == 0 && ldx >= D && ldy >= D && ldd >= D && ldxo >= D,
                 "fm_layernorm_fwd_res_ls: leading dims must be multiples of 4 and >= D=%d", D);
    FM_CHECK_ARG((((uintptr_t)delta) & 7) == 0 && (((uintptr_t)x_out | (uintptr_t)x | (uintptr_t)gamma | (uintptr_t)w | (uintptr_t)b) & 15) == 0 &&
                 (((uintptr_t)y) & (y_is_f32 ? 15 : 7)) == 0, "fm_layernorm_fwd_res_ls: alignment (delta / bf16 y 8 B, everything else 16 B)");
    FM_CHECK_ARG(x != x_out, "fm_layernorm_fwd_res_ls: x_out may not alias x");
    int grid = (R + 3) / 4;
    if (grid > 256 * 16) grid = 256 * 16;
#define LN_LS(T, C)                                                                                                                    \
    hipLaunchKernelGGL((ln_fwd_ls_kernel<T, C>), dim3(grid), dim3(256), 0, (hipStream_t)stream, (const float*)x, ldx, (const float*)w,  \
                       (const float*)b, (T*)y, ldy, (float*)mean, (float*)rstd, row_map, R, D, eps, (const bf16_t*)delta, ldd,         \
                       (const float*)gamma, (float*)x_out, ldxo)
#define LN_LS_C(T)                                    \
    switch (ls_chunks_for(D)) {                       \
        case 2: LN_LS(T, 2); break;                   \
        case 3: LN_LS(T, 3); break;                   \
        case 4: LN_LS(T, 4); break;                   \
        default: LN_LS(T, 8); break;                  \
    }
    if (y_is_f32) { LN_LS_C(float) } else { LN_LS_C(bf16_t) }
#undef LN_LS_C
#undef LN_LS
    FM_CHECK_LAUNCH("fm_layernorm_fwd_res_ls");
    return 0;
}

extern "C" int fm_layerscale_add(const void* x, int ldx, const void* delta, int ldd, int delta_is_f32, const void* gamma, void* x_out, int ldxo,
                                 int R, int D, void* stream) {
    FM_CHECK_ARG(x && delta && gamma && x_out, "fm_layerscale_add: null pointer");
    FM_CHECK_ARG(R > 0 && D > 0 && D % 4 == 0, "fm_layerscale_add: R=%d must be positive and D=%d a positive multiple of 4", R, D);
    FM_CHECK_ARG(ldx % 4 == 0 && ldd % 4 == 0 && ldxo % 4 == 0 && ldx >= D && ldd >= D && ldxo >= D,
                 "fm_layerscale_add: leading dims must be multiples of 4 and >= D=%d", D);
    FM_CHECK_ARG((((uintptr_t)delta) & (delta_is_f32 ? 15 : 7)) == 0 && (((uintptr_t)x_out | (uintptr_t)x | (uintptr_t)gamma) & 15) == 0,
                 "fm_layerscale_add: alignment (bf16 delta 8 B, everything else 16 B)");
    FM_CHECK_ARG(x != x_out || ldx == ldxo, "fm_layerscale_add: an in-place sum needs ldx == ldxo");
    const int nch = D / 4;
    const long long total = (long long)R * nch;
    long long blocks = (total + 255) / 256;
    const int grid = (int)(blocks > 256 * 32 ? 256 * 32 : blocks);
    if (delta_is_f32)
        hipLaunchKernelGGL((layerscale_add_kernel<true>), dim3(grid), dim3(256), 0, (hipStream_t)stream, (const float*)x, ldx, delta, ldd,
                           (const float*)gamma, (float*)x_out, ldxo, R, nch);
    else
        hipLaunchKernelGGL((layerscale_add_kernel<false>), dim3(grid), dim3(256), 0, (hipStream_t)stream, (const float*)x, ldx, delta, ldd,
                           (const float*)gamma, (float*)x_out, ldxo, R, nch);
    FM_CHECK_LAUNCH("fm_layerscale_add");
    return 0;
}
