// Front end of CLIP's VisionTransformer (upstream fourm/utils/clip/model.py:229-237):
//     x = conv1(x) as rows;  x = cat([class_embedding, x]);  x = x + positional_embedding;  x = ln_pre(x)
// The conv1 rows come from the patch GEMM (bias-free, (B * G, D)); everything behind it is this one pass: a wavefront owns an output row
// of the residual stream, builds it in registers from the class embedding or its patch row plus the position row, takes the LayerNorm
// statistics in fp32 (eps inside the sqrt, F.layer_norm semantics) and writes the normalised row as fp32 - the stream the blocks read.
// 4 (B * G * D) + 2 or 4 (B * G * D) bytes move once; the position table and the affine vectors stay in cache.  Unfused, the same rows
// would be written by a cat / add pass and read again by the norm.
#include "common.h"
#include "fourm_hip.h"

namespace {

constexpr int CLIP_MAXC_LIMIT = 8;      // float4 chunks per lane -> D <= 64 * 4 * 8 = 2048 (as fm_layernorm_fwd)

template <bool F32, int MAXC>
__global__ __launch_bounds__(256) void clip_embed_ln_kernel(const void* __restrict__ patches, int ldp, const float* __restrict__ cls, const float* __restrict__ pos,
                                                            const float* __restrict__ w, const float* __restrict__ b, float* __restrict__ out, int ldo,
                                                            int rows, int G, int D, float eps) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nch = D >> 2;
    for (int r = blockIdx.x * 4 + wave; r < rows; r += gridDim.x * 4) {
        const int bi = r / (G + 1), t = r - bi * (G + 1);             // t = 0: the class token, else patch t - 1 of image bi
        const size_t prow = (size_t)bi * G + (t > 0 ? t - 1 : 0);
        float4 v[MAXC];
#pragma unroll
        for (int c = 0; c < MAXC; ++c) {
            const int ch = lane + 64 * c;
            v[c] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (ch < nch) {
                const float4 p = *(const float4*)(pos + (size_t)t * D + ch * 4);
                float4 x;
                if (t == 0) x = *(const float4*)(cls + ch * 4);
                else if constexpr (F32) x = *(const float4*)((const float*)patches + prow * ldp + ch * 4);
                else {
                    float x4[4];
                    unpack_bf4(*(const uint2*)((const bf16_t*)patches + prow * ldp + ch * 4), x4);
                    x = make_float4(x4[0], x4[1], x4[2], x4[3]);
                }
                v[c] = make_float4(x.x + p.x, x.y + p.y, x.z + p.z, x.w + p.w);
            }
        }
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < MAXC; ++c) s += (v[c].x + v[c].y) + (v[c].z + v[c].w);
        const float mu = wave_sum(s) / (float)D;
        float sq = 0.f;
#pragma unroll
        for (int c = 0; c < MAXC; ++c) {
            if (lane + 64 * c < nch) {
                const float a0 = v[c].x - mu, a1 = v[c].y - mu, a2 = v[c].z - mu, a3 = v[c].w - mu;
                sq += (a0 * a0 + a1 * a1) + (a2 * a2 + a3 * a3);
            }
        }
        const float rs = rsqrtf(wave_sum(sq) / (float)D + eps);
        float* orow = out + (size_t)r * ldo;
#pragma unroll
        for (int c = 0; c < MAXC; ++c) {
            const int ch = lane + 64 * c;
            if (ch < nch) {
                const float4 ww = *(const float4*)(w + ch * 4);
                const float4 bb = b ? *(const float4*)(b + ch * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
                *(float4*)(orow + ch * 4) = make_float4((v[c].x - mu) * rs * ww.x + bb.x, (v[c].y - mu) * rs * ww.y + bb.y,
                                                        (v[c].z - mu) * rs * ww.z + bb.z, (v[c].w - mu) * rs * ww.w + bb.w);
            }
        }
    }
}

}  // namespace

extern "C" int fm_clip_embed_ln(const void* patches, int ldp, int patches_f32, const void* cls, const void* pos, const void* w, const void* b,
                                void* out, int ldo, int B, int G, int D, float eps, void* stream) {
    FM_CHECK_ARG(patches && cls && pos && w && out, "fm_clip_embed_ln: null pointer");
    FM_CHECK_ARG(B > 0 && G > 0 && D > 0, "fm_clip_embed_ln: B=%d G=%d D=%d must be positive", B, G, D);
    FM_CHECK_ARG(D % 4 == 0 && D <= 64 * 4 * CLIP_MAXC_LIMIT, "fm_clip_embed_ln: D=%d must be a multiple of 4 and <= %d", D, 64 * 4 * CLIP_MAXC_LIMIT);
    FM_CHECK_ARG(ldp >= D && ldo >= D && ldp % 4 == 0 && ldo % 4 == 0, "fm_clip_embed_ln: ldp=%d ldo=%d must be multiples of 4 and >= D=%d", ldp, ldo, D);
    FM_CHECK_ARG(((((uintptr_t)patches) | ((uintptr_t)cls) | ((uintptr_t)pos) | ((uintptr_t)w) | ((uintptr_t)b) | ((uintptr_t)out)) & 15) == 0,
                 "fm_clip_embed_ln: pointers must be 16-byte aligned");
    const long long rows = (long long)B * (G + 1);
    FM_CHECK_ARG(rows <= 0x7fffffffLL, "fm_clip_embed_ln: %lld rows exceed the grid", rows);
    int grid = (int)((rows + 3) / 4);
    if (grid > 256 * 16) grid = 256 * 16;
    const int chunks = (D / 4 + 63) / 64;
#define CLIP_LN(F, C)                                                                                                                       \
    hipLaunchKernelGGL((clip_embed_ln_kernel<F, C>), dim3(grid), dim3(256), 0, (hipStream_t)stream, patches, ldp, (const float*)cls,         \
                       (const float*)pos, (const float*)w, (const float*)b, (float*)out, ldo, (int)rows, G, D, eps)
#define CLIP_LN_C(F)                                                     \
    if (chunks <= 2) CLIP_LN(F, 2); else if (chunks <= 3) CLIP_LN(F, 3); \
    else if (chunks <= 4) CLIP_LN(F, 4); else CLIP_LN(F, 8)
    if (patches_f32) { CLIP_LN_C(true); } else { CLIP_LN_C(false); }
#undef CLIP_LN_C
#undef CLIP_LN
    FM_CHECK_LAUNCH("fm_clip_embed_ln");
    return 0;
}
