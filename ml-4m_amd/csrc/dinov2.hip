// Front end of DINOv2's DinoVisionTransformer (prepare_tokens_with_masks without masks):
//     x = patch_embed(x) as rows;  x = cat([cls_token, x]) + pos(gh, gw);  x = cat([x[:, :1], register_tokens, x[:, 1:]])
// The patch rows come from the patch GEMM (the conv bias rides on its bias=); this pass assembles the fp32 residual stream (B * T, D),
// T = 1 + n_reg + G: row 0 of a sample is cls + pos[0], rows 1 .. n_reg are the register tokens as they are (they get no position), row
// 1 + n_reg + g is patch g + pos[1 + g].  One fp32 add per element, row-local: a sample's rows are the same bits in any batch.  4 (B T D)
// bytes are written once and 2 or 4 (B G D) read once; the table, the class token and the registers stay in cache.
#include "common.h"
#include "fourm_hip.h"

namespace {

template <bool F32>
__global__ __launch_bounds__(256) void cls_pos_embed_kernel(const void* __restrict__ patches, int ldp, const float* __restrict__ cls,
                                                            const float* __restrict__ reg, int n_reg, const float* __restrict__ pos,
                                                            float* __restrict__ out, int ldo, long long rows, int G, int nch) {
    const int T = 1 + n_reg + G;
    const long long total = rows * nch;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long r = i / nch;
        const int ch = (int)(i - r * nch), D = nch * 4;
        const long long bi = r / T;
        const int t = (int)(r - bi * T);
        float4 v;
        if (t >= 1 && t <= n_reg) {
            v = *(const float4*)(reg + (size_t)(t - 1) * D + ch * 4);
        } else {
            const int g = t == 0 ? 0 : t - 1 - n_reg;                       // patch index (unused for the class row)
            const float4 p = *(const float4*)(pos + (size_t)(t == 0 ? 0 : 1 + g) * D + ch * 4);
            float4 x;
            if (t == 0) x = *(const float4*)(cls + ch * 4);
            else if constexpr (F32) x = *(const float4*)((const float*)patches + ((size_t)bi * G + g) * ldp + ch * 4);
            else {
                float x4[4];
                unpack_bf4(*(const uint2*)((const bf16_t*)patches + ((size_t)bi * G + g) * ldp + ch * 4), x4);
                x = make_float4(x4[0], x4[1], x4[2], x4[3]);
            }
            v = make_float4(x.x + p.x, x.y + p.y, x.z + p.z, x.w + p.w);
        }
        *(float4*)(out + (size_t)r * ldo + ch * 4) = v;
    }
}

}  // namespace

extern "C" int fm_cls_pos_embed(const void* patches, int ldp, int patches_f32, const void* cls, const void* reg, int n_reg, const void* pos,
                                void* out, int ldo, int B, int G, int D, void* stream) {
    FM_CHECK_ARG(patches && cls && pos && out, "fm_cls_pos_embed: null pointer");
    FM_CHECK_ARG(B > 0 && G > 0 && D > 0 && D % 4 == 0, "fm_cls_pos_embed: B=%d G=%d must be positive and D=%d a positive multiple of 4", B, G, D);
    FM_CHECK_ARG(n_reg >= 0 && (n_reg == 0 || reg), "fm_cls_pos_embed: n_reg=%d register rows need a register table", n_reg);
    FM_CHECK_ARG(ldp >= D && ldo >= D && ldp % 4 == 0 && ldo % 4 == 0, "fm_cls_pos_embed: ldp=%d ldo=%d must be multiples of 4 and >= D=%d", ldp, ldo, D);
    FM_CHECK_ARG((((uintptr_t)patches) & (patches_f32 ? 15 : 7)) == 0 && (((uintptr_t)cls | (uintptr_t)reg | (uintptr_t)pos | (uintptr_t)out) & 15) == 0,
                 "fm_cls_pos_embed: alignment (bf16 patch rows 8 B, everything else 16 B)");
    const long long rows = (long long)B * (1 + n_reg + G);
    FM_CHECK_ARG(rows <= 0x7fffffffLL, "fm_cls_pos_embed: %lld rows exceed the row index range", rows);
    const int nch = D / 4;
    const long long blocks = (rows * nch + 255) / 256;
    const int grid = (int)(blocks > 256 * 32 ? 256 * 32 : blocks);
    if (patches_f32)
        hipLaunchKernelGGL((cls_pos_embed_kernel<true>), dim3(grid), dim3(256), 0, (hipStream_t)stream, patches, ldp, (const float*)cls,
                           (const float*)reg, n_reg, (const float*)pos, (float*)out, ldo, rows, G, nch);
    else
        hipLaunchKernelGGL((cls_pos_embed_kernel<false>), dim3(grid), dim3(256), 0, (hipStream_t)stream, patches, ldp, (const float*)cls,
                           (const float*)reg, n_reg, (const float*)pos, (float*)out, ldo, rows, G, nch);
    FM_CHECK_LAUNCH("fm_cls_pos_embed");
    return 0;
}
