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

// Adjoint of the pass above with respect to the patch rows (the tower is frozen: no class-token, position or ln_pre gradient).  A wavefront
// owns a patch row: it rebuilds the pre-norm row x = patch + pos in registers, takes the statistics again exactly as the forward did, and
// writes  dx = rstd (dy w - mean(dy w) - x_hat mean(dy w x_hat))  in the type of the patch rows.
template <bool F32, int MAXC>
__global__ __launch_bounds__(256) void clip_embed_ln_bwd_kernel(const float* __restrict__ dy, int lddy, const void* __restrict__ patches, int ldp,
                                                                const float* __restrict__ pos, const float* __restrict__ w, void* __restrict__ dpat, int lddp,
                                                                int rows, int G, int D, float eps) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nch = D >> 2;
    for (int r = blockIdx.x * 4 + wave; r < rows; r += gridDim.x * 4) {          // r: patch row b * G + g
        const int bi = r / G, t = r - bi * G + 1;
        const float* grow = dy + ((size_t)bi * (G + 1) + t) * lddy;
        float4 v[MAXC], gw[MAXC];
#pragma unroll
        for (int c = 0; c < MAXC; ++c) {
            const int ch = lane + 64 * c;
            v[c] = gw[c] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (ch < nch) {
                const float4 p = *(const float4*)(pos + (size_t)t * D + ch * 4);
                float4 x;
                if constexpr (F32) x = *(const float4*)((const float*)patches + (size_t)r * ldp + ch * 4);
                else {
                    float x4[4];
                    unpack_bf4(*(const uint2*)((const bf16_t*)patches + (size_t)r * ldp + ch * 4), x4);
                    x = make_float4(x4[0], x4[1], x4[2], x4[3]);
                }
                v[c] = make_float4(x.x + p.x, x.y + p.y, x.z + p.z, x.w + p.w);
                const float4 d = *(const float4*)(grow + ch * 4), ww = *(const float4*)(w + ch * 4);
                gw[c] = make_float4(d.x * ww.x, d.y * ww.y, d.z * ww.z, d.w * ww.w);
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
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int c = 0; c < MAXC; ++c) {
            if (lane + 64 * c < nch) {
                v[c] = make_float4((v[c].x - mu) * rs, (v[c].y - mu) * rs, (v[c].z - mu) * rs, (v[c].w - mu) * rs);          // x_hat
                s1 += (gw[c].x + gw[c].y) + (gw[c].z + gw[c].w);
                s2 += (gw[c].x * v[c].x + gw[c].y * v[c].y) + (gw[c].z * v[c].z + gw[c].w * v[c].w);
            }
        }
        const float c1 = wave_sum(s1) / (float)D, c2 = wave_sum(s2) / (float)D;
#pragma unroll
        for (int c = 0; c < MAXC; ++c) {
            const int ch = lane + 64 * c;
            if (ch < nch) {
                const float o0 = rs * (gw[c].x - c1 - v[c].x * c2), o1 = rs * (gw[c].y - c1 - v[c].y * c2);
                const float o2 = rs * (gw[c].z - c1 - v[c].z * c2), o3 = rs * (gw[c].w - c1 - v[c].w * c2);
                if constexpr (F32) *(float4*)((float*)dpat + (size_t)r * lddp + ch * 4) = make_float4(o0, o1, o2, o3);
                else *(uint2*)((bf16_t*)dpat + (size_t)r * lddp + ch * 4) = make_uint2(pack2bf(o0, o1), pack2bf(o2, o3));
            }
        }
    }
}

// Feature distance of one tap of the perceptual loss and its gradient (header: fm_feat_distance).  Workgroup b = sample b, 16 wavefronts;
// wavefront k walks tokens k, k + 16, ... : both rows in registers, three sums over D (|p|^2, |t|^2, <p, t>) reduced across the wave, the
// token's value added to the wave's running sum and the token's gradient row written.  The 16 running sums meet in LDS and are added
// in wave order by one thread, which then adds the sample's value to loss[b]: no atomics anywhere, every sum in a fixed order.
constexpr int FEAT_WAVES = 16;

template <int MODE, int MAXC>
__global__ __launch_bounds__(64 * FEAT_WAVES) void feat_distance_kernel(const float* __restrict__ pred, int ldp, const float* __restrict__ tgt, int ldt, int B, int T,
                                                                        int D, float* __restrict__ loss, float* __restrict__ dpred, int lddp) {
    __shared__ float part[FEAT_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, b = blockIdx.x;
    const int nch = D >> 2;
    const float coef = 1.0f / ((float)T * (float)B);          // d(sample value) / d(token value), up to the sign of the cosine form
    float acc = 0.f;
    for (int t = wave; t < T; t += FEAT_WAVES) {
        const size_t row = (size_t)b * T + t;
        float4 p[MAXC], q[MAXC];
        float pp = 0.f, qq = 0.f, pq = 0.f;
#pragma unroll
        for (int c = 0; c < MAXC; ++c) {
            const int ch = lane + 64 * c;
            p[c] = q[c] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (ch < nch) {
                p[c] = *(const float4*)(pred + row * ldp + ch * 4);
                q[c] = *(const float4*)(tgt + row * ldt + ch * 4);
            }
            // explicit fused multiply-adds: |p|^2 and |t|^2 go through the SAME sequence of operations, so equal rows have equal norms bit for
            // bit and p^ - t^ is exactly 0 there (sign(0) = 0), whatever the compiler would have contracted
            pp = fmaf(p[c].w, p[c].w, fmaf(p[c].z, p[c].z, fmaf(p[c].y, p[c].y, fmaf(p[c].x, p[c].x, pp))));
            qq = fmaf(q[c].w, q[c].w, fmaf(q[c].z, q[c].z, fmaf(q[c].y, q[c].y, fmaf(q[c].x, q[c].x, qq))));
            pq = fmaf(p[c].w, q[c].w, fmaf(p[c].z, q[c].z, fmaf(p[c].y, q[c].y, fmaf(p[c].x, q[c].x, pq))));
        }
        pp = wave_sum(pp); qq = wave_sum(qq); pq = wave_sum(pq);
        const float np = sqrtf(pp), nq = sqrtf(qq);
        float* drow = dpred + row * lddp;
        if constexpr (MODE == FM_FEAT_COSINE) {
            // cos = <p, t> / (max(|p|, eps) max(|t|, eps));  d cos / d p = t / (cp ct) - cos p / |p|^2  (the second term only above the clamp)
            const float eps = 1e-8f;
            const float cp = fmaxf(np, eps), cq = fmaxf(nq, eps);
            const float inv = 1.0f / (cp * cq);
            const float cs = pq * inv;
            acc += cs;
            const float a = -coef * inv, bq = np > eps ? coef * cs / pp : 0.f;          // d(-coef cos) / dp = a t + bq p
#pragma unroll
            for (int c = 0; c < MAXC; ++c) {
                const int ch = lane + 64 * c;
                if (ch < nch)
                    *(float4*)(drow + ch * 4) = make_float4(a * q[c].x + bq * p[c].x, a * q[c].y + bq * p[c].y, a * q[c].z + bq * p[c].z, a * q[c].w + bq * p[c].w);
            }
        } else {
#pragma clang fp contract(off)          // p^ and t^ are rounded BEFORE they are subtracted (a fused p ip - t^ would make equal rows differ by a rounding error)
            // value = sum_d |p^ - t^|,  x^ = x / max(|x|, eps);  d value / d p = (s - p^ <s, p^>) / |p| with s = sign(p^ - t^)  (s / eps below the clamp)
            const float eps = 1e-12f;
            const float ip = 1.0f / fmaxf(np, eps), iq = 1.0f / fmaxf(nq, eps);
            float val = 0.f, sp = 0.f;
#pragma unroll
            for (int c = 0; c < MAXC; ++c) {
                const float px[4] = {p[c].x * ip, p[c].y * ip, p[c].z * ip, p[c].w * ip};
                const float qx[4] = {q[c].x * iq, q[c].y * iq, q[c].z * iq, q[c].w * iq};
                float sg[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float d = px[e] - qx[e];
                    sg[e] = d > 0.f ? 1.0f : d < 0.f ? -1.0f : 0.f;
                    val += fabsf(d);
                    sp += sg[e] * px[e];
                }
                p[c] = make_float4(px[0], px[1], px[2], px[3]);          // p^
                q[c] = make_float4(sg[0], sg[1], sg[2], sg[3]);          // s
            }
            val = wave_sum(val);
            sp = np > eps ? wave_sum(sp) : 0.f;
            acc += val;
            const float k = coef * ip;
#pragma unroll
            for (int c = 0; c < MAXC; ++c) {
                const int ch = lane + 64 * c;
                if (ch < nch)
                    *(float4*)(drow + ch * 4) = make_float4(k * (q[c].x - p[c].x * sp), k * (q[c].y - p[c].y * sp), k * (q[c].z - p[c].z * sp), k * (q[c].w - p[c].w * sp));
            }
        }
    }
    if (lane == 0) part[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < FEAT_WAVES; ++k) s += part[k];
        const float mean = s / (float)T;
        loss[b] += (MODE == FM_FEAT_COSINE ? 1.0f - mean : mean) / (float)B;
    }
}

}  // namespace

extern "C" int fm_clip_embed_ln_bwd(const void* dy, int lddy, const void* patches, int ldp, int patches_f32, const void* pos, const void* w,
                                    void* d_patches, int lddp, int B, int G, int D, float eps, void* stream) {
    FM_CHECK_ARG(dy && patches && pos && w && d_patches, "fm_clip_embed_ln_bwd: null pointer");
    FM_CHECK_ARG(B > 0 && G > 0 && D > 0, "fm_clip_embed_ln_bwd: B=%d G=%d D=%d must be positive", B, G, D);
    FM_CHECK_ARG(D % 4 == 0 && D <= 64 * 4 * CLIP_MAXC_LIMIT, "fm_clip_embed_ln_bwd: D=%d must be a multiple of 4 and <= %d", D, 64 * 4 * CLIP_MAXC_LIMIT);
    FM_CHECK_ARG(lddy >= D && ldp >= D && lddp >= D && lddy % 4 == 0 && ldp % 4 == 0 && lddp % 4 == 0,
                 "fm_clip_embed_ln_bwd: lddy=%d ldp=%d lddp=%d must be multiples of 4 and >= D=%d", lddy, ldp, lddp, D);
    FM_CHECK_ARG(((((uintptr_t)dy) | ((uintptr_t)patches) | ((uintptr_t)pos) | ((uintptr_t)w) | ((uintptr_t)d_patches)) & 15) == 0,
                 "fm_clip_embed_ln_bwd: pointers must be 16-byte aligned");
    const long long rows = (long long)B * G;
    FM_CHECK_ARG((long long)B * (G + 1) <= 0x7fffffffLL, "fm_clip_embed_ln_bwd: %lld rows exceed the grid", (long long)B * (G + 1));
    int grid = (int)((rows + 3) / 4);
    if (grid > 256 * 16) grid = 256 * 16;
    const int chunks = (D / 4 + 63) / 64;
#define CLIP_LNB(F, C)                                                                                                                          \
    hipLaunchKernelGGL((clip_embed_ln_bwd_kernel<F, C>), dim3(grid), dim3(256), 0, (hipStream_t)stream, (const float*)dy, lddy, patches, ldp,    \
                       (const float*)pos, (const float*)w, d_patches, lddp, (int)rows, G, D, eps)
#define CLIP_LNB_C(F)                                                      \
    if (chunks <= 2) CLIP_LNB(F, 2); else if (chunks <= 3) CLIP_LNB(F, 3); \
    else if (chunks <= 4) CLIP_LNB(F, 4); else CLIP_LNB(F, 8)
    if (patches_f32) { CLIP_LNB_C(true); } else { CLIP_LNB_C(false); }
#undef CLIP_LNB_C
#undef CLIP_LNB
    FM_CHECK_LAUNCH("fm_clip_embed_ln_bwd");
    return 0;
}

extern "C" int fm_feat_distance(const void* pred, int ldp, const void* tgt, int ldt, int B, int T, int D, int mode, void* loss, void* dpred, int lddp,
                                void* stream) {
    FM_CHECK_ARG(pred && tgt && loss && dpred, "fm_feat_distance: null pointer");
    FM_CHECK_ARG(mode == FM_FEAT_COSINE || mode == FM_FEAT_L1, "fm_feat_distance: mode=%d is neither FM_FEAT_COSINE nor FM_FEAT_L1", mode);
    FM_CHECK_ARG(B > 0 && T > 0 && D > 0, "fm_feat_distance: B=%d T=%d D=%d must be positive", B, T, D);
    FM_CHECK_ARG(D % 4 == 0 && D <= 64 * 4 * CLIP_MAXC_LIMIT, "fm_feat_distance: D=%d must be a multiple of 4 and <= %d", D, 64 * 4 * CLIP_MAXC_LIMIT);
    FM_CHECK_ARG(ldp >= D && ldt >= D && lddp >= D && ldp % 4 == 0 && ldt % 4 == 0 && lddp % 4 == 0,
                 "fm_feat_distance: ldp=%d ldt=%d lddp=%d must be multiples of 4 and >= D=%d", ldp, ldt, lddp, D);
    FM_CHECK_ARG(((((uintptr_t)pred) | ((uintptr_t)tgt) | ((uintptr_t)dpred)) & 15) == 0 && (((uintptr_t)loss) & 3) == 0,
                 "fm_feat_distance: rows must be 16-byte aligned");
    const int chunks = (D / 4 + 63) / 64;
#define FEAT(M, C)                                                                                                                              \
    hipLaunchKernelGGL((feat_distance_kernel<M, C>), dim3(B), dim3(64 * FEAT_WAVES), 0, (hipStream_t)stream, (const float*)pred, ldp,           \
                       (const float*)tgt, ldt, B, T, D, (float*)loss, (float*)dpred, lddp)
#define FEAT_C(M)                                                  \
    if (chunks <= 1) FEAT(M, 1); else if (chunks <= 2) FEAT(M, 2); \
    else if (chunks <= 3) FEAT(M, 3); else if (chunks <= 4) FEAT(M, 4); else FEAT(M, 8)
    if (mode == FM_FEAT_COSINE) { FEAT_C(FM_FEAT_COSINE); } else { FEAT_C(FM_FEAT_L1); }
#undef FEAT_C
#undef FEAT
    FM_CHECK_LAUNCH("fm_feat_distance");
    return 0;
}

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
