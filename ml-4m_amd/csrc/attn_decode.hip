// fm_attn_decode: the attention step of incremental (K/V-cache) decoding in one launch - one query row per sample against the first
// Nk rows of that sample's keys / values, with the per-head LayerNorm of qk_norm models (NormAttention / NormCrossAttention,
// fourm/models/fm_utils.py:222-261) folded in: q is normalised on chip, the new token's key is normalised, written back into the
// cache and used as the stored value.  A decoding step is a chain of ~135 dependent launches of a few microseconds each (DESIGN.md
// section 7), so what counts here is the number of launches and the latency of one, not bandwidth: Nk is 1 to a few hundred.
//
// One workgroup of 4 waves per (sample, head):
//   1. wave 0 loads q (lane d = feature d) and normalises it; wave 1 does the same for the key of row k_new_row and stores it;
//      both leave their 64 values in LDS.  The norm runs in double (6 shuffle steps on the data shifted by its first element,
//      mean and mean square together): the stored key is then the correctly rounded LayerNorm also where x - mean cancels.
//   2. scores, one key per thread: 64 fused multiply-adds in feature order over 16-byte loads of the key row, q broadcast from LDS.
//   3. block maximum and sum (wave shuffles, then the four waves in a fixed order), exp in place in LDS.
//   4. P V, 16 bytes of a value row per lane (8 / 16 lanes per key), the key groups of a wave meet in shuffles, the waves in LDS.
// Every loop is bounded by Nk; no workgroup reads or writes what another one writes.
#include "common.h"
#include "fourm_hip.h"

namespace {

constexpr float DEC_NEG_BF16 = -3.3895313892515355e38f;     // -finfo(bfloat16).max (fm_attn_fwd)
constexpr float DEC_NEG_F32 = -3.4028234663852886e38f;      // -finfo(float32).max  (fm_attn_f32_fwd)

struct DecArgs {
    const void* q; void* k; const void* v; void* o;
    const float* q_w; const float* q_b; const float* k_w; const float* k_b;
    const uint8_t* kpad;
    int ldq, ldk, ldv, ldo, H, Nk, kvr, k_new_row, zero_attn;
    float scale, eps;
};

__device__ __forceinline__ float ld1(const float* p) { return *p; }
__device__ __forceinline__ float ld1(const bf16_t* p) { return bf2f(*p); }
__device__ __forceinline__ float st1(float* p, float v) { *p = v; return v; }                       // -> the value as stored
__device__ __forceinline__ float st1(bf16_t* p, float v) { const bf16_t b = f2bf(v); *p = b; return bf2f(b); }
// 16 bytes of a row: 4 fp32 / 8 bf16 elements
__device__ __forceinline__ void ld16(const float* p, float (&v)[4]) {
    const float4 t = *(const float4*)p;
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
}
__device__ __forceinline__ void ld16(const bf16_t* p, float (&v)[8]) {
    const uint4 t = *(const uint4*)p;
    v[0] = bf2f((bf16_t)(t.x & 0xffff)); v[1] = bf2f((bf16_t)(t.x >> 16)); v[2] = bf2f((bf16_t)(t.y & 0xffff)); v[3] = bf2f((bf16_t)(t.y >> 16));
    v[4] = bf2f((bf16_t)(t.z & 0xffff)); v[5] = bf2f((bf16_t)(t.z >> 16)); v[6] = bf2f((bf16_t)(t.w & 0xffff)); v[7] = bf2f((bf16_t)(t.w >> 16));
}

// LayerNorm of the 64 values a wave holds (one per lane).  Shifted by lane 0's value, so mean and mean square can be reduced together
// without the cancellation of E[x^2] - E[x]^2 on data far from zero.
__device__ __forceinline__ float head_norm(float x, const float* w, const float* b, float eps, int lane) {
    const double t = (double)x - (double)__shfl(x, 0, 64);
    double s1 = t, s2 = t * t;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s1 += __shfl_xor(s1, o, 64);
        s2 += __shfl_xor(s2, o, 64);
    }
    const double m = s1 * (1.0 / 64.0);
    const double var = fmax(s2 * (1.0 / 64.0) - m * m, 0.0);
    const double y = (t - m) * (1.0 / sqrt(var + (double)eps)) * (double)w[lane] + (b ? (double)b[lane] : 0.0);
    return (float)y;
}

template <typename T>
__global__ __launch_bounds__(256) void attn_decode_kernel(DecArgs a) {
    constexpr int VEC = 16 / sizeof(T);          // elements per 16-byte load
    constexpr int LPK = 64 / VEC;                // lanes that share one value row in the P V phase
    constexpr int KPW = 64 / LPK;                // value rows a wave reads at once
    extern __shared__ float sp[];                // [Nk] scores, then exp(score - max)
    __shared__ __attribute__((aligned(16))) float sq[64];
    __shared__ __attribute__((aligned(16))) float snew[64];
    __shared__ float sred[4][64];
    __shared__ float swred[8];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.x / a.H, h = blockIdx.x - b * a.H;
    const int Nk = a.Nk;
    const T* q = (const T*)a.q + (size_t)b * a.ldq + h * 64;
    T* kb = (T*)a.k + (size_t)b * a.kvr * a.ldk + h * 64;
    const T* vb = (const T*)a.v + (size_t)b * a.kvr * a.ldv + h * 64;
    const int knew = a.q_w ? a.k_new_row : -1;   // (< Nk: checked on the host)

    if (wave == 0) {
        float x = ld1(q + lane);
        if (a.q_w) x = head_norm(x, a.q_w, a.q_b, a.eps, lane);
        sq[lane] = x;
    } else if (wave == 1 && knew >= 0) {
        T* kr = kb + (size_t)knew * a.ldk;
        snew[lane] = st1(kr + lane, head_norm(ld1(kr + lane), a.k_w, a.k_b, a.eps, lane));
    }
    __syncthreads();

    // ---- scores --------------------------------------------------------------------------------------------------------------
    const float neg = sizeof(T) == 4 ? DEC_NEG_F32 : DEC_NEG_BF16;
    float mx = -INFINITY;
    for (int j = tid; j < Nk; j += 256) {
        float s = 0.f;
        if (j == knew) {
#pragma unroll
            for (int d = 0; d < 64; ++d) s = fmaf(sq[d], snew[d], s);
        } else {
            const T* kr = kb + (size_t)j * a.ldk;
#pragma unroll
            for (int c = 0; c < 64; c += VEC) {
                float kv[VEC];
                ld16(kr + c, kv);
#pragma unroll
                for (int e = 0; e < VEC; ++e) s = fmaf(sq[c + e], kv[e], s);
            }
        }
        s *= a.scale;
        if (a.kpad && a.kpad[(size_t)b * Nk + j]) s = neg;
        sp[j] = s;
        mx = fmaxf(mx, s);
    }
    mx = wave_max(mx);
    if (lane == 0) swred[wave] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(swred[0], swred[1]), fmaxf(swred[2], swred[3]));
    if (a.zero_attn) mx = fmaxf(mx, 0.f);          // softmax1 (fm_utils.py:28-30): one extra zero logit whose probability is dropped
    float sum = 0.f;
    for (int j = tid; j < Nk; j += 256) {          // (the scores this thread wrote itself)
        const float e = expf(sp[j] - mx);
        sp[j] = e;
        sum += e;
    }
    sum = wave_sum(sum);
    if (lane == 0) swred[4 + wave] = sum;
    __syncthreads();
    sum = (swred[4] + swred[5]) + (swred[6] + swred[7]);
    if (a.zero_attn) sum += expf(-mx);

    // ---- o = sum_j p_j v_j ----------------------------------------------------------------------------------------------------
    const int sub = lane / LPK, c0 = (lane - sub * LPK) * VEC;
    float acc[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[e] = 0.f;
    for (int j = wave * KPW + sub; j < Nk; j += 4 * KPW) {
        float vv[VEC];
        ld16(vb + (size_t)j * a.ldv + c0, vv);
        const float p = sp[j];
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[e] = fmaf(p, vv[e], acc[e]);
    }
#pragma unroll
    for (int o = LPK; o < 64; o <<= 1)
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[e] += __shfl_xor(acc[e], o, 64);
    if (sub == 0) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) sred[wave][c0 + e] = acc[e];
    }
    __syncthreads();
    if (tid < 64) {
        const float o = ((sred[0][tid] + sred[1][tid]) + (sred[2][tid] + sred[3][tid])) / sum;
        st1((T*)a.o + (size_t)b * a.ldo + h * 64 + tid, o);
    }
}

}  // namespace

extern "C" int fm_attn_decode(const fm_attn_decode_args* p, void* stream) {
    FM_CHECK_ARG(p && p->q && p->k && p->v && p->o, "fm_attn_decode: null pointer");
    FM_CHECK_ARG(p->B >= 1 && p->H >= 1, "fm_attn_decode: B=%d, H=%d must be >= 1", p->B, p->H);
    FM_CHECK_ARG(p->Nk >= 1 && p->Nk <= FM_ATTN_DECODE_MAX_NK, "fm_attn_decode: Nk=%d outside 1 .. %d", p->Nk, FM_ATTN_DECODE_MAX_NK);
    const int kvr = p->kv_batch_rows > 0 ? p->kv_batch_rows : p->Nk;
    FM_CHECK_ARG(p->B == 1 || kvr >= p->Nk, "fm_attn_decode: kv_batch_rows=%d < Nk=%d", p->kv_batch_rows, p->Nk);
    FM_CHECK_ARG(p->k_new_row < p->Nk, "fm_attn_decode: k_new_row=%d is not one of the Nk=%d rows", p->k_new_row, p->Nk);
    FM_CHECK_ARG(!(p->q_w && p->k_new_row >= 0 && !p->k_w), "fm_attn_decode: k_new_row=%d needs k_w", p->k_new_row);
    const int D = 64 * p->H;
    FM_CHECK_ARG(p->ldq >= D && p->ldk >= D && p->ldv >= D && p->ldo >= D, "fm_attn_decode: a row stride is smaller than 64 H = %d", D);
    const int esz = p->is_f32 ? 4 : 2, vec = 16 / esz;
    FM_CHECK_ARG((uintptr_t)p->k % 16 == 0 && (uintptr_t)p->v % 16 == 0 && p->ldk % vec == 0 && p->ldv % vec == 0,
                 "fm_attn_decode: misaligned k / v (16 bytes, row strides multiples of %d elements)", vec);
    FM_CHECK_ARG((uintptr_t)p->q % esz == 0 && (uintptr_t)p->o % esz == 0 && (uintptr_t)p->q_w % 4 == 0 && (uintptr_t)p->q_b % 4 == 0 &&
                 (uintptr_t)p->k_w % 4 == 0 && (uintptr_t)p->k_b % 4 == 0, "fm_attn_decode: misaligned q / o / norm vector");
    DecArgs a;
    a.q = p->q; a.k = p->k; a.v = p->v; a.o = p->o;
    a.q_w = (const float*)p->q_w; a.q_b = (const float*)p->q_b; a.k_w = (const float*)p->k_w; a.k_b = (const float*)p->k_b;
    a.kpad = (const uint8_t*)p->kpad;
    a.ldq = p->ldq; a.ldk = p->ldk; a.ldv = p->ldv; a.ldo = p->ldo; a.H = p->H; a.Nk = p->Nk; a.kvr = kvr; a.k_new_row = p->k_new_row;
    a.zero_attn = p->zero_attn; a.scale = p->scale; a.eps = p->eps;
    const dim3 grid((unsigned)p->B * (unsigned)p->H);
    const size_t lds = (size_t)p->Nk * sizeof(float);
    if (p->is_f32) hipLaunchKernelGGL(attn_decode_kernel<float>, grid, dim3(256), lds, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(attn_decode_kernel<bf16_t>, grid, dim3(256), lds, (hipStream_t)stream, a);
    FM_CHECK_LAUNCH("fm_attn_decode");
    return 0;
}
