// Tokenizer training objective: what a training step does around VQVAE.forward / backward besides the perceptual losses (include/fourm_hip.h,
// "tokenizer training objective"; upstream run_training_vqvae.py:857-878 and :961-1003, fourm/utils/timm/model_ema.py:70-81,
// run_training_divae.py:966-986, fourm/vq/vq_utils.py:18-46).  Everything is fp32.  Compiled with -ffp-contract=off: fm_mask_out_samples,
// fm_ema_update and fm_diffusion_pair are bit-exact contracts (separately rounded multiplies and adds, spelled with the _rn intrinsics).
// No floating-point atomics anywhere: partial sums go to scratch per workgroup and are added in a fixed order; the integer atomics of
// fm_token_usage (LDS bitmap) and of the valid-pixel count do not depend on the order.
//
// Layouts of fm_reconst_loss: the three element-wise modes walk the flat tensor, 16 bytes per lane; cosine takes one wavefront per (b, c) row
// of H W contiguous values; the three modes that reduce over the strided channel axis (index cross-entropy, binary cross-entropy, cosine_1d)
// take one thread per pixel, so the lanes of a wavefront read consecutive addresses of one channel plane at a time.  The modes that need a
// row's statistics before its gradient read the row a second time (third: the softmax maximum); a workgroup's rows are small enough to be
// served by the cache then.
#include <math.h>

#include "common.h"
#include "fourm_hip.h"

namespace {

constexpr float COS_EPS = 1e-8f;          // F.cosine_similarity's default eps

// workgroup (256 threads) sum in a fixed order: the lanes by the shuffle tree, then the 4 wavefronts in order
__device__ __forceinline__ float block_sum(float v, float* part) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((part[0] + part[1]) + part[2]) + part[3];
}

// ---- mse / l1 / smooth_l1 ---------------------------------------------------------------------------------------------------------------
template <int MODE>
__device__ __forceinline__ void ew_term(float x, float t, float inv_n, float& loss, float& g) {
    const float d = x - t;
    if (MODE == FM_LOSS_MSE) {
        loss = d * d;
        g = (2.0f * d) * inv_n;
    } else if (MODE == FM_LOSS_L1) {
        loss = fabsf(d);
        g = d > 0.f ? inv_n : d < 0.f ? -inv_n : d == 0.f ? 0.f : d;              // sign(0) = 0; a NaN stays one
    } else {                                                                        // smooth_l1, beta = 1
        const float a = fabsf(d);
        loss = a < 1.0f ? (0.5f * d) * d : a - 0.5f;
        g = a < 1.0f ? d * inv_n : d > 0.f ? inv_n : d < 0.f ? -inv_n : d;
    }
}

// thread t of a workgroup owns elements [4 t, 4 t + 4) of each 1024-element slice of its chunk, whichever way they are loaded
template <int MODE, bool VEC>
__global__ __launch_bounds__(256) void loss_elementwise_kernel(const float* __restrict__ x, const float* __restrict__ t, float* __restrict__ grad,
                                                               float* __restrict__ scratch, long long n, float inv_n) {
    __shared__ float part[4];
    const long long base = (long long)blockIdx.x * FM_RECONST_CHUNK;
    float sum = 0.f;
#pragma unroll
    for (int it = 0; it < FM_RECONST_CHUNK / 1024; ++it) {
        const long long e = base + it * 1024 + threadIdx.x * 4;
        if (e >= n) break;
        const int cnt = n - e >= 4 ? 4 : (int)(n - e);
        float xv[4] = {0.f, 0.f, 0.f, 0.f}, tv[4] = {0.f, 0.f, 0.f, 0.f}, gv[4];
        if (VEC && cnt == 4) {
            const float4 a = *(const float4*)(x + e), b = *(const float4*)(t + e);
            xv[0] = a.x; xv[1] = a.y; xv[2] = a.z; xv[3] = a.w; tv[0] = b.x; tv[1] = b.y; tv[2] = b.z; tv[3] = b.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < cnt) { xv[j] = x[e + j]; tv[j] = t[e + j]; }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float l;
            ew_term<MODE>(xv[j], tv[j], inv_n, l, gv[j]);
            if (j < cnt) sum += l;
        }
        if (grad) {
            if (VEC && cnt == 4) *(float4*)(grad + e) = make_float4(gv[0], gv[1], gv[2], gv[3]);
            else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (j < cnt) grad[e + j] = gv[j];
            }
        }
    }
    const float s = block_sum(sum, part);
    if (threadIdx.x == 0) scratch[blockIdx.x] = s;
}

// ---- cosine over the contiguous H W axis: one wavefront per (b, c) row -----------------------------------------------------------------------
// d cos / d x = t / (|x|' |t|') - cos x / (|x|' |x|), |.|' = max(|.|, eps): the installed torch clamps the norms without recording the clamp,
// so its autograd differentiates |x|' as |x|.  A row of norm 0 gets the first term only.
__device__ __forceinline__ void cos_coeffs(float dot, float sxx, float stt, float& cosv, float& a, float& b) {
    const float nx = sqrtf(sxx), nt = sqrtf(stt);
    const float dx = fmaxf(nx, COS_EPS), dt = fmaxf(nt, COS_EPS);
    a = 1.0f / (dx * dt);
    cosv = dot * a;
    b = nx > 0.f ? cosv / (dx * nx) : 0.f;
}

template <bool VEC>
__global__ __launch_bounds__(256) void loss_cosine_kernel(const float* __restrict__ x, const float* __restrict__ t, float* __restrict__ grad,
                                                          float* __restrict__ scratch, long long R, long long HW, float inv_r) {
    __shared__ float part[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long row = (long long)blockIdx.x * 4 + wave;
    float cosv = 0.f;
    if (row < R) {                                                                  // (uniform over the wavefront)
        const float* xr = x + row * HW;
        const float* tr = t + row * HW;
        float dot = 0.f, sxx = 0.f, stt = 0.f;
        if (VEC) {
            for (long long i = lane * 4; i < HW; i += 256) {
                const float4 p = *(const float4*)(xr + i), q = *(const float4*)(tr + i);
                dot += p.x * q.x; dot += p.y * q.y; dot += p.z * q.z; dot += p.w * q.w;
                sxx += p.x * p.x; sxx += p.y * p.y; sxx += p.z * p.z; sxx += p.w * p.w;
                stt += q.x * q.x; stt += q.y * q.y; stt += q.z * q.z; stt += q.w * q.w;
            }
        } else {                                                                    // (the same elements per lane in the same order, loaded one by one)
            for (long long i = lane * 4; i < HW; i += 256)
                for (long long k = i; k < i + 4 && k < HW; ++k) {
                    const float p = xr[k], q = tr[k];
                    dot += p * q; sxx += p * p; stt += q * q;
                }
        }
        dot = wave_sum(dot); sxx = wave_sum(sxx); stt = wave_sum(stt);
        float a, b;
        cos_coeffs(dot, sxx, stt, cosv, a, b);
        if (grad) {
            float* gr = grad + row * HW;
            if (VEC) {
                for (long long i = lane * 4; i < HW; i += 256) {
                    const float4 p = *(const float4*)(xr + i), q = *(const float4*)(tr + i);
                    *(float4*)(gr + i) = make_float4((b * p.x - a * q.x) * inv_r, (b * p.y - a * q.y) * inv_r, (b * p.z - a * q.z) * inv_r,
                                                     (b * p.w - a * q.w) * inv_r);
                }
            } else {
                for (long long i = lane; i < HW; i += 64) gr[i] = (b * xr[i] - a * tr[i]) * inv_r;
            }
        }
    }
    if (lane == 0) part[wave] = cosv;
    __syncthreads();
    if (threadIdx.x == 0) scratch[blockIdx.x] = ((part[0] + part[1]) + part[2]) + part[3];
}

// ---- the modes that reduce over the strided channel axis: one thread per pixel ------------------------------------------------------------
__global__ __launch_bounds__(256) void loss_cosine1d_kernel(const float* __restrict__ x, const float* __restrict__ t, float* __restrict__ grad,
                                                            float* __restrict__ scratch, int C, long long HW, long long npix, float inv_r) {
    __shared__ float part[4];
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    float cosv = 0.f;
    if (p < npix) {
        const long long off = (p / HW) * C * HW + p % HW;
        float dot = 0.f, sxx = 0.f, stt = 0.f;
        for (int c = 0; c < C; ++c) {
            const float u = x[off + c * HW], v = t[off + c * HW];
            dot += u * v; sxx += u * u; stt += v * v;
        }
        float a, b;
        cos_coeffs(dot, sxx, stt, cosv, a, b);
        if (grad)
            for (int c = 0; c < C; ++c) grad[off + c * HW] = (b * x[off + c * HW] - a * t[off + c * HW]) * inv_r;
    }
    const float s = block_sum(cosv, part);
    if (threadIdx.x == 0) scratch[blockIdx.x] = s;
}

// F.cross_entropy with class indices, ignore_index = -100.  count[0]: the number of pixels whose label is not -100 (count_valid_kernel).
// A label outside [0, K) other than -100: that pixel's loss and gradient are NaN; the label is never used as an index.
__global__ __launch_bounds__(256) void loss_ce_index_kernel(const float* __restrict__ x, const long long* __restrict__ labels, float* __restrict__ grad,
                                                            float* __restrict__ scratch, int K, long long HW, long long npix,
                                                            const int* __restrict__ count) {
    __shared__ float part[4];
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    float loss = 0.f;
    if (p < npix) {
        const long long off = (p / HW) * K * HW + p % HW;
        const long long l = labels[p];
        if (l == -100) {
            if (grad)
                for (int k = 0; k < K; ++k) grad[off + k * HW] = 0.f;
        } else {
            const bool ok = l >= 0 && l < K;
            const int li = ok ? (int)l : 0;
            float m = x[off];
            for (int k = 1; k < K; ++k) m = fmaxf(m, x[off + k * HW]);
            float s = 0.f;
            for (int k = 0; k < K; ++k) s += expf(x[off + k * HW] - m);
            const float lse = m + logf(s);
            const float nan = __int_as_float(0x7fc00000);
            loss = ok ? lse - x[off + li * HW] : nan;
            if (grad) {
                const float inv = 1.0f / (float)count[0];
                for (int k = 0; k < K; ++k) {
                    const float pk = expf(x[off + k * HW] - lse);
                    grad[off + k * HW] = ok ? (k == li ? pk - 1.0f : pk) * inv : nan;
                }
            }
        }
    }
    const float s = block_sum(loss, part);
    if (threadIdx.x == 0) scratch[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void count_valid_kernel(const long long* __restrict__ labels, long long npix, int* __restrict__ count) {
    int c = 0;
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < npix; p += (long long)gridDim.x * 256) c += labels[p] != -100 ? 1 : 0;
    c = wave_sum_i(c);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(count, c);
}

// upstream's binary_cross_entropy: s = sigmoid(x); F.cross_entropy of the 2 C "logits" [s_1..s_C, 1 - s_1..1 - s_C] against the
// probabilities q = [t_1..t_C, 1 - t_1..1 - t_C] (sum q = C).  Per pixel: loss = sum_k q_k (lse - z_k) = C lse - sum_k q_k z_k;
// d loss / d z_k = C p_k - q_k; d / d s_c = that at k = c minus that at k = C + c; d / d x_c = (d / d s_c) s_c (1 - s_c).
__global__ __launch_bounds__(256) void loss_bce_kernel(const float* __restrict__ x, const float* __restrict__ t, float* __restrict__ grad,
                                                       float* __restrict__ scratch, int C, long long HW, long long npix, float inv_n) {
    __shared__ float part[4];
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    float loss = 0.f;
    if (p < npix) {
        const long long off = (p / HW) * C * HW + p % HW;
        const float fc = (float)C;
        float S = 0.f, A = 0.f;
        for (int c = 0; c < C; ++c) {
            const float s = 1.0f / (1.0f + expf(-x[off + c * HW])), u = 1.0f - s, q = t[off + c * HW];
            S += expf(s); S += expf(u);
            A += q * s; A += (1.0f - q) * u;
        }
        const float lse = logf(S);
        loss = fc * lse - A;
        if (grad)
            for (int c = 0; c < C; ++c) {
                const float s = 1.0f / (1.0f + expf(-x[off + c * HW])), u = 1.0f - s, q = t[off + c * HW];
                const float g1 = fc * expf(s - lse) - q, g2 = fc * expf(u - lse) - (1.0f - q);
                grad[off + c * HW] = ((g1 - g2) * (s * u)) * inv_n;
            }
    }
    const float s = block_sum(loss, part);
    if (threadIdx.x == 0) scratch[blockIdx.x] = s;
}

// the workgroups' partial sums in a fixed order (thread i takes partials i, i + 256, ...; then the tree) -> the loss
__global__ __launch_bounds__(256) void loss_finish_kernel(const float* __restrict__ scratch, int nparts, int mode, float denom, const int* __restrict__ count,
                                                          float* __restrict__ loss) {
    __shared__ float part[4];
    float s = 0.f;
    for (int i = threadIdx.x; i < nparts; i += 256) s += scratch[i];
    s = block_sum(s, part);
    if (threadIdx.x != 0) return;
    if (mode == FM_LOSS_CE_INDEX) loss[0] = s / (float)count[0];                   // no pixel counted: 0 / 0 = nan, as torch
    else if (mode == FM_LOSS_COSINE || mode == FM_LOSS_COSINE_1D) loss[0] = 1.0f - s / denom;
    else loss[0] = s / denom;
}

// the backward of the loss: grad *= scale[0], nothing touched when the incoming scalar is exactly 1
__global__ __launch_bounds__(256) void scale_kernel(float* __restrict__ x, const float* __restrict__ scale, long long n) {
    const float s = scale[0];
    if (s == 1.0f) return;
    const long long base = (long long)blockIdx.x * FM_RECONST_CHUNK;
#pragma unroll
    for (int it = 0; it < FM_RECONST_CHUNK / 256; ++it) {
        const long long i = base + it * 256 + threadIdx.x;
        if (i < n) x[i] *= s;
    }
}

// ---- mask_out_samples -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mask_out_kernel(float* __restrict__ clean, const uint8_t* __restrict__ valid, float mask_value, float* __restrict__ out,
                                                       int C, long long HW, long long total) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long long hw = i % HW, bc = i / HW;
    const long long b = bc / (C + 1);
    const int c = (int)(bc - b * (C + 1));
    const bool v = valid[b * HW + hw] != 0;
    if (c == C) { out[i] = v ? 1.0f : -1.0f; return; }                              // float(valid) * 2 - 1
    const long long src = (b * C + c) * HW + hw;
    float val = clean[src];
    if (!v) clean[src] = val = mask_value;
    out[i] = val;
}

// ---- ModelEma.update: one launch over a job list -------------------------------------------------------------------------------------------
__device__ __forceinline__ float ema_one(float e, float m, float decay, float one_minus) {
    return __fadd_rn(__fmul_rn(e, decay), __fmul_rn(one_minus, m));
}
__global__ __launch_bounds__(256) void ema_update_kernel(const fm_ema_job* __restrict__ jobs, int n_jobs, float decay, float one_minus) {
    const long long bid = blockIdx.x;
    int lo = 0, hi = n_jobs - 1;                                                    // the last job whose first chunk is <= bid
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (jobs[mid].first_chunk <= bid) lo = mid; else hi = mid - 1;
    }
    const fm_ema_job j = jobs[lo];
    const long long base = (bid - j.first_chunk) * FM_EMA_CHUNK;
    if (bid < j.first_chunk || base >= j.n) return;                                // (a table that does not cover this workgroup)
    float* e = (float*)j.ema;
    const float* m = (const float*)j.model;
    const bool vec = ((((uintptr_t)e) | ((uintptr_t)m)) & 15) == 0;
#pragma unroll
    for (int it = 0; it < FM_EMA_CHUNK / 1024; ++it) {
        const long long i = base + it * 1024 + threadIdx.x * 4;
        if (i >= j.n) break;
        if (vec && j.n - i >= 4) {
            const float4 a = *(const float4*)(e + i), b = *(const float4*)(m + i);
            *(float4*)(e + i) = make_float4(ema_one(a.x, b.x, decay, one_minus), ema_one(a.y, b.y, decay, one_minus), ema_one(a.z, b.z, decay, one_minus),
                                            ema_one(a.w, b.w, decay, one_minus));
        } else {
            const int cnt = j.n - i >= 4 ? 4 : (int)(j.n - i);
            for (int k = 0; k < cnt; ++k) e[i + k] = ema_one(e[i + k], m[i + k], decay, one_minus);
        }
    }
}

// ---- diffusion training pair ------------------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(256) void diffusion_pair_kernel(const float* __restrict__ clean, const float* __restrict__ noise, const long long* __restrict__ timesteps,
                                                             const float* __restrict__ sqrt_alpha, const float* __restrict__ sqrt_sigma, int T,
                                                             float* __restrict__ noisy, float* __restrict__ velocity, long long per) {
    const int b = blockIdx.y;
    const long long ts = timesteps[b];
    const bool ok = ts >= 0 && ts < T;                                              // a timestep outside the table is never used as an index: NaN
    const float nan = __int_as_float(0x7fc00000);
    const float sa = ok ? sqrt_alpha[ts] : nan, ss = ok ? sqrt_sigma[ts] : nan;
    const float* c = clean + (long long)b * per;
    const float* z = noise + (long long)b * per;
    float* o = noisy + (long long)b * per;
    float* v = velocity ? velocity + (long long)b * per : nullptr;
    const long long base = (long long)blockIdx.x * FM_EMA_CHUNK;
#pragma unroll
    for (int it = 0; it < FM_EMA_CHUNK / 1024; ++it) {
        const long long i = base + it * 1024 + threadIdx.x * 4;
        if (i >= per) break;
        if (VEC) {                                                                  // (per % 4 == 0)
            const float4 x = *(const float4*)(c + i), n = *(const float4*)(z + i);
            *(float4*)(o + i) = make_float4(__fadd_rn(__fmul_rn(sa, x.x), __fmul_rn(ss, n.x)), __fadd_rn(__fmul_rn(sa, x.y), __fmul_rn(ss, n.y)),
                                            __fadd_rn(__fmul_rn(sa, x.z), __fmul_rn(ss, n.z)), __fadd_rn(__fmul_rn(sa, x.w), __fmul_rn(ss, n.w)));
            if (v)
                *(float4*)(v + i) = make_float4(__fsub_rn(__fmul_rn(sa, n.x), __fmul_rn(ss, x.x)), __fsub_rn(__fmul_rn(sa, n.y), __fmul_rn(ss, x.y)),
                                                __fsub_rn(__fmul_rn(sa, n.z), __fmul_rn(ss, x.z)), __fsub_rn(__fmul_rn(sa, n.w), __fmul_rn(ss, x.w)));
        } else {
            const int cnt = per - i >= 4 ? 4 : (int)(per - i);
            for (int k = 0; k < cnt; ++k) {
                const float x = c[i + k], n = z[i + k];
                o[i + k] = __fadd_rn(__fmul_rn(sa, x), __fmul_rn(ss, n));
                if (v) v[i + k] = __fsub_rn(__fmul_rn(sa, n), __fmul_rn(ss, x));
            }
        }
    }
}

// ---- codebook usage: distinct tokens per window ---------------------------------------------------------------------------------------------
// One workgroup per window: a bitmap of K bits in LDS (integer atomicOr: the result does not depend on the order), then its population count.
template <typename T>
__global__ __launch_bounds__(256) void token_usage_kernel(const T* __restrict__ tokens, long long window, int K, int* __restrict__ counts, int* __restrict__ bad) {
    extern __shared__ unsigned int bm[];                                            // (K + 31) / 32 words | 4 + 4 ints of the final sums
    const int words = (K + 31) >> 5;
    int* red = (int*)(bm + words);
    for (int i = threadIdx.x; i < words; i += 256) bm[i] = 0u;
    __syncthreads();
    const T* w = tokens + (long long)blockIdx.x * window;
    int nbad = 0;
    for (long long i = threadIdx.x; i < window; i += 256) {
        const long long v = (long long)w[i];
        if (v >= 0 && v < K) {
            const unsigned int bit = 1u << (v & 31);
            if (!(((volatile unsigned int*)bm)[v >> 5] & bit)) atomicOr(&bm[v >> 5], bit);      // (the plain read only spares atomics on a bit already set)
        } else {
            ++nbad;
        }
    }
    __syncthreads();
    int c = 0;
    for (int i = threadIdx.x; i < words; i += 256) c += __popc(bm[i]);
    c = wave_sum_i(c);
    nbad = wave_sum_i(nbad);
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = c; red[4 + (threadIdx.x >> 6)] = nbad; }
    __syncthreads();
    if (threadIdx.x == 0) {
        counts[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
        const int nb = red[4] + red[5] + red[6] + red[7];
        if (nb) atomicAdd(bad, nb);
    }
}

inline bool aligned(const void* p, uintptr_t a) { return (((uintptr_t)p) & (a - 1)) == 0; }
inline bool fits_grid(long long blocks) { return blocks > 0 && blocks <= 0x7fffffffLL; }

// number of partial sums (= workgroups of the main launch) of a mode; 0: bad arguments
long long reconst_parts(int mode, int B, int C, long long HW) {
    if (B <= 0 || C <= 0 || HW <= 0 || mode < FM_LOSS_MSE || mode > FM_LOSS_COSINE_1D) return 0;
    if ((long long)B * C > 0x7fffffffLL || HW > 0x7fffffffLL || (double)B * C * (double)HW > 4.0e12) return 0;
    if (mode <= FM_LOSS_SMOOTH_L1) return ((long long)B * C * HW + FM_RECONST_CHUNK - 1) / FM_RECONST_CHUNK;
    if (mode == FM_LOSS_COSINE) return ((long long)B * C + 3) / 4;
    return ((long long)B * HW + 255) / 256;
}

}  // namespace

extern "C" int fm_reconst_loss_scratch(int mode, int B, int C, int64_t HW) {
    const long long parts = reconst_parts(mode, B, C, HW);
    FM_CHECK_ARG(fits_grid(parts) && parts < 0x7ffffff0LL, "fm_reconst_loss_scratch: bad mode / shape (mode=%d B=%d C=%d HW=%lld)", mode, B, C, (long long)HW);
    return (int)parts + 1;                                                          // + the valid-pixel count of the index cross-entropy
}

extern "C" int fm_reconst_loss(const void* x, const void* target, int mode, int B, int C, int64_t HW, void* grad, void* scratch, void* loss, void* stream) {
    FM_CHECK_ARG(x && target && scratch && loss, "fm_reconst_loss: null pointer");
    const long long parts = reconst_parts(mode, B, C, HW);
    FM_CHECK_ARG(fits_grid(parts) && parts < 0x7ffffff0LL, "fm_reconst_loss: bad mode / shape (mode=%d B=%d C=%d HW=%lld)", mode, B, C, (long long)HW);
    FM_CHECK_ARG(aligned(x, 4) && aligned(grad, 4) && aligned(scratch, 4) && aligned(loss, 4) && aligned(target, mode == FM_LOSS_CE_INDEX ? 8 : 4),
                 "fm_reconst_loss: misaligned pointer");
    hipStream_t st = (hipStream_t)stream;
    const float* xf = (const float*)x;
    const float* tf = (const float*)target;
    float* gf = (float*)grad;
    float* sc = (float*)scratch;
    int* count = (int*)(sc + parts);
    const dim3 grid((unsigned)parts), blk(256);
    const long long n = (long long)B * C * HW, npix = (long long)B * HW, R = (long long)B * C;
    const bool vec = aligned(x, 16) && aligned(target, 16) && aligned(grad, 16);
    float denom = (float)n;
    if (mode <= FM_LOSS_SMOOTH_L1) {
        const float inv_n = 1.0f / (float)n;
#define FM_EW(M) do { if (vec) hipLaunchKernelGGL((loss_elementwise_kernel<M, true>), grid, blk, 0, st, xf, tf, gf, sc, n, inv_n); \
                      else hipLaunchKernelGGL((loss_elementwise_kernel<M, false>), grid, blk, 0, st, xf, tf, gf, sc, n, inv_n); } while (0)
        if (mode == FM_LOSS_MSE) FM_EW(FM_LOSS_MSE); else if (mode == FM_LOSS_L1) FM_EW(FM_LOSS_L1); else FM_EW(FM_LOSS_SMOOTH_L1);
#undef FM_EW
    } else if (mode == FM_LOSS_COSINE) {
        denom = (float)R;
        if (vec && HW % 4 == 0) hipLaunchKernelGGL(loss_cosine_kernel<true>, grid, blk, 0, st, xf, tf, gf, sc, R, (long long)HW, 1.0f / denom);
        else hipLaunchKernelGGL(loss_cosine_kernel<false>, grid, blk, 0, st, xf, tf, gf, sc, R, (long long)HW, 1.0f / denom);
    } else if (mode == FM_LOSS_COSINE_1D) {
        denom = (float)npix;
        hipLaunchKernelGGL(loss_cosine1d_kernel, grid, blk, 0, st, xf, tf, gf, sc, C, (long long)HW, npix, 1.0f / denom);
    } else if (mode == FM_LOSS_BCE) {
        denom = (float)npix;
        hipLaunchKernelGGL(loss_bce_kernel, grid, blk, 0, st, xf, tf, gf, sc, C, (long long)HW, npix, 1.0f / denom);
    } else {
        if (hipMemsetAsync(count, 0, sizeof(int), st) != hipSuccess) { fm_set_error("fm_reconst_loss: hipMemsetAsync failed"); return -2; }
        const long long cb = (npix + 255) / 256;
        hipLaunchKernelGGL(count_valid_kernel, dim3((unsigned)(cb > 1024 ? 1024 : cb)), blk, 0, st, (const long long*)target, npix, count);
        FM_CHECK_LAUNCH("fm_reconst_loss (count)");
        hipLaunchKernelGGL(loss_ce_index_kernel, grid, blk, 0, st, xf, (const long long*)target, gf, sc, C, (long long)HW, npix, (const int*)count);
    }
    FM_CHECK_LAUNCH("fm_reconst_loss");
    hipLaunchKernelGGL(loss_finish_kernel, dim3(1), blk, 0, st, (const float*)sc, (int)parts, mode, denom, (const int*)count, (float*)loss);
    FM_CHECK_LAUNCH("fm_reconst_loss (finish)");
    return 0;
}

extern "C" int fm_scale_f32(void* x, const void* scale, int64_t n, void* stream) {
    FM_CHECK_ARG(x && scale && n > 0 && aligned(x, 4) && aligned(scale, 4), "fm_scale_f32: null / misaligned pointer or n=%lld", (long long)n);
    const long long blocks = (n + FM_RECONST_CHUNK - 1) / FM_RECONST_CHUNK;
    FM_CHECK_ARG(fits_grid(blocks), "fm_scale_f32: too many elements");
    hipLaunchKernelGGL(scale_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (float*)x, (const float*)scale, (long long)n);
    FM_CHECK_LAUNCH("fm_scale_f32");
    return 0;
}

extern "C" int fm_mask_out_samples(void* clean, const void* valid, float mask_value, void* out, int B, int C, int64_t HW, void* stream) {
    FM_CHECK_ARG(clean && valid && out, "fm_mask_out_samples: null pointer");
    FM_CHECK_ARG(B > 0 && C > 0 && HW > 0 && (double)B * (C + 1.0) * (double)HW < 4.0e12, "fm_mask_out_samples: bad shape B=%d C=%d HW=%lld", B, C, (long long)HW);
    FM_CHECK_ARG(aligned(clean, 4) && aligned(out, 4), "fm_mask_out_samples: misaligned pointer");
    const long long total = (long long)B * (C + 1) * HW, blocks = (total + 255) / 256;
    FM_CHECK_ARG(fits_grid(blocks), "fm_mask_out_samples: too many elements");
    hipLaunchKernelGGL(mask_out_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (float*)clean, (const uint8_t*)valid, mask_value, (float*)out, C,
                       (long long)HW, total);
    FM_CHECK_LAUNCH("fm_mask_out_samples");
    return 0;
}

extern "C" int fm_ema_update(const void* jobs, int n_jobs, int64_t chunks, float decay, float one_minus_decay, void* stream) {
    FM_CHECK_ARG(jobs && n_jobs > 0 && aligned(jobs, 8), "fm_ema_update: no job table");
    FM_CHECK_ARG(fits_grid(chunks), "fm_ema_update: chunks=%lld", (long long)chunks);
    hipLaunchKernelGGL(ema_update_kernel, dim3((unsigned)chunks), dim3(256), 0, (hipStream_t)stream, (const fm_ema_job*)jobs, n_jobs, decay, one_minus_decay);
    FM_CHECK_LAUNCH("fm_ema_update");
    return 0;
}

extern "C" int fm_diffusion_pair(const void* clean, const void* noise, const void* timesteps, const void* sqrt_alpha, const void* sqrt_sigma, int T, void* noisy,
                                 void* velocity, int B, int64_t per_sample, void* stream) {
    FM_CHECK_ARG(clean && noise && timesteps && sqrt_alpha && sqrt_sigma && noisy, "fm_diffusion_pair: null pointer");
    FM_CHECK_ARG(B > 0 && B <= 65535 && T > 0 && per_sample > 0, "fm_diffusion_pair: bad shape B=%d T=%d per_sample=%lld (B <= 65535)", B, T, (long long)per_sample);
    FM_CHECK_ARG(aligned(clean, 4) && aligned(noise, 4) && aligned(noisy, 4) && aligned(velocity, 4) && aligned(timesteps, 8) && aligned(sqrt_alpha, 4) &&
                 aligned(sqrt_sigma, 4), "fm_diffusion_pair: misaligned pointer");
    const long long blocks = (per_sample + FM_EMA_CHUNK - 1) / FM_EMA_CHUNK;
    FM_CHECK_ARG(fits_grid(blocks), "fm_diffusion_pair: too many elements");
    const dim3 grid((unsigned)blocks, B), blk(256);
    const bool vec = per_sample % 4 == 0 && aligned(clean, 16) && aligned(noise, 16) && aligned(noisy, 16) && aligned(velocity, 16);
    if (vec) hipLaunchKernelGGL(diffusion_pair_kernel<true>, grid, blk, 0, (hipStream_t)stream, (const float*)clean, (const float*)noise, (const long long*)timesteps,
                                (const float*)sqrt_alpha, (const float*)sqrt_sigma, T, (float*)noisy, (float*)velocity, (long long)per_sample);
    else hipLaunchKernelGGL(diffusion_pair_kernel<false>, grid, blk, 0, (hipStream_t)stream, (const float*)clean, (const float*)noise, (const long long*)timesteps,
                            (const float*)sqrt_alpha, (const float*)sqrt_sigma, T, (float*)noisy, (float*)velocity, (long long)per_sample);
    FM_CHECK_LAUNCH("fm_diffusion_pair");
    return 0;
}

extern "C" int fm_token_usage(const void* tokens, int elem_size, int64_t n_windows, int64_t window, int K, void* counts, void* bad, void* stream) {
    FM_CHECK_ARG(tokens && counts && bad, "fm_token_usage: null pointer");
    FM_CHECK_ARG(elem_size == 2 || elem_size == 4 || elem_size == 8, "fm_token_usage: tokens of %d bytes (int16, int32 or int64)", elem_size);
    FM_CHECK_ARG(K > 0 && K <= FM_TOKEN_USAGE_MAX_K && window > 0 && fits_grid(n_windows), "fm_token_usage: K=%d (<= %d), window=%lld, n_windows=%lld", K,
                 FM_TOKEN_USAGE_MAX_K, (long long)window, (long long)n_windows);
    FM_CHECK_ARG(aligned(tokens, elem_size) && aligned(counts, 4) && aligned(bad, 4), "fm_token_usage: misaligned pointer");
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = ((size_t)((K + 31) / 32) + 8) * 4;
    static bool once = (hipFuncSetAttribute((const void*)token_usage_kernel<long long>, hipFuncAttributeMaxDynamicSharedMemorySize, (FM_TOKEN_USAGE_MAX_K / 32 + 8) * 4) == hipSuccess) &&
                       (hipFuncSetAttribute((const void*)token_usage_kernel<int>, hipFuncAttributeMaxDynamicSharedMemorySize, (FM_TOKEN_USAGE_MAX_K / 32 + 8) * 4) == hipSuccess) &&
                       (hipFuncSetAttribute((const void*)token_usage_kernel<short>, hipFuncAttributeMaxDynamicSharedMemorySize, (FM_TOKEN_USAGE_MAX_K / 32 + 8) * 4) == hipSuccess);
    FM_CHECK_ARG(once, "fm_token_usage: the LDS bitmap could not be reserved");
    if (hipMemsetAsync(bad, 0, sizeof(int), st) != hipSuccess) { fm_set_error("fm_token_usage: hipMemsetAsync failed"); return -2; }
    const dim3 grid((unsigned)n_windows), blk(256);
    if (elem_size == 8) hipLaunchKernelGGL(token_usage_kernel<long long>, grid, blk, lds, st, (const long long*)tokens, (long long)window, K, (int*)counts, (int*)bad);
    else if (elem_size == 4) hipLaunchKernelGGL(token_usage_kernel<int>, grid, blk, lds, st, (const int*)tokens, (long long)window, K, (int*)counts, (int*)bad);
    else hipLaunchKernelGGL(token_usage_kernel<short>, grid, blk, lds, st, (const short*)tokens, (long long)window, K, (int*)counts, (int*)bad);
    FM_CHECK_LAUNCH("fm_token_usage");
    return 0;
}
