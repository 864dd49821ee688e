// Low-rank adapters (LoRA, fourm/models/lora_utils.py) beside a frozen or trainable nn.Linear: the rank-r path the dense GEMM family
// has no place for.  Two kernels:
//   fm_lora_apply  P = x down^T (fp32), y += scale P up^T in place, P written out.  The backward's dX term is the same call with the two
//                  small matrices exchanged and transposed through their element strides (header).
//   fm_lora_grad   out[n][j] (+)= scale sum_rows a[row][n] b[row][j]: the adapters' own gradients, a tall-skinny reduction over the rows.
// Both stream the big operand once with 8 / 16 bytes per lane and keep the rank-r operand on chip; neither uses the matrix cores: with
// r <= 64 the work is r multiply-adds per streamed element, far below what HBM delivers.
#include "common.h"
#include "fourm_hip.h"

namespace {

constexpr int LORA_TM = 64;          // rows of x / y per tile: 16 per wave
constexpr int LORA_WCAP = 10240;     // fp32 staged per workgroup for down / up (40 KiB)
constexpr int LORA_PS = 64;          // row stride of the P tile (r <= 64)

__device__ __forceinline__ void load4(const float* p, float (&v)[4]) {
    const float4 t = *(const float4*)p;
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
}
__device__ __forceinline__ void load4(const bf16_t* p, float (&v)[4]) { unpack_bf4(*(const uint2*)p, v); }
__device__ __forceinline__ void store4(float* p, const float (&v)[4]) { *(float4*)p = make_float4(v[0], v[1], v[2], v[3]); }
__device__ __forceinline__ void store4(bf16_t* p, const float (&v)[4]) { *(uint2*)p = make_uint2(pack2bf(v[0], v[1]), pack2bf(v[2], v[3])); }
__device__ __forceinline__ void store1(float* p, float v) { *p = v; }
__device__ __forceinline__ void store1(bf16_t* p, float v) { *p = f2bf(v); }

// dst[j * ld + c] = src[j * s_row + (c0 + c) * s_col] for j < r, c < cols; the pad columns cols .. ld - 1 are zeroed.
// The index that is contiguous in memory runs fastest over the threads.
__device__ __forceinline__ void lora_stage(float* dst, int ld, const float* __restrict__ src, int r, int c0, int cols, int64_t s_row, int64_t s_col) {
    const int total = r * ld;
    if (s_col == 1) {
        for (int idx = threadIdx.x; idx < total; idx += 256) {
            const int j = idx / ld, c = idx - j * ld;
            dst[idx] = c < cols ? src[j * s_row + (c0 + c)] : 0.f;
        }
    } else {
        for (int idx = threadIdx.x; idx < total; idx += 256) {
            const int c = idx / r, j = idx - c * r;
            dst[j * ld + c] = c < cols ? src[j * s_row + (int64_t)(c0 + c) * s_col] : 0.f;
        }
    }
}

// RT: compile-time bound of r (16 or 64); ROWS: rows a wave reduces at once in the first phase (ROWS * RT accumulators per lane).
template <typename TX, typename TY, int RT, int ROWS>
__global__ __launch_bounds__(256) void lora_apply_kernel(const TX* __restrict__ x, int ldx, const float* __restrict__ down, int64_t sdr, int64_t sdk,
                                                         const float* __restrict__ up, int64_t sun, int64_t sur, TY* y, int ldy, float scale,
                                                         float* __restrict__ p_out, int R, int K, int N, int r, int KS, int NS, int resident) {
    __shared__ __attribute__((aligned(16))) float sW[LORA_WCAP];
    __shared__ __attribute__((aligned(16))) float sP[LORA_TM * LORA_PS];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ldK = (KS + 3) & ~3, ldN = (NS + 3) & ~3;
    float* sDown = sW;
    float* sUp = resident ? sW + r * ldK : sW;
    if (resident) {      // both matrices fit: staged once for every tile of this workgroup
        lora_stage(sDown, ldK, down, r, 0, K, sdr, sdk);
        lora_stage(sUp, ldN, up, r, 0, N, sur, sun);
    }
    const int n_tiles = (R + LORA_TM - 1) / LORA_TM;
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int row0 = tile * LORA_TM, wrow = wave * 16;
        for (int idx = tid; idx < LORA_TM * LORA_PS; idx += 256) sP[idx] = 0.f;
        __syncthreads();
        // ---- phase 1: P = x down^T, lanes over k (4 contiguous elements each), one wave reduction per (row, j) and K slice -----------
        for (int k0 = 0; k0 < K; k0 += KS) {
            const int ks = min(KS, K - k0);
            if (!resident) {
                __syncthreads();
                lora_stage(sDown, ldK, down, r, k0, ks, sdr, sdk);
                __syncthreads();
            }
#pragma unroll 1
            for (int g = 0; g < 16; g += ROWS) {
                float acc[ROWS][RT];
#pragma unroll
                for (int i = 0; i < ROWS; ++i)
#pragma unroll
                    for (int j = 0; j < RT; ++j) acc[i][j] = 0.f;
                for (int kk = 4 * lane; kk < ks; kk += 256) {
                    float xv[ROWS][4];
#pragma unroll
                    for (int i = 0; i < ROWS; ++i) {
                        const int row = row0 + wrow + g + i;
                        if (row < R) {
                            load4(x + (size_t)row * ldx + k0 + kk, xv[i]);
#pragma unroll
                            for (int c = 0; c < 4; ++c)
                                if (kk + c >= ks) xv[i][c] = 0.f;      // (the pad columns may hold anything)
                        } else {
#pragma unroll
                            for (int c = 0; c < 4; ++c) xv[i][c] = 0.f;
                        }
                    }
#pragma unroll
                    for (int j = 0; j < RT; ++j) {
                        if (j < r) {
                            const float4 d = *(const float4*)&sDown[j * ldK + kk];
#pragma unroll
                            for (int i = 0; i < ROWS; ++i)
                                acc[i][j] = fmaf(xv[i][3], d.w, fmaf(xv[i][2], d.z, fmaf(xv[i][1], d.y, fmaf(xv[i][0], d.x, acc[i][j]))));
                        }
                    }
                }
                float mine[ROWS];
#pragma unroll
                for (int i = 0; i < ROWS; ++i) mine[i] = 0.f;
#pragma unroll
                for (int j = 0; j < RT; ++j) {
                    if (j < r) {
#pragma unroll
                        for (int i = 0; i < ROWS; ++i) {
                            const float v = wave_sum(acc[i][j]);
                            if (lane == j) mine[i] = v;
                        }
                    }
                }
                if (lane < r) {
#pragma unroll
                    for (int i = 0; i < ROWS; ++i) sP[(wrow + g + i) * LORA_PS + lane] += mine[i];      // (a row belongs to one wave)
                }
            }
        }
        __syncthreads();
        for (int idx = tid; idx < LORA_TM * r; idx += 256) {
            const int row = idx / r, j = idx - row * r;
            if (row0 + row < R) p_out[(size_t)(row0 + row) * r + j] = sP[row * LORA_PS + j];
        }
        // ---- phase 2: y += scale P up^T, lanes over n (4 contiguous columns each), 16 rows per wave against one register copy of up ------
        for (int n0 = 0; n0 < N; n0 += NS) {
            const int ns = min(NS, N - n0);
            if (!resident) {
                __syncthreads();
                lora_stage(sUp, ldN, up, r, n0, ns, sur, sun);
                __syncthreads();
            }
            for (int nn = 4 * lane; nn < ns; nn += 256) {
                float acc[16][4];
#pragma unroll
                for (int i = 0; i < 16; ++i)
#pragma unroll
                    for (int c = 0; c < 4; ++c) acc[i][c] = 0.f;
                for (int jc = 0; jc < r; jc += 16) {
                    float4 u[16];
#pragma unroll
                    for (int j = 0; j < 16; ++j) u[j] = jc + j < r ? *(const float4*)&sUp[(jc + j) * ldN + nn] : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const float* prow = &sP[(wrow + i) * LORA_PS + jc];
#pragma unroll
                        for (int j4 = 0; j4 < 16; j4 += 4) {
                            if (jc + j4 < r) {
                                const float4 p4 = *(const float4*)(prow + j4);      // (entries past r are zero)
                                const float p[4] = {p4.x, p4.y, p4.z, p4.w};
#pragma unroll
                                for (int j = 0; j < 4; ++j) {
                                    acc[i][0] = fmaf(p[j], u[j4 + j].x, acc[i][0]);
                                    acc[i][1] = fmaf(p[j], u[j4 + j].y, acc[i][1]);
                                    acc[i][2] = fmaf(p[j], u[j4 + j].z, acc[i][2]);
                                    acc[i][3] = fmaf(p[j], u[j4 + j].w, acc[i][3]);
                                }
                            }
                        }
                    }
                }
                const int n = n0 + nn;
                const bool whole = nn + 3 < ns;
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int row = row0 + wrow + i;
                    if (row < R) {
                        TY* yp = y + (size_t)row * ldy + n;
                        float yv[4];
                        load4(yp, yv);
                        if (whole) {
#pragma unroll
                            for (int c = 0; c < 4; ++c) yv[c] = fmaf(scale, acc[i][c], yv[c]);
                            store4(yp, yv);
                        } else {
#pragma unroll
                            for (int c = 0; c < 4; ++c)
                                if (nn + c < ns) store1(yp + c, fmaf(scale, acc[i][c], yv[c]));
                        }
                    }
                }
            }
        }
        __syncthreads();
    }
}

template <typename TX, typename TY>
int lora_apply_launch(const void* x, int ldx, const float* down, int64_t sdr, int64_t sdk, const float* up, int64_t sun, int64_t sur, void* y, int ldy,
                      float scale, float* p_out, int R, int K, int N, int r, hipStream_t st) {
    const int Kp = (K + 3) & ~3, Np = (N + 3) & ~3;
    const int resident = r * Kp + r * Np <= LORA_WCAP;
    const int KS = resident ? K : min(Kp, (LORA_WCAP / r) & ~3), NS = resident ? N : min(Np, (LORA_WCAP / r) & ~3);
    const int n_tiles = (R + LORA_TM - 1) / LORA_TM;
    const int grid = min(n_tiles, 512);
    if (r <= 16)
        lora_apply_kernel<TX, TY, 16, 4><<<grid, 256, 0, st>>>((const TX*)x, ldx, down, sdr, sdk, up, sun, sur, (TY*)y, ldy, scale, p_out, R, K, N, r, KS, NS, resident);
    else
        lora_apply_kernel<TX, TY, 64, 1><<<grid, 256, 0, st>>>((const TX*)x, ldx, down, sdr, sdk, up, sun, sur, (TY*)y, ldy, scale, p_out, R, K, N, r, KS, NS, resident);
    return 0;
}

// ---- fm_lora_grad ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void lora_zero_kernel(float* out, int64_t son, int64_t sor, int n, int r) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx < n * r) {
        const int c = idx / r, j = idx - c * r;
        out[c * son + j * sor] = 0.f;
    }
}

// CV columns of a per lane (a wave covers 64 * CV columns), CV * RT accumulators.  blockIdx.x: column chunk, blockIdx.y: row range; the four
// waves take every fourth row of the range, meet in LDS and the workgroup issues one fp32 atomic per output element.
template <typename TA, int RT, int CV>
__global__ __launch_bounds__(256) void lora_grad_kernel(const TA* __restrict__ a, int lda, const float* __restrict__ b, float* out, int64_t son, int64_t sor,
                                                        float scale, int R, int n, int r, int rows_per_wg) {
    __shared__ float sRed[RT * CV * 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int col = blockIdx.x * (64 * CV) + lane * CV;
    const int rbeg = blockIdx.y * rows_per_wg, rend = min(R, rbeg + rows_per_wg);      // (rows >= R are never read)
    for (int idx = tid; idx < RT * CV * 64; idx += 256) sRed[idx] = 0.f;
    float acc[CV][RT];
#pragma unroll
    for (int c = 0; c < CV; ++c)
#pragma unroll
        for (int j = 0; j < RT; ++j) acc[c][j] = 0.f;
    if (col < n) {
        for (int row = rbeg + wave; row < rend; row += 4) {
            float av[CV];
            if constexpr (CV == 4) {
                float t[4];
                load4(a + (size_t)row * lda + col, t);
#pragma unroll
                for (int c = 0; c < 4; ++c) av[c] = col + c < n ? t[c] : 0.f;
            } else {
                if constexpr (sizeof(TA) == 2) av[0] = bf2f(((const bf16_t*)a)[(size_t)row * lda + col]);
                else av[0] = ((const float*)a)[(size_t)row * lda + col];
            }
            const float* brow = b + (size_t)row * r;
#pragma unroll
            for (int j = 0; j < RT; ++j) {
                if (j < r) {
                    const float bj = brow[j];
#pragma unroll
                    for (int c = 0; c < CV; ++c) acc[c][j] = fmaf(av[c], bj, acc[c][j]);
                }
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < RT; ++j)
        if (j < r) {
#pragma unroll
            for (int c = 0; c < CV; ++c) atomicAdd(&sRed[(j * CV + c) * 64 + lane], acc[c][j]);
        }
    __syncthreads();
    for (int idx = tid; idx < r * CV * 64; idx += 256) {
        const int j = idx / (CV * 64), rem = idx - j * (CV * 64), c = rem / 64, l = rem - c * 64;
        const int cc = blockIdx.x * (64 * CV) + l * CV + c;
        if (cc < n) atomicAdd(&out[cc * son + j * sor], scale * sRed[idx]);
    }
}

template <typename TA>
int lora_grad_launch(const void* a, int lda, const float* b, float* out, int64_t son, int64_t sor, float scale, int R, int n, int r, hipStream_t st) {
    const int cv = r <= 16 ? 4 : 1;
    const int chunks = (n + 64 * cv - 1) / (64 * cv);
    int splits = max(1, min((R + 255) / 256, max(1, 512 / chunks)));
    const int rows_per_wg = (R + splits - 1) / splits;
    splits = (R + rows_per_wg - 1) / rows_per_wg;
    const dim3 grid(chunks, splits);
    if (r <= 16) lora_grad_kernel<TA, 16, 4><<<grid, 256, 0, st>>>((const TA*)a, lda, b, out, son, sor, scale, R, n, r, rows_per_wg);
    else lora_grad_kernel<TA, 64, 1><<<grid, 256, 0, st>>>((const TA*)a, lda, b, out, son, sor, scale, R, n, r, rows_per_wg);
    return 0;
}

}  // namespace

extern "C" int fm_lora_apply(const void* x, int ldx, const void* down, int64_t down_sr, int64_t down_sk, const void* up, int64_t up_sn, int64_t up_sr,
                             void* y, int ldy, float scale, void* p_out, int R, int K, int N, int r, int x_f32, int y_f32, void* stream) {
    FM_CHECK_ARG(x && down && up && y && p_out, "fm_lora_apply: null pointer");
    FM_CHECK_ARG(r >= 1 && r <= 64, "fm_lora_apply: rank %d outside 1 .. 64", r);
    FM_CHECK_ARG(R >= 1 && K >= 1 && N >= 1, "fm_lora_apply: R, K, N must be >= 1");
    FM_CHECK_ARG(ldx % 4 == 0 && ldx >= K && ldy % 4 == 0 && ldy >= N, "fm_lora_apply: leading dimensions must be multiples of 4 and cover K / N");
    FM_CHECK_ARG((uintptr_t)x % (x_f32 ? 16 : 8) == 0 && (uintptr_t)y % (y_f32 ? 16 : 8) == 0 && (uintptr_t)down % 4 == 0 && (uintptr_t)up % 4 == 0 &&
                 (uintptr_t)p_out % 4 == 0, "fm_lora_apply: misaligned pointer (x / y: 4 elements)");
    FM_CHECK_ARG(!(x_f32 && !y_f32), "fm_lora_apply: fp32 x with bf16 y is not built");
    hipStream_t st = (hipStream_t)stream;
    const float *d = (const float*)down, *u = (const float*)up;
    if (x_f32) lora_apply_launch<float, float>(x, ldx, d, down_sr, down_sk, u, up_sn, up_sr, y, ldy, scale, (float*)p_out, R, K, N, r, st);
    else if (y_f32) lora_apply_launch<bf16_t, float>(x, ldx, d, down_sr, down_sk, u, up_sn, up_sr, y, ldy, scale, (float*)p_out, R, K, N, r, st);
    else lora_apply_launch<bf16_t, bf16_t>(x, ldx, d, down_sr, down_sk, u, up_sn, up_sr, y, ldy, scale, (float*)p_out, R, K, N, r, st);
    FM_CHECK_LAUNCH("fm_lora_apply");
    return 0;
}

extern "C" int fm_lora_grad(const void* a, int lda, const void* b, void* out, int64_t out_sn, int64_t out_sr, float scale, int accumulate,
                            int R, int n, int r, int a_f32, void* stream) {
    FM_CHECK_ARG(a && b && out, "fm_lora_grad: null pointer");
    FM_CHECK_ARG(r >= 1 && r <= 64, "fm_lora_grad: rank %d outside 1 .. 64", r);
    FM_CHECK_ARG(R >= 1 && n >= 1, "fm_lora_grad: R, n must be >= 1");
    FM_CHECK_ARG(lda % 4 == 0 && lda >= n, "fm_lora_grad: lda must be a multiple of 4 and cover n");
    FM_CHECK_ARG((uintptr_t)a % (a_f32 ? 16 : 8) == 0 && (uintptr_t)b % 4 == 0 && (uintptr_t)out % 4 == 0, "fm_lora_grad: misaligned pointer (a: 4 elements)");
    hipStream_t st = (hipStream_t)stream;
    if (!accumulate) lora_zero_kernel<<<(n * r + 255) / 256, 256, 0, st>>>((float*)out, out_sn, out_sr, n, r);
    if (a_f32) lora_grad_launch<float>(a, lda, (const float*)b, (float*)out, out_sn, out_sr, scale, R, n, r, st);
    else lora_grad_launch<bf16_t>(a, lda, (const float*)b, (float*)out, out_sn, out_sr, scale, R, n, r, st);
    FM_CHECK_LAUNCH("fm_lora_grad");
    return 0;
}
