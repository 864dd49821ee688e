// Backward of the fp32 compute mode of the diffusion detokenizer (csrc/unet_f32.hip): what a training step of the UNet on a frozen encoder needs
// besides fm_gemm_f32 (dX = dY W and dW = dY^T X are that kernel through its strides).  The adjoint of the 3 x 3 im2col, the backward of
// GroupNorm (+ addend, + SiLU), of the spatial self-attention and of SiLU.  Plain kernels like their forward counterparts: the library's
// accurate expf / sqrtf / division, every reduction in a fixed order and every output element written by exactly one thread (a gather where the
// forward scatters) - two runs agree bit for bit.  Verification mode: not tuned, no throughput claim.
#include "common.h"
#include "fourm_hip.h"

namespace {

// ------------------------------------------------------------------------------------------------------------------------------------
// col2im: the adjoint of im2col_f32_kernel with respect to src1 (3 x 3, C2 = 0).  Gather form: one thread owns 4 channels of one SOURCE pixel
// (b, sy, sx) and sums, in the fixed order (up-sampled pixel y, x; tap ky, kx), every col[(b, oy, ox)][tap * C + c] the forward filled from it:
// oy * stride + ky - 1 = y, 0 <= oy < Ho.  At most 9 terms, 36 with up1 (a source pixel is four pixels of the (H, W) grid).
// ------------------------------------------------------------------------------------------------------------------------------------
struct Col2imF32Args {
    const float* col; float* dsrc;
    int ldc, ld;
    int B, H, W, C;         // (H, W): the logical input grid of the forward (after the up-sampling of src1)
    int Ho, Wo, stride, up1, accumulate;
};

__global__ __launch_bounds__(256) void col2im_f32_kernel(Col2imF32Args a) {
    const int vec_per_row = a.C / 4;
    const int sh = a.H >> a.up1, sw = a.W >> a.up1, rep = 1 << a.up1;
    const long long total = (long long)a.B * sh * sw * vec_per_row;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int c = (int)(i % vec_per_row) * 4;
        const long long pix = i / vec_per_row;
        const int sx = (int)(pix % sw), sy = (int)((pix / sw) % sh), b = (int)(pix / ((long long)sw * sh));
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int uy = 0; uy < rep; ++uy)
            for (int ux = 0; ux < rep; ++ux) {
                const int y = sy * rep + uy, x = sx * rep + ux;
                for (int ky = 0; ky < 3; ++ky) {
                    const int ty = y + 1 - ky;
                    if (ty < 0 || ty % a.stride) continue;
                    const int oy = ty / a.stride;
                    if (oy >= a.Ho) continue;
                    for (int kx = 0; kx < 3; ++kx) {
                        const int tx = x + 1 - kx;
                        if (tx < 0 || tx % a.stride) continue;
                        const int ox = tx / a.stride;
                        if (ox >= a.Wo) continue;
                        const float4 v = *(const float4*)(a.col + ((size_t)(b * a.Ho + oy) * a.Wo + ox) * a.ldc + (ky * 3 + kx) * a.C + c);
                        s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
                    }
                }
            }
        float4* dst = (float4*)(a.dsrc + (size_t)pix * a.ld + c);
        if (a.accumulate) { const float4 o = *dst; s.x += o.x; s.y += o.y; s.z += o.z; s.w += o.w; }
        *dst = s;
    }
}

// sum over the 256 threads of a workgroup in a fixed order (wave butterfly, then the four waves left to right)
__device__ __forceinline__ float block_sum_256(float v, float* red) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

__device__ __forceinline__ float silu_grad(float t) {
    const float s = 1.0f / (1.0f + expf(-t));
    return s * (1.0f + t * (1.0f - s));
}

// ------------------------------------------------------------------------------------------------------------------------------------
// GroupNorm backward.  Workgroup (g, b) as in gn_f32_kernel; z = x + add, xh = (z - mean) rstd, t = xh w + bias, y = [silu] t.
//   g_ = dy [silu'(t)];  per channel over HW: cg = sum g_, cgx = sum g_ xh  (-> the per-sample partial sums of db, dw in scratch);
//   m1 = sum_j w_j cg_j / n, m2 = sum_j w_j cgx_j / n;  dx = rstd (g_ w - m1 - xh m2);  dadd[b][c] = sum_HW dx.
// mean and rstd are recomputed exactly as the forward computes them.  Threads are laid out (row lane, channel lane): a channel's sum over HW is
// the sum of its row lanes' partial sums, taken in order by one thread.
// ------------------------------------------------------------------------------------------------------------------------------------
struct GnBwdF32Args {
    const float* dy; const float* x; const float* add; const float* w; const float* bias;
    float* dx; float* dadd; float* part_dw; float* part_db;      // part_*: (B, C) per-sample partial sums, or NULL
    int lddy, ldx, ld_add, lddx, ld_dadd;
    int HW, C, G, silu;
    float eps;
};

// channel sums of this thread's rows -> the channel's total, left in tot[j] by the channel's first row lane (callers separate uses by barriers)
__device__ __forceinline__ void channel_total(float v, float* part, float* tot, int j, int rl, int lpr, int nrl, bool valid) {
    __syncthreads();
    part[threadIdx.x] = v;
    __syncthreads();
    if (valid && rl == 0) {
        float s = 0.f;
        for (int k = 0; k < nrl; ++k) s += part[k * lpr + (int)(threadIdx.x)];
        tot[j] = s;
    }
}

__global__ __launch_bounds__(256) void gn_bwd_f32_kernel(GnBwdF32Args a) {
    __shared__ float red[4];
    __shared__ float part[256];
    __shared__ float cg[1024], cgx[1024];                         // per-channel sums of the group (cpg <= C <= 1024)
    const int g = blockIdx.x, b = blockIdx.y;
    const int cpg = a.C / a.G, HW = a.HW;
    const long long n = (long long)HW * cpg;
    const float* xb = a.x + (size_t)b * HW * a.ldx + g * cpg;
    const float* dyb = a.dy + (size_t)b * HW * a.lddy + g * cpg;
    const float* ab = a.add ? a.add + (size_t)b * a.ld_add + g * cpg : nullptr;
    const float* wg = a.w + g * cpg;
    const float* bg = a.bias + g * cpg;
    const float inv_n = 1.0f / ((float)HW * (float)cpg);
    // the forward's statistics, in the forward's order
    float s = 0.f;
    for (long long e = threadIdx.x; e < n; e += 256) {
        const int r = (int)(e / cpg), j = (int)(e % cpg);
        s += xb[(size_t)r * a.ldx + j] + (ab ? ab[j] : 0.f);
    }
    const float mean = block_sum_256(s, red) * inv_n;
    float q = 0.f;
    for (long long e = threadIdx.x; e < n; e += 256) {
        const int r = (int)(e / cpg), j = (int)(e % cpg);
        const float d = xb[(size_t)r * a.ldx + j] + (ab ? ab[j] : 0.f) - mean;
        q += d * d;
    }
    const float rstd = 1.0f / sqrtf(block_sum_256(q, red) * inv_n + a.eps);
    // (row lane, channel lane) layout
    const int lpr = cpg < 256 ? cpg : 256, nrl = 256 / lpr;
    const int jl = threadIdx.x % lpr, rl = threadIdx.x / lpr;
    const int chunks = (cpg + lpr - 1) / lpr;
    for (int jc = 0; jc < chunks; ++jc) {
        const int j = jc * lpr + jl;
        const bool valid = rl < nrl && j < cpg;
        float sg = 0.f, sgx = 0.f;
        if (valid) {
            const float wj = wg[j], bj = bg[j], aj = ab ? ab[j] : 0.f;
            for (int r = rl; r < HW; r += nrl) {
                const float xh = (xb[(size_t)r * a.ldx + j] + aj - mean) * rstd;
                float gg = dyb[(size_t)r * a.lddy + j];
                if (a.silu) gg *= silu_grad(xh * wj + bj);
                sg += gg;
                sgx += gg * xh;
            }
        }
        channel_total(sg, part, cg, j, rl, lpr, nrl, valid);
        channel_total(sgx, part, cgx, j, rl, lpr, nrl, valid);
    }
    __syncthreads();
    float p1 = 0.f, p2 = 0.f;
    for (int j = threadIdx.x; j < cpg; j += 256) {
        p1 += wg[j] * cg[j];
        p2 += wg[j] * cgx[j];
        if (a.part_db) a.part_db[(size_t)b * a.C + g * cpg + j] = cg[j];
        if (a.part_dw) a.part_dw[(size_t)b * a.C + g * cpg + j] = cgx[j];
    }
    const float m1 = block_sum_256(p1, red) * inv_n;
    const float m2 = block_sum_256(p2, red) * inv_n;
    float* dxb = a.dx + (size_t)b * HW * a.lddx + g * cpg;
    for (int jc = 0; jc < chunks; ++jc) {
        const int j = jc * lpr + jl;
        const bool valid = rl < nrl && j < cpg;
        float sd = 0.f;
        if (valid) {
            const float wj = wg[j], bj = bg[j], aj = ab ? ab[j] : 0.f;
            for (int r = rl; r < HW; r += nrl) {
                const float xh = (xb[(size_t)r * a.ldx + j] + aj - mean) * rstd;
                float gg = dyb[(size_t)r * a.lddy + j];
                if (a.silu) gg *= silu_grad(xh * wj + bj);
                const float d = rstd * (gg * wj - m1 - xh * m2);
                dxb[(size_t)r * a.lddx + j] = d;
                sd += d;
            }
        }
        if (a.dadd) {                                             // (uniform over the workgroup)
            channel_total(sd, part, cg, j, rl, lpr, nrl, valid);
            if (valid && rl == 0) a.dadd[(size_t)b * a.ld_dadd + g * cpg + j] = cg[j];
        }
    }
}

// dw[c] = sum_b part_dw[b][c], db[c] = sum_b part_db[b][c], samples in order
__global__ __launch_bounds__(256) void gn_bwd_combine_f32_kernel(const float* __restrict__ part_dw, const float* __restrict__ part_db, float* __restrict__ dw,
                                                                 float* __restrict__ db, int B, int C) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    float sw = 0.f, sb = 0.f;
    for (int b = 0; b < B; ++b) {
        if (dw) sw += part_dw[(size_t)b * C + c];
        if (db) sb += part_db[(size_t)b * C + c];
    }
    if (dw) dw[c] = sw;
    if (db) db[c] = sb;
}

// ------------------------------------------------------------------------------------------------------------------------------------
// Backward of unet_attn_f32_kernel.  S[t][s] = (q_t sc) . (k_s sc), P = softmax_s S, O = P V, sc = ch^-1/4:
//   dP[t][s] = dO_t . v_s,  D_t = sum_s P[t][s] dP[t][s],  dS = P (dP - D);
//   dq_t = sc sum_s dS[t][s] (k_s sc),  dk_s = sc sum_t dS[t][s] (q_t sc),  dv_s = sum_t P[t][s] dO_t.
// Two kernels, each a gather: one workgroup per QUERY recomputes its row of P as the forward does, writes dq_t and leaves (row max, row sum,
// D_t) in scratch; one workgroup per KEY rebuilds its column of P and dS from those and writes dk_s and dv_s.  The score is the forward's
// fmaf chain over the channels in both, so both see the forward's probabilities.
// ------------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float dot_scaled(const float* __restrict__ lds_vec, const float* __restrict__ row, int ch, float scale) {
    float s = 0.f;
    for (int d = 0; d < ch; d += 4) {
        const float4 v = *(const float4*)(row + d);
        s = fmaf(lds_vec[d], v.x * scale, s);
        s = fmaf(lds_vec[d + 1], v.y * scale, s);
        s = fmaf(lds_vec[d + 2], v.z * scale, s);
        s = fmaf(lds_vec[d + 3], v.w * scale, s);
    }
    return s;
}

__global__ __launch_bounds__(256) void unet_attn_bwd_q_f32_kernel(const float* __restrict__ qkv, int ld, const float* __restrict__ dout, int lddo, float* __restrict__ dqkv,
                                                                  int lddqkv, float* __restrict__ stats, int T, int ch, int H) {
    extern __shared__ __attribute__((aligned(16))) float sm[];   // red[4] | q sc [ch] | dO_t [ch] | p[T] | dP -> dS [T]
    float* red = sm; float* qs = sm + 4; float* dos = qs + ch; float* p = dos + ch; float* dp = p + T;
    const int q = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    const float* base = qkv + (size_t)b * T * ld + (size_t)h * 3 * ch;
    const float scale = 1.0f / sqrtf(sqrtf((float)ch));
    for (int d = threadIdx.x; d < ch; d += 256) {
        qs[d] = base[(size_t)q * ld + d] * scale;
        dos[d] = dout[((size_t)b * T + q) * lddo + (size_t)h * ch + d];
    }
    __syncthreads();
    float mx = -INFINITY;
    for (int k = threadIdx.x; k < T; k += 256) {
        const float s = dot_scaled(qs, base + (size_t)k * ld + ch, ch, scale);
        p[k] = s;
        mx = fmaxf(mx, s);
        dp[k] = dot_scaled(dos, base + (size_t)k * ld + 2 * ch, ch, 1.0f);
    }
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    float sum = 0.f;
    for (int k = threadIdx.x; k < T; k += 256) { const float e = expf(p[k] - mx); p[k] = e; sum += e; }
    const float l = block_sum_256(sum, red);
    const float inv = 1.0f / l;
    float dsum = 0.f;
    for (int k = threadIdx.x; k < T; k += 256) { p[k] *= inv; dsum += p[k] * dp[k]; }
    const float D = block_sum_256(dsum, red);
    for (int k = threadIdx.x; k < T; k += 256) dp[k] = p[k] * (dp[k] - D);
    __syncthreads();
    for (int d = threadIdx.x; d < ch; d += 256) {
        const float* kr = base + ch + d;
        float o = 0.f;
        for (int k = 0; k < T; ++k) o = fmaf(dp[k], kr[(size_t)k * ld] * scale, o);
        dqkv[((size_t)b * T + q) * lddqkv + (size_t)h * 3 * ch + d] = o * scale;
    }
    if (threadIdx.x == 0) {
        float* st = stats + (((size_t)b * H + h) * T + q) * 3;
        st[0] = mx; st[1] = l; st[2] = D;
    }
}

__global__ __launch_bounds__(256) void unet_attn_bwd_kv_f32_kernel(const float* __restrict__ qkv, int ld, const float* __restrict__ dout, int lddo, float* __restrict__ dqkv,
                                                                   int lddqkv, const float* __restrict__ stats, int T, int ch, int H) {
    extern __shared__ __attribute__((aligned(16))) float sm[];   // red[4] (unused, keeps the layout) | k sc [ch] | v [ch] | p[T] | dS[T]
    float* ks = sm + 4; float* vs = ks + ch; float* p = vs + ch; float* ds = p + T;
    const int k = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    const float* base = qkv + (size_t)b * T * ld + (size_t)h * 3 * ch;
    const float* dob = dout + (size_t)b * T * lddo + (size_t)h * ch;
    const float* st = stats + ((size_t)b * H + h) * T * 3;
    const float scale = 1.0f / sqrtf(sqrtf((float)ch));
    for (int d = threadIdx.x; d < ch; d += 256) {
        ks[d] = base[(size_t)k * ld + ch + d] * scale;
        vs[d] = base[(size_t)k * ld + 2 * ch + d];
    }
    __syncthreads();
    for (int t = threadIdx.x; t < T; t += 256) {
        // (q_t sc) . (k_s sc) with the forward's operands: lds_vec * (row * scale) = (k sc) * (q sc)
        const float s = dot_scaled(ks, base + (size_t)t * ld, ch, scale);
        const float pt = expf(s - st[t * 3]) * (1.0f / st[t * 3 + 1]);
        const float dpt = dot_scaled(vs, dob + (size_t)t * lddo, ch, 1.0f);
        p[t] = pt;
        ds[t] = pt * (dpt - st[t * 3 + 2]);
    }
    __syncthreads();
    float* out = dqkv + ((size_t)b * T + k) * lddqkv + (size_t)h * 3 * ch;
    for (int d = threadIdx.x; d < ch; d += 256) {
        float dk = 0.f, dv = 0.f;
        for (int t = 0; t < T; ++t) {
            dk = fmaf(ds[t], base[(size_t)t * ld + d] * scale, dk);
            dv = fmaf(p[t], dob[(size_t)t * lddo + d], dv);
        }
        out[ch + d] = dk * scale;
        out[2 * ch + d] = dv;
    }
}

// dx = dy silu'(x)
__global__ __launch_bounds__(256) void silu_bwd_f32_kernel(const float* __restrict__ dy, const float* __restrict__ x, float* __restrict__ dx, long long n) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) dx[i] = dy[i] * silu_grad(x[i]);
}

inline unsigned grid_for(long long total, int block = 256) {
    long long g = (total + block - 1) / block;
    return (unsigned)(g < 1 ? 1 : g > 65535 * 16 ? 65535 * 16 : g);
}

}  // namespace

extern "C" int fm_unet_col2im_f32(const void* col, int ldc, void* dsrc, int ld, int C, int B, int H, int W, int ksize, int stride, int up1, int accumulate, void* stream) {
    FM_CHECK_ARG(col && dsrc && B > 0 && H > 0 && W > 0, "fm_unet_col2im_f32: bad argument");
    FM_CHECK_ARG(ksize == 3, "fm_unet_col2im_f32: ksize=%d (3: a ksize-1 im2col is a copy, its adjoint a view)", ksize);
    FM_CHECK_ARG(stride == 1 || stride == 2, "fm_unet_col2im_f32: stride=%d (1 or 2)", stride);
    FM_CHECK_ARG(C > 0 && C % 4 == 0 && ld % 4 == 0 && ld >= C && ldc % 4 == 0 && ldc >= 9 * C, "fm_unet_col2im_f32: C=%d ld=%d ldc=%d (multiples of 4, ld >= C, ldc >= 9 C)", C, ld, ldc);
    FM_CHECK_ARG(up1 == 0 || (up1 == 1 && H % 2 == 0 && W % 2 == 0), "fm_unet_col2im_f32: up1");
    FM_CHECK_ARG(accumulate == 0 || accumulate == 1, "fm_unet_col2im_f32: accumulate=%d (0 or 1)", accumulate);
    FM_CHECK_ARG(((uintptr_t)col | (uintptr_t)dsrc) % 16 == 0, "fm_unet_col2im_f32: pointers must be 16-byte aligned");
    Col2imF32Args a{};
    a.col = (const float*)col; a.dsrc = (float*)dsrc; a.ldc = ldc; a.ld = ld; a.B = B; a.H = H; a.W = W; a.C = C;
    a.Ho = (H + 2 - 3) / stride + 1; a.Wo = (W + 2 - 3) / stride + 1; a.stride = stride; a.up1 = up1; a.accumulate = accumulate;
    FM_CHECK_ARG((long long)B * a.Ho * a.Wo <= 0x7fffffffLL && (long long)B * H * W <= 0x7fffffffLL, "fm_unet_col2im_f32: too many pixels");
    const long long total = (long long)B * (H >> up1) * (W >> up1) * (C / 4);
    hipLaunchKernelGGL(col2im_f32_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, a);
    FM_CHECK_LAUNCH("fm_unet_col2im_f32");
    return 0;
}

extern "C" int fm_groupnorm_nhwc_bwd_f32(const void* dy, int lddy, const void* x, int ldx, const void* add, int ld_add, const void* w, const void* b, void* dx, int lddx,
                                         void* dw, void* db, void* dadd, int ld_dadd, void* scratch, int B, int HW, int C, int groups, float eps, int silu, void* stream) {
    FM_CHECK_ARG(dy && x && w && b && dx && B > 0 && HW > 0 && C > 0 && groups > 0, "fm_groupnorm_nhwc_bwd_f32: bad argument");
    FM_CHECK_ARG(C % groups == 0 && C <= 1024, "fm_groupnorm_nhwc_bwd_f32: C=%d groups=%d (C %% groups == 0, C <= 1024)", C, groups);
    FM_CHECK_ARG(lddy >= C && ldx >= C && lddx >= C && (!add || ld_add >= C) && (!dadd || ld_dadd >= C) && B <= 65535,
                 "fm_groupnorm_nhwc_bwd_f32: lddy=%d ldx=%d lddx=%d ld_add=%d ld_dadd=%d B=%d", lddy, ldx, lddx, ld_add, ld_dadd, B);
    FM_CHECK_ARG(!(dw || db) || scratch, "fm_groupnorm_nhwc_bwd_f32: dw / db need the scratch of 2 * B * C floats");
    GnBwdF32Args a{};
    a.dy = (const float*)dy; a.x = (const float*)x; a.add = (const float*)add; a.w = (const float*)w; a.bias = (const float*)b;
    a.dx = (float*)dx; a.dadd = (float*)dadd;
    a.part_dw = dw ? (float*)scratch : nullptr;
    a.part_db = db ? (float*)scratch + (size_t)B * C : nullptr;
    a.lddy = lddy; a.ldx = ldx; a.ld_add = ld_add; a.lddx = lddx; a.ld_dadd = ld_dadd; a.HW = HW; a.C = C; a.G = groups; a.silu = silu; a.eps = eps;
    hipLaunchKernelGGL(gn_bwd_f32_kernel, dim3(groups, B), dim3(256), 0, (hipStream_t)stream, a);
    FM_CHECK_LAUNCH("fm_groupnorm_nhwc_bwd_f32");
    if (dw || db) {
        hipLaunchKernelGGL(gn_bwd_combine_f32_kernel, dim3((C + 255) / 256), dim3(256), 0, (hipStream_t)stream, a.part_dw, a.part_db, (float*)dw, (float*)db, B, C);
        FM_CHECK_LAUNCH("fm_groupnorm_nhwc_bwd_f32");
    }
    return 0;
}

extern "C" int fm_unet_attention_bwd_f32(const void* qkv, int ld, const void* dout, int lddo, void* dqkv, int lddqkv, void* scratch, int B, int T, int heads, int ch,
                                         void* stream) {
    FM_CHECK_ARG(qkv && dout && dqkv && scratch && B > 0 && T > 0 && heads > 0 && ch > 0, "fm_unet_attention_bwd_f32: bad argument");
    FM_CHECK_ARG(ch % 4 == 0 && ld % 4 == 0 && lddo % 4 == 0 && ((uintptr_t)qkv | (uintptr_t)dout) % 16 == 0,
                 "fm_unet_attention_bwd_f32: ch=%d ld=%d lddo=%d (multiples of 4, 16-byte aligned qkv and dout)", ch, ld, lddo);
    FM_CHECK_ARG(ld >= heads * 3 * ch && lddqkv >= heads * 3 * ch && lddo >= heads * ch && heads <= 65535 && B <= 65535,
                 "fm_unet_attention_bwd_f32: ld=%d lddqkv=%d lddo=%d too small for %d heads of %d", ld, lddqkv, lddo, heads, ch);
    FM_CHECK_ARG((size_t)(ch + T) * 4 <= 60 * 1024, "fm_unet_attention_bwd_f32: ch + T = %d too large", ch + T);
    const size_t lds = (size_t)(4 + 2 * ch + 2 * T) * 4;          // twice the forward's rows: <= 120 KB of the 160 KB of a gfx950 CU
    if (lds > 64 * 1024) {
        FM_CHECK_ARG(hipFuncSetAttribute((const void*)unet_attn_bwd_q_f32_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess &&
                     hipFuncSetAttribute((const void*)unet_attn_bwd_kv_f32_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess,
                     "fm_unet_attention_bwd_f32: %zu bytes of LDS refused by the runtime", lds);
    }
    hipLaunchKernelGGL(unet_attn_bwd_q_f32_kernel, dim3(T, heads, B), dim3(256), lds, (hipStream_t)stream, (const float*)qkv, ld, (const float*)dout, lddo, (float*)dqkv, lddqkv,
                       (float*)scratch, T, ch, heads);
    FM_CHECK_LAUNCH("fm_unet_attention_bwd_f32");
    hipLaunchKernelGGL(unet_attn_bwd_kv_f32_kernel, dim3(T, heads, B), dim3(256), lds, (hipStream_t)stream, (const float*)qkv, ld, (const float*)dout, lddo, (float*)dqkv, lddqkv,
                       (const float*)scratch, T, ch, heads);
    FM_CHECK_LAUNCH("fm_unet_attention_bwd_f32");
    return 0;
}

extern "C" int fm_silu_bwd_f32(const void* dy, const void* x, void* dx, int64_t n, void* stream) {
    FM_CHECK_ARG(dy && x && dx && n > 0, "fm_silu_bwd_f32: bad argument");
    hipLaunchKernelGGL(silu_bwd_f32_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, (const float*)dy, (const float*)x, (float*)dx, (long long)n);
    FM_CHECK_LAUNCH("fm_silu_bwd_f32");
    return 0;
}
