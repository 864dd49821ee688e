// fp32 compute mode of the diffusion detokenizer (DiVAE decoder): the kernels of csrc/unet.hip once more with f32 feature maps and no bf16
// rounding anywhere, so that the UNet's launch sequence can be held to upstream's fp32 evaluation at fp32 tolerances (compute_precision =
// "fp32" on PatchedUNetCondCat / DiVAE).  Same semantics and index rules as unet.hip; plain kernels like csrc/fp32_verify.hip, not tuned ones:
// every convolution and Linear of this mode is fm_unet_im2col_f32 (3 x 3) + fm_gemm_f32.  The library's accurate expf / sqrtf / division are
// used instead of the fast intrinsics of the bf16 kernels.  Every reduction runs in a fixed order: two runs agree bit for bit.
#include "common.h"
#include "fourm_hip.h"

namespace {

// ------------------------------------------------------------------------------------------------------------------------------------
// im2col: out[(b, oy, ox)][tap * C + c] = in[b][oy * stride + ky - pad][ox * stride + kx - pad][c]   (zero outside), C = C1 + C2,
// in = [src1 | src2]: src1 read at (y >> up1, x >> up1), src2 at (min(floorf(y * sy), H2 - 1), min(floorf(x * sx), W2 - 1)) with
// sy = fp32(H2) / fp32(H), sx = fp32(W2) / fp32(W): F.interpolate(mode="nearest") bit for bit (see unet.hip).  One thread = 4 floats.
// ------------------------------------------------------------------------------------------------------------------------------------
struct Im2colF32Args {
    const float* src1; const float* src2; float* out;
    int ld1, ld2, ldo;
    int B, H, W;            // logical input grid (after the up-sampling of src1)
    int C1, C2, H2, W2;
    int Ho, Wo, ksize, stride, up1;
    int kpad;               // columns [ksize^2 * C, kpad) are written as zeros
    float sy2, sx2;         // (float)H2 / (float)H, (float)W2 / (float)W
};

__global__ __launch_bounds__(256) void im2col_f32_kernel(Im2colF32Args a) {
    const int C = a.C1 + a.C2;
    const int vec_per_row = a.kpad / 4;
    const long long total = (long long)a.B * a.Ho * a.Wo * vec_per_row;
    const int pad = a.ksize / 2;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int v = (int)(i % vec_per_row);
        const long long row = i / vec_per_row;
        const int ox = (int)(row % a.Wo), oy = (int)((row / a.Wo) % a.Ho), b = (int)(row / ((long long)a.Wo * a.Ho));
        const int k = v * 4;
        float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
        if (k < a.ksize * a.ksize * C) {
            const int tap = k / C, c = k % C;            // C1, C2 are multiples of 4: a vector never straddles taps or sources
            const int y = oy * a.stride + tap / a.ksize - pad, x = ox * a.stride + tap % a.ksize - pad;
            if (y >= 0 && y < a.H && x >= 0 && x < a.W) {
                if (c < a.C1) {
                    const int sy = y >> a.up1, sx = x >> a.up1, sw = a.W >> a.up1, sh = a.H >> a.up1;
                    val = *(const float4*)(a.src1 + ((size_t)(b * sh + sy) * sw + sx) * a.ld1 + c);
                } else {
                    const int sy = min((int)floorf((float)y * a.sy2), a.H2 - 1), sx = min((int)floorf((float)x * a.sx2), a.W2 - 1);
                    val = *(const float4*)(a.src2 + ((size_t)(b * a.H2 + sy) * a.W2 + sx) * a.ld2 + (c - a.C1));
                }
            }
        }
        *(float4*)(a.out + (size_t)row * a.ldo + k) = val;
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

// ------------------------------------------------------------------------------------------------------------------------------------
// GroupNorm(G) over (B, HW, C) f32 rows (nn.py:23-25), optional per-(sample, channel) addend in front and SiLU behind.  Workgroup (g, b)
// owns the HW x C / G values of its group and sweeps them three times: sum -> mean; squared deviations about the mean -> rstd (the two-pass
// variance of F.group_norm, no cancellation); normalise, affine, SiLU, store.  Any C / G (element = (row, channel of the group)).
// ------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gn_f32_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ add, int ld_add, const float* __restrict__ w,
                                                     const float* __restrict__ bias, float* __restrict__ y, int ldy, int HW, int C, int G, int silu, float eps) {
    __shared__ float red[4];
    const int g = blockIdx.x, b = blockIdx.y;
    const int cpg = C / G;
    const long long n = (long long)HW * cpg;
    const float* xb = x + (size_t)b * HW * ldx + g * cpg;
    const float* ab = add ? add + (size_t)b * ld_add + g * cpg : nullptr;
    const float inv_n = 1.0f / ((float)HW * (float)cpg);
    float s = 0.f;
    for (long long e = threadIdx.x; e < n; e += 256) {
        const int r = (int)(e / cpg), j = (int)(e % cpg);
        s += xb[(size_t)r * ldx + j] + (ab ? ab[j] : 0.f);
    }
    const float mean = block_sum_256(s, red) * inv_n;
    float q = 0.f;
    for (long long e = threadIdx.x; e < n; e += 256) {
        const int r = (int)(e / cpg), j = (int)(e % cpg);
        const float d = xb[(size_t)r * ldx + j] + (ab ? ab[j] : 0.f) - mean;
        q += d * d;
    }
    const float rstd = 1.0f / sqrtf(block_sum_256(q, red) * inv_n + eps);
    float* yb = y + (size_t)b * HW * ldy + g * cpg;
    for (long long e = threadIdx.x; e < n; e += 256) {
        const int r = (int)(e / cpg), j = (int)(e % cpg);
        float t = (xb[(size_t)r * ldx + j] + (ab ? ab[j] : 0.f) - mean) * rstd * w[g * cpg + j] + bias[g * cpg + j];
        if (silu) t = t / (1.0f + expf(-t));
        yb[(size_t)r * ldy + j] = t;
    }
}

// out = a + b (f32 feature maps: skip_connection(x) + h, x + attention)
__global__ __launch_bounds__(256) void add_f32_kernel(const float* __restrict__ a, int lda, const float* __restrict__ b, int ldb, float* __restrict__ out, int ldo,
                                                      long long rows, int C) {
    const long long total = rows * C;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long row = i / C;
        const int c = (int)(i % C);
        out[(size_t)row * ldo + c] = a[(size_t)row * lda + c] + b[(size_t)row * ldb + c];
    }
}

// y = silu(x): the activation in front of ResBlock.emb_layers / inside time_embed
__global__ __launch_bounds__(256) void silu_f32_kernel(const float* __restrict__ x, float* __restrict__ y, long long n) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const float t = x[i];
        y[i] = t / (1.0f + expf(-t));
    }
}

// [cos(t f_i) | sin(t f_i)], f_i = exp(-ln(max_period) i / half)   (nn.py:120-140); neg_log = fp32(-ln(max_period)) from the host, then
// the operations of upstream's fp32 expression in its order: (neg_log * i) / half, exp, t * f
__global__ void timestep_embedding_f32_kernel(const float* __restrict__ t, float* __restrict__ out, int ldo, int B, int dim, float neg_log) {
    const int half = dim / 2;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * half) return;
    const int b = i / half, j = i % half;
    const float f = expf(neg_log * (float)j / (float)half);
    const float arg = t[b] * f;
    out[(size_t)b * ldo + j] = cosf(arg);
    out[(size_t)b * ldo + half + j] = sinf(arg);
    if ((dim & 1) && j == 0) out[(size_t)b * ldo + dim - 1] = 0.f;
}

// ------------------------------------------------------------------------------------------------------------------------------------
// spatial self-attention of AttentionBlock (QKVAttentionLegacy): qkv rows (B * T, H * 3 * ch) f32 with a head's channels as [q | k | v];
// weight = softmax((q s)(k s)^T), s = ch^-1/4; out rows (B * T, H * ch) f32.  One workgroup per (query, head, sample).
// ------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void unet_attn_f32_kernel(const float* __restrict__ qkv, int ld, float* __restrict__ out, int ldo, int T, int ch, int H) {
    extern __shared__ float sm[];                         // q[ch] | p[T]
    float* qs = sm; float* p = sm + ch;
    __shared__ float red[4];
    const int q = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    const float* base = qkv + (size_t)b * T * ld + (size_t)h * 3 * ch;
    const float scale = 1.0f / sqrtf(sqrtf((float)ch));   // ch^-1/4 on q and on k, as upstream
    for (int d = threadIdx.x; d < ch; d += 256) qs[d] = base[(size_t)q * ld + d] * scale;
    __syncthreads();
    float mx = -INFINITY;
    for (int k = threadIdx.x; k < T; k += 256) {
        const float* kr = base + (size_t)k * ld + ch;
        float s = 0.f;
        for (int d = 0; d < ch; d += 4) {
            const float4 kv = *(const float4*)(kr + d);
            s = fmaf(qs[d], kv.x * scale, s);
            s = fmaf(qs[d + 1], kv.y * scale, s);
            s = fmaf(qs[d + 2], kv.z * scale, s);
            s = fmaf(qs[d + 3], kv.w * scale, s);
        }
        p[k] = s;
        mx = fmaxf(mx, s);
    }
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    float sum = 0.f;
    for (int k = threadIdx.x; k < T; k += 256) { const float e = expf(p[k] - mx); p[k] = e; sum += e; }
    const float inv = 1.0f / block_sum_256(sum, red);     // (its barriers also publish p[] to every thread)
    for (int d = threadIdx.x; d < ch; d += 256) {
        const float* vr = base + 2 * ch + d;
        float o = 0.f;
        for (int k = 0; k < T; ++k) o = fmaf(p[k], vr[(size_t)k * ld], o);
        out[((size_t)b * T + q) * ldo + (size_t)h * ch + d] = o * inv;
    }
}

inline unsigned grid_for(long long total, int block = 256) {
    long long g = (total + block - 1) / block;
    return (unsigned)(g < 1 ? 1 : g > 65535 * 16 ? 65535 * 16 : g);
}

}  // namespace

extern "C" int fm_unet_im2col_f32(const void* src1, int ld1, int C1, const void* src2, int ld2, int C2, int H2, int W2, void* out, int ldo, int kpad,
                                  int B, int H, int W, int ksize, int stride, int up1, void* stream) {
    FM_CHECK_ARG(src1 && out && B > 0 && H > 0 && W > 0, "fm_unet_im2col_f32: bad argument");
    FM_CHECK_ARG(ksize == 1 || ksize == 3, "fm_unet_im2col_f32: ksize=%d (1 or 3)", ksize);
    FM_CHECK_ARG(stride == 1 || stride == 2, "fm_unet_im2col_f32: stride=%d (1 or 2)", stride);
    FM_CHECK_ARG(C1 > 0 && C1 % 4 == 0 && C2 >= 0 && C2 % 4 == 0 && ld1 % 4 == 0 && ld1 >= C1 && (C2 == 0 || (src2 && ld2 % 4 == 0 && ld2 >= C2 && H2 > 0 && W2 > 0)),
                 "fm_unet_im2col_f32: channels / leading dims must be multiples of 4");
    FM_CHECK_ARG(kpad % 4 == 0 && kpad >= ksize * ksize * (C1 + C2) && ldo >= kpad && ldo % 4 == 0, "fm_unet_im2col_f32: kpad=%d ldo=%d too small for %d x %d", kpad, ldo,
                 ksize * ksize, C1 + C2);
    FM_CHECK_ARG(up1 == 0 || (up1 == 1 && H % 2 == 0 && W % 2 == 0), "fm_unet_im2col_f32: up1");
    FM_CHECK_ARG(((uintptr_t)src1 | (uintptr_t)src2 | (uintptr_t)out) % 16 == 0, "fm_unet_im2col_f32: pointers must be 16-byte aligned");
    Im2colF32Args a{};
    a.src1 = (const float*)src1; a.src2 = (const float*)src2; a.out = (float*)out;
    a.ld1 = ld1; a.ld2 = ld2; a.ldo = ldo; a.B = B; a.H = H; a.W = W; a.C1 = C1; a.C2 = C2; a.H2 = C2 ? H2 : 1; a.W2 = C2 ? W2 : 1;
    a.ksize = ksize; a.stride = stride; a.up1 = up1; a.kpad = kpad;
    a.sy2 = (float)a.H2 / (float)H; a.sx2 = (float)a.W2 / (float)W;
    const int pad = ksize / 2;
    a.Ho = (H + 2 * pad - ksize) / stride + 1; a.Wo = (W + 2 * pad - ksize) / stride + 1;
    const long long total = (long long)B * a.Ho * a.Wo * (kpad / 4);
    hipLaunchKernelGGL(im2col_f32_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, a);
    FM_CHECK_LAUNCH("fm_unet_im2col_f32");
    return 0;
}

extern "C" int fm_groupnorm_nhwc_f32(const void* x, int ldx, const void* add, int ld_add, const void* w, const void* b, void* y, int ldy, int B, int HW, int C,
                                     int groups, float eps, int silu, void* stream) {
    FM_CHECK_ARG(x && w && b && y && B > 0 && HW > 0 && C > 0 && groups > 0, "fm_groupnorm_nhwc_f32: bad argument");
    FM_CHECK_ARG(C % groups == 0 && C <= 1024, "fm_groupnorm_nhwc_f32: C=%d groups=%d (C %% groups == 0, C <= 1024)", C, groups);
    FM_CHECK_ARG(ldx >= C && ldy >= C && (!add || ld_add >= C) && B <= 65535, "fm_groupnorm_nhwc_f32: ldx=%d ldy=%d ld_add=%d B=%d", ldx, ldy, ld_add, B);
    hipLaunchKernelGGL(gn_f32_kernel, dim3(groups, B), dim3(256), 0, (hipStream_t)stream, (const float*)x, ldx, (const float*)add, ld_add, (const float*)w, (const float*)b,
                       (float*)y, ldy, HW, C, groups, silu, eps);
    FM_CHECK_LAUNCH("fm_groupnorm_nhwc_f32");
    return 0;
}

extern "C" int fm_add_f32(const void* a, int lda, const void* b, int ldb, void* out, int ldo, int64_t rows, int C, void* stream) {
    FM_CHECK_ARG(a && b && out && rows > 0 && C > 0 && lda >= C && ldb >= C && ldo >= C, "fm_add_f32: bad argument");
    hipLaunchKernelGGL(add_f32_kernel, dim3(grid_for(rows * C)), dim3(256), 0, (hipStream_t)stream, (const float*)a, lda, (const float*)b, ldb, (float*)out, ldo,
                       (long long)rows, C);
    FM_CHECK_LAUNCH("fm_add_f32");
    return 0;
}

extern "C" int fm_silu_f32(const void* x, void* y, int64_t n, void* stream) {
    FM_CHECK_ARG(x && y && n > 0, "fm_silu_f32: bad argument");
    hipLaunchKernelGGL(silu_f32_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, (const float*)x, (float*)y, (long long)n);
    FM_CHECK_LAUNCH("fm_silu_f32");
    return 0;
}

extern "C" int fm_timestep_embedding_f32(const void* t, void* out, int ldo, int B, int dim, float max_period, void* stream) {
    FM_CHECK_ARG(t && out && B > 0 && dim > 1 && ldo >= dim && max_period > 0.f, "fm_timestep_embedding_f32: bad argument");
    const float neg_log = (float)(-log((double)max_period));
    hipLaunchKernelGGL(timestep_embedding_f32_kernel, dim3((B * (dim / 2) + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const float*)t, (float*)out, ldo, B, dim, neg_log);
    FM_CHECK_LAUNCH("fm_timestep_embedding_f32");
    return 0;
}

extern "C" int fm_unet_attention_f32(const void* qkv, int ld, void* out, int ldo, int B, int T, int heads, int ch, void* stream) {
    FM_CHECK_ARG(qkv && out && B > 0 && T > 0 && heads > 0 && ch > 0, "fm_unet_attention_f32: bad argument");
    FM_CHECK_ARG(ch % 4 == 0 && ld % 4 == 0 && (uintptr_t)qkv % 16 == 0, "fm_unet_attention_f32: ch=%d ld=%d (ch %% 4 == 0, ld %% 4 == 0, 16-byte aligned qkv)", ch, ld);
    FM_CHECK_ARG(ld >= heads * 3 * ch && ldo >= heads * ch && heads <= 65535 && B <= 65535, "fm_unet_attention_f32: ld=%d ldo=%d too small for %d heads of %d", ld, ldo, heads, ch);
    const size_t lds = (size_t)(ch + T) * 4;
    FM_CHECK_ARG(lds <= 60 * 1024, "fm_unet_attention_f32: ch + T = %d too large", ch + T);
    hipLaunchKernelGGL(unet_attn_f32_kernel, dim3(T, heads, B), dim3(256), lds, (hipStream_t)stream, (const float*)qkv, ld, (float*)out, ldo, T, ch, heads);
    FM_CHECK_LAUNCH("fm_unet_attention_f32");
    return 0;
}
