// ConvNeXt block behind the tokenizer's ViT decoder (ViTDecoder(out_conv=True): two of them smooth the patch seams of the
// unpatchified image; vq/models/vit_models.py:298-335, :583-584, :655-657):
//
//     y = x + gamma * pwconv2( GELU( pwconv1( LayerNorm_C( dwconv7x7(x) ) ) ) )
//
// depthwise 7 x 7 convolution (zero padding 3, bias), LayerNorm over the channel axis (biased variance, affine), Linear(C, 4C),
// exact (erf) GELU, Linear(4C, C), per-channel layer scale, residual.  The decoder's out_channels is 1 (instance masks) or 3 (RGB):
// C <= 4, so the pointwise MLP of a pixel lives in registers (at most 16 hidden values) and the whole block is ONE launch: a
// workgroup stages a 32 x 8 pixel tile of every channel plus its 3-pixel halo in LDS, a thread owns one pixel.  NCHW fp32 in and
// out, fp32 throughout; memory-bound and tiny next to the decoder blocks.
// With C = 1 LayerNorm returns its bias for every finite input (x - mean(x) = 0), so upstream's block adds a constant and the
// depthwise weights never reach the output; the same formula runs here and gives the same result.
#include "common.h"
#include "fourm_hip.h"

namespace {

constexpr int CN_TW = 32, CN_TH = 8, CN_HALO = 3;
constexpr int CN_LW = CN_TW + 2 * CN_HALO, CN_LH = CN_TH + 2 * CN_HALO;

struct ConvNextArgs {
    const float* x; float* y;
    const float* dw_w; const float* dw_b; const float* ln_w; const float* ln_b;
    const float* w1; const float* b1; const float* w2; const float* b2; const float* gamma;
    int H, W;
    float eps;
};

template <int C>
__global__ __launch_bounds__(256) void convnext_block_kernel(ConvNextArgs a) {
    __shared__ float tile[C][CN_LH][CN_LW + 1];
    const int H = a.H, W = a.W;
    const int x0 = blockIdx.x * CN_TW, y0 = blockIdx.y * CN_TH;
    const size_t img = (size_t)blockIdx.z * C * H * W;
    for (int i = threadIdx.x; i < C * CN_LH * CN_LW; i += 256) {
        const int c = i / (CN_LH * CN_LW), ly = (i / CN_LW) % CN_LH, lx = i % CN_LW;
        const int gy = y0 + ly - CN_HALO, gx = x0 + lx - CN_HALO;
        tile[c][ly][lx] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? a.x[img + ((size_t)c * H + gy) * W + gx] : 0.f;      // zero padding
    }
    __syncthreads();
    const int tx = threadIdx.x % CN_TW, ty = threadIdx.x / CN_TW;
    const int px = x0 + tx, py = y0 + ty;
    if (px >= W || py >= H) return;
    // depthwise 7 x 7 (cross-correlation, like nn.Conv2d): rows first, then columns, one fmaf chain per channel
    float d[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        float s = a.dw_b[c];
#pragma unroll
        for (int ky = 0; ky < 7; ++ky)
#pragma unroll
            for (int kx = 0; kx < 7; ++kx) s = fmaf(a.dw_w[(c * 7 + ky) * 7 + kx], tile[c][ty + ky][tx + kx], s);
        d[c] = s;
    }
    // LayerNorm over the C channels of the pixel
    float mean = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) mean += d[c];
    mean *= 1.0f / C;
    float var = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) { const float t = d[c] - mean; var = fmaf(t, t, var); }
    const float rstd = 1.0f / sqrtf(var * (1.0f / C) + a.eps);
    float n[C];
#pragma unroll
    for (int c = 0; c < C; ++c) n[c] = fmaf((d[c] - mean) * rstd, a.ln_w[c], a.ln_b[c]);
    // Linear(C, 4C) + GELU + Linear(4C, C)
    float o[C];
#pragma unroll
    for (int c = 0; c < C; ++c) o[c] = a.b2[c];
#pragma unroll
    for (int k = 0; k < 4 * C; ++k) {
        float h = a.b1[k];
#pragma unroll
        for (int c = 0; c < C; ++c) h = fmaf(a.w1[k * C + c], n[c], h);
        const float g = 0.5f * h * (1.0f + erff(h * 0.70710678118654752f));
#pragma unroll
        for (int c = 0; c < C; ++c) o[c] = fmaf(a.w2[c * 4 * C + k], g, o[c]);
    }
#pragma unroll
    for (int c = 0; c < C; ++c)
        a.y[img + ((size_t)c * H + py) * W + px] = fmaf(a.gamma[c], o[c], tile[c][ty + CN_HALO][tx + CN_HALO]);
}

}  // namespace

extern "C" int fm_convnext_block(const void* x, void* y, const void* dw_weight, const void* dw_bias, const void* ln_weight, const void* ln_bias,
                                 const void* pw1_weight, const void* pw1_bias, const void* pw2_weight, const void* pw2_bias, const void* gamma,
                                 int B, int C, int H, int W, float eps, void* stream) {
    FM_CHECK_ARG(x && y && dw_weight && dw_bias && ln_weight && ln_bias && pw1_weight && pw1_bias && pw2_weight && pw2_bias && gamma,
                 "fm_convnext_block: null pointer");
    FM_CHECK_ARG(x != y, "fm_convnext_block: in place is not supported (the halo of a tile is another tile's output)");
    FM_CHECK_ARG(C >= 1 && C <= FM_CONVNEXT_MAX_C, "fm_convnext_block: C=%d unsupported (1 <= C <= %d: the pointwise MLP is held in registers)", C, FM_CONVNEXT_MAX_C);
    FM_CHECK_ARG(B > 0 && B <= 65535 && H > 0 && W > 0 && (H + CN_TH - 1) / CN_TH <= 65535 && eps >= 0.f, "fm_convnext_block: bad shape");
    ConvNextArgs a{(const float*)x, (float*)y, (const float*)dw_weight, (const float*)dw_bias, (const float*)ln_weight, (const float*)ln_bias,
                   (const float*)pw1_weight, (const float*)pw1_bias, (const float*)pw2_weight, (const float*)pw2_bias, (const float*)gamma, H, W, eps};
    const dim3 grid((W + CN_TW - 1) / CN_TW, (H + CN_TH - 1) / CN_TH, B);
    hipStream_t s = (hipStream_t)stream;
    switch (C) {
        case 1: hipLaunchKernelGGL(convnext_block_kernel<1>, grid, dim3(256), 0, s, a); break;
        case 2: hipLaunchKernelGGL(convnext_block_kernel<2>, grid, dim3(256), 0, s, a); break;
        case 3: hipLaunchKernelGGL(convnext_block_kernel<3>, grid, dim3(256), 0, s, a); break;
        default: hipLaunchKernelGGL(convnext_block_kernel<4>, grid, dim3(256), 0, s, a); break;
    }
    FM_CHECK_LAUNCH("fm_convnext_block");
    return 0;
}
