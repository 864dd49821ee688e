// Dense front end of FourMViT (fourm/models/fm_vit.py): every patch of every image, in grid order, as rows of the patch-projection GEMM,
// and the (position + modality) embedding rows that GEMM's residual epilogue adds onto.
//
// fm_select_embed (select_embed.hip) gathers ONE selected patch per wave with a lane stride over features, channel fastest: neighbouring
// lanes read pixels of different channel planes.  That is the shape of the pre-training step (a handful of RGB patches per sample).  Here
// all patches are taken, so a workgroup owns a strip of S horizontally adjacent patches of one image:
//   read  : for every (channel, row inside the patch) one segment of S * P pixels, contiguous along W, 16 bytes per lane where P and W
//           allow it, into an fp32 LDS tile [c][py][x] (the store is contiguous too: no bank conflicts);
//   write : the S output rows of the strip are adjacent in memory (S * ld elements).  A lane builds one 16-byte chunk - 8 bf16 or 4 fp32
//           consecutive features f = (py * P + px) * C + c - from scalar LDS reads and stores it; consecutive lanes store consecutive
//           chunks.  The LDS stores are 16 bytes per lane on consecutive addresses (conflict-free); the scalar LDS reads of one
//           instruction step by 8 / C (4 / C) pixels inside a plane, which for C = 3, P = 16 puts up to 3 lanes of a 32-lane group
//           on one bank - about 500 LDS cycles per strip against ~4000 cycles of its HBM traffic, so the kernel stays
//           bound by memory.  Planes are padded by 4 floats so that the channels start 4 banks apart.
// The kernel only moves and rounds (float -> bf16 round-to-nearest-even, as torch's .to(bfloat16)).
#include "common.h"
#include "fourm_hip.h"

namespace {

constexpr int VIT_LDS_FLOATS = 8192;      // 32 KB tile: S * P * P * C <= 8192

template <bool F32, bool VEC>
__global__ __launch_bounds__(256) void vit_patch_rows_kernel(const float* __restrict__ px, void* __restrict__ rows, int ld, int C, int H, int W, int P,
                                                             int S, int nstrips) {
    __shared__ __attribute__((aligned(16))) float tile[VIT_LDS_FLOATS + 64];       // + plane padding (4 floats for up to 16 channels)
    const int gw = W / P, gh = H / P;
    int bid = blockIdx.x;
    const int strip = bid % nstrips; bid /= nstrips;
    const int gy = bid % gh;
    const int b = bid / gh;
    const int gx0 = strip * S;
    const int Sn = min(S, gw - gx0);              // patches of this strip
    if (Sn <= 0) return;                          // (uniform per workgroup: taken before any barrier)
    const int SW = Sn * P;                        // pixels per image-row segment
    const int plane = P * SW + (C <= 16 ? 4 : 0);  // floats per channel plane (padded: planes start 4 banks apart, still 16-byte aligned)
    const float* img = px + (size_t)b * C * H * W + (size_t)(gy * P) * W + gx0 * P;
    // ---- image -> LDS -------------------------------------------------------------------------------------------------------------
    if constexpr (VEC) {
        const int q4 = SW >> 2, total = C * P * q4;
        for (int i = threadIdx.x; i < total; i += 256) {
            const int x4 = i % q4, r = i / q4, py = r % P, c = r / P;
            const float4 v = *(const float4*)(img + ((size_t)c * H + py) * W + x4 * 4);
            *(float4*)(tile + c * plane + py * SW + x4 * 4) = v;
        }
    } else {
        const int total = C * P * SW;
        for (int i = threadIdx.x; i < total; i += 256) {
            const int x = i % SW, r = i / SW, py = r % P, c = r / P;
            tile[c * plane + py * SW + x] = img[((size_t)c * H + py) * W + x];
        }
    }
    __syncthreads();
    // ---- LDS -> rows: 16-byte chunks, pad columns zero -------------------------------------------------------------------------------
    constexpr int EPC = F32 ? 4 : 8;              // elements per 16-byte chunk
    const int live = P * P * C, cpr = ld / EPC;
    const size_t row0 = ((size_t)b * gh + gy) * gw + gx0;
    for (int q = threadIdx.x; q < Sn * cpr; q += 256) {
        const int s = q / cpr, ch = q % cpr;
        int f = ch * EPC;
        int c = f % C, pp = f / C;
        int pxl = pp % P, py = pp / P;
        float v[EPC];
#pragma unroll
        for (int j = 0; j < EPC; ++j) {
            v[j] = (f + j < live) ? tile[c * plane + py * SW + s * P + pxl] : 0.f;
            if (++c == C) { c = 0; if (++pxl == P) { pxl = 0; ++py; } }
        }
        if constexpr (F32) {
            *(float4*)((float*)rows + (row0 + s) * ld + f) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
            *(uint4*)((bf16_t*)rows + (row0 + s) * ld + f) = make_uint4(pack2bf(v[0], v[1]), pack2bf(v[2], v[3]), pack2bf(v[4], v[5]), pack2bf(v[6], v[7]));
        }
    }
}

// x[(b * Np + n)][d] = pos[n][d] + mod[d]  (fp32, 16 bytes per lane)
__global__ __launch_bounds__(256) void vit_emb_rows_kernel(const float* __restrict__ pos, const float* __restrict__ mod, float* __restrict__ x, int ldx,
                                                           long long rows, int Np, int D4) {
    const long long total = rows * D4;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const long long r = i / D4;
        const int d4 = (int)(i % D4), n = (int)(r % Np);
        const float4 p = *(const float4*)(pos + ((size_t)n * D4 + d4) * 4), m = *(const float4*)(mod + d4 * 4);
        *(float4*)(x + (size_t)r * ldx + d4 * 4) = make_float4(p.x + m.x, p.y + m.y, p.z + m.z, p.w + m.w);
    }
}

// Exact-as-fp32-allows column sum of an fp32 matrix: every column is summed in double in a fixed order (partial[y][n] over the row slice y,
// then the slices), added to db[n] in double and rounded once.  64 columns x 4 waves per workgroup: a wave reads 256 contiguous bytes per row.
__global__ __launch_bounds__(256) void vit_colsum_partial_kernel(const float* __restrict__ dy, int ldy, double* __restrict__ partial, int R, int N) {
    __shared__ double red[4][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int n = blockIdx.x * 64 + lane;
    double s = 0.0;
    if (n < N)
        for (int r = blockIdx.y * 4 + w; r < R; r += gridDim.y * 4) s += (double)dy[(size_t)r * ldy + n];
    red[w][lane] = s;
    __syncthreads();
    if (w == 0 && n < N) partial[(size_t)blockIdx.y * N + n] = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
}
__global__ __launch_bounds__(256) void vit_colsum_final_kernel(const double* __restrict__ partial, float* __restrict__ db, int Y, int N) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    double s = 0.0;
    for (int y = 0; y < Y; ++y) s += partial[(size_t)y * N + n];
    db[n] = (float)((double)db[n] + s);
}

}  // namespace

extern "C" int fm_vit_patch_rows(const void* pixels, void* rows, int ld, int B, int C, int H, int W, int P, int rows_f32, void* stream) {
    FM_CHECK_ARG(pixels && rows, "fm_vit_patch_rows: null pointer (pixels %p, rows %p)", pixels, rows);
    FM_CHECK_ARG(B > 0 && C > 0 && H > 0 && W > 0 && P > 0, "fm_vit_patch_rows: B=%d C=%d H=%d W=%d P=%d must be positive", B, C, H, W, P);
    FM_CHECK_ARG(H % P == 0 && W % P == 0, "fm_vit_patch_rows: image %d x %d is not a whole number of %d x %d patches", H, W, P, P);
    FM_CHECK_ARG(ld % 8 == 0, "fm_vit_patch_rows: ld=%d is not a multiple of 8 (16-byte stores)", ld);
    FM_CHECK_ARG((long long)P * P * C <= VIT_LDS_FLOATS, "fm_vit_patch_rows: a patch of %d x %d x %d values exceeds the %d-value LDS tile", P, P, C, VIT_LDS_FLOATS);
    FM_CHECK_ARG(ld >= P * P * C, "fm_vit_patch_rows: ld=%d is smaller than the %d features of a patch", ld, P * P * C);
    FM_CHECK_ARG((((uintptr_t)pixels) & 15) == 0, "fm_vit_patch_rows: pixels are not 16-byte aligned");
    FM_CHECK_ARG((((uintptr_t)rows) & 15) == 0, "fm_vit_patch_rows: rows are not 16-byte aligned");
    const int gw = W / P, gh = H / P;
    FM_CHECK_ARG((long long)B * gh * gw <= 0x7fffffffLL / 4, "fm_vit_patch_rows: %lld patches exceed the grid", (long long)B * gh * gw);
    const int smax = VIT_LDS_FLOATS / (P * P * C);
    const int nstrips = (gw + smax - 1) / smax;
    const int S = (gw + nstrips - 1) / nstrips;               // even strips: S <= smax
    const bool vec = P % 4 == 0 && W % 4 == 0;                // every segment starts and ends on a 16-byte boundary
    const dim3 grid((unsigned)(B * gh * nstrips)), block(256);
    const hipStream_t s = (hipStream_t)stream;
    const float* px = (const float*)pixels;
    if (rows_f32) {
        if (vec) hipLaunchKernelGGL((vit_patch_rows_kernel<true, true>), grid, block, 0, s, px, rows, ld, C, H, W, P, S, nstrips);
        else hipLaunchKernelGGL((vit_patch_rows_kernel<true, false>), grid, block, 0, s, px, rows, ld, C, H, W, P, S, nstrips);
    } else {
        if (vec) hipLaunchKernelGGL((vit_patch_rows_kernel<false, true>), grid, block, 0, s, px, rows, ld, C, H, W, P, S, nstrips);
        else hipLaunchKernelGGL((vit_patch_rows_kernel<false, false>), grid, block, 0, s, px, rows, ld, C, H, W, P, S, nstrips);
    }
    FM_CHECK_LAUNCH("fm_vit_patch_rows");
    return 0;
}

extern "C" int fm_vit_emb_rows(const void* pos, const void* mod_emb, void* x, int ldx, int B, int Np, int D, void* stream) {
    FM_CHECK_ARG(pos && mod_emb && x, "fm_vit_emb_rows: null pointer");
    FM_CHECK_ARG(B > 0 && Np > 0 && D > 0 && D % 4 == 0 && ldx >= D && ldx % 4 == 0, "fm_vit_emb_rows: B=%d Np=%d D=%d ldx=%d (D, ldx multiples of 4, ldx >= D)", B, Np, D, ldx);
    FM_CHECK_ARG(((((uintptr_t)pos) | ((uintptr_t)mod_emb) | ((uintptr_t)x)) & 15) == 0, "fm_vit_emb_rows: pointers must be 16-byte aligned");
    const long long rows = (long long)B * Np, total = rows * (D / 4);
    const unsigned blocks = (unsigned)((total + 255) / 256 < 8192 ? (total + 255) / 256 : 8192);
    hipLaunchKernelGGL(vit_emb_rows_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const float*)pos, (const float*)mod_emb, (float*)x, ldx, rows, Np, D / 4);
    FM_CHECK_LAUNCH("fm_vit_emb_rows");
    return 0;
}

extern "C" int fm_vit_colsum(const void* dy, int ldy, void* db, int R, int N, void* ws, int64_t ws_bytes, void* stream) {
    FM_CHECK_ARG(dy && db && ws, "fm_vit_colsum: null pointer");
    FM_CHECK_ARG(R > 0 && N > 0 && ldy >= N, "fm_vit_colsum: R=%d N=%d ldy=%d (ldy >= N)", R, N, ldy);
    FM_CHECK_ARG((((uintptr_t)ws) & 7) == 0, "fm_vit_colsum: workspace is not 8-byte aligned");
    const int Y = R >= 64 * 32 ? 64 : (R + 31) / 32;          // row slices: at least 32 rows each, at most 64 slices
    FM_CHECK_ARG(ws_bytes >= (long long)Y * N * 8, "fm_vit_colsum: workspace of %lld bytes, %lld needed", (long long)ws_bytes, (long long)Y * N * 8);
    hipLaunchKernelGGL(vit_colsum_partial_kernel, dim3((N + 63) / 64, Y), dim3(256), 0, (hipStream_t)stream, (const float*)dy, ldy, (double*)ws, R, N);
    FM_CHECK_LAUNCH("fm_vit_colsum");
    hipLaunchKernelGGL(vit_colsum_final_kernel, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const double*)ws, (float*)db, Y, N);
    FM_CHECK_LAUNCH("fm_vit_colsum");
    return 0;
}
