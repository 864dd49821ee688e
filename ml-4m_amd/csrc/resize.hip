// Image resize, forward and adjoint (include/fourm_hip.h, "image resize"): what upstream's tokenizer trainer does with F.interpolate on the
// device every iteration - prepare_inputs (bilinear for images, nearest for class maps) and the antialiased Resize in front of the CLIP loss,
// whose gradient flows back into the decoder.  Both bilinear modes are separable; one axis is a table (start, count, weights) per output
// index, made on the host in double by fm_resize_axis_table (api.cpp) and rounded once to fp32.
//
// Forward: one workgroup (256 threads) per (plane, tile of th x tw outputs, at most 32 x 32).  The table rows of the tile go to LDS, their
// union is the tile's input window [r0, r1) x [c0, c1); the window is staged in LDS with row-contiguous loads (a wavefront reads up to 256
// consecutive bytes of an image row), filtered along the rows into mid (window rows x tw), then along the columns; the store of a tile row is
// tw consecutive floats.  Adjoint: the same structure over a tile of INPUT pixels (at most 64 x 64) and the window of dy given by the transposed tables; every
// input pixel adds the outputs that read it in index order - a gather, no atomics, the same bits every time.  All LDS is dynamic and read
// with 32-bit accesses: in the column pass the 32 lanes of a half wavefront read consecutive words of one row of mid (no bank conflicts), in
// the row pass they read a row of the window at a stride of the scale factor (2 - 3 way for 512 -> 224).  The host picks the largest tile
// whose window bound fits 64 KiB; a kernel uses a table entry as an index only after checking it against the sizes and the LDS capacities
// (a tile with inconsistent table rows is filled with NaN instead).
#include <limits.h>
#include <math.h>

#include "common.h"
#include "fourm_hip.h"

namespace {

constexpr int LDS_BYTES = 64 * 1024;
constexpr int NT = 256;

struct ResizeArgs {
    const float* src;            // x (forward) or dy (adjoint)
    float* dst;                  // y or dx
    const int *start_h, *count_h, *start_w, *count_w;
    const float *w_h, *w_w;
    const int *ts_h, *tc_h, *ts_w, *tc_w;          // transposed ranges (adjoint only)
    const float *scale, *shift;
    int C, H_in, W_in, H_out, W_out;
    int taps_h, taps_w;
    int th, tw, tw_shift, cap_h, cap_w, tiles_x, tiles_y;
};

__device__ __forceinline__ int imin(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int imax(int a, int b) { return a > b ? a : b; }

__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = imin(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = imax(v, __shfl_xor(v, o, 64));
    return v;
}

// One wavefront, lane i < n holding the range (s, c) of tile entry i (n <= 64): out[0 .. 3] = lo, hi of the union [lo, hi) of the ranges, the
// largest count, and whether every one of them is a range inside [0, limit) of at most max_count.  lo and hi mean nothing when that is 0.
__device__ __forceinline__ void union_of_ranges(int lane, int n, int s, int c, int limit, int max_count, int* out) {
    const bool in = lane < n;
    const bool ok = !in || (c >= 0 && c <= max_count && c <= limit && s >= 0 && s <= limit - c);
    const int lo = wave_min_i(in && ok ? s : INT_MAX), hi = wave_max_i(in && ok ? s + c : 0);
    const int mx = wave_max_i(in && ok ? c : 0), all = wave_min_i(ok ? 1 : 0);
    if (lane == 0) { out[0] = imin(lo, hi); out[1] = hi; out[2] = mx; out[3] = all; }
}

// rows x cols floats from global (row stride ld) into LDS (row stride cap): consecutive threads take consecutive columns of a row; STAGE_LOADS
// loads are in flight per thread before the first is stored.  8, measured: 24 (the 77 x 77 window of 512 -> 224 in one round trip) gained 10 %
// there, but its registers cost the small-window cases three of their eight waves per SIMD (512 -> 384 forward at 0.75 x, both adjoints slower).
constexpr int STAGE_LOADS = 8;
__device__ __forceinline__ void stage_window(const float* __restrict__ g, long long ld, float* __restrict__ l, int cap, int rows, int cols) {
    if (rows <= 0 || cols <= 0) return;
    int r = threadIdx.x / cols, c = threadIdx.x - r * cols;
    const int dq = NT / cols, dr = NT - dq * cols;
    while (r < rows) {
        float v[STAGE_LOADS];
        int at[STAGE_LOADS];
#pragma unroll
        for (int u = 0; u < STAGE_LOADS; ++u) {
            const bool in = r < rows;
            at[u] = in ? r * cap + c : -1;
            v[u] = in ? g[r * ld + c] : 0.f;
            r += dq;
            c += dr;
            if (c >= cols) { c -= cols; ++r; }
        }
#pragma unroll
        for (int u = 0; u < STAGE_LOADS; ++u)
            if (at[u] >= 0) l[at[u]] = v[u];
    }
}

constexpr int FT = 8;          // windows of up to FT taps are filtered from registers, all loads of a dot product issued before its first multiply

// sum_j w[j] p[j stride] over j < cnt <= FT in index order (w[j] = 0 for j >= cnt)
__device__ __forceinline__ float dot_taps(const float (&w)[FT], const float* p, int stride, int cnt) {
    float v[FT];
#pragma unroll
    for (int j = 0; j < FT; ++j) v[j] = j < cnt ? p[j * stride] : 0.f;
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < FT; ++j) acc = fmaf(w[j], v[j], acc);
    return acc;
}

__device__ __forceinline__ void fill_tile(float* __restrict__ p, int ld, int rows, int cols, int tw_shift, float v) {
    for (int idx = threadIdx.x; idx < (rows << tw_shift); idx += NT) {
        const int r = idx >> tw_shift, c = idx & ((1 << tw_shift) - 1);
        if (c < cols) p[(long long)r * ld + c] = v;
    }
}

extern __shared__ __attribute__((aligned(16))) char resize_smem[];

// ---- forward: y = a R(x) + b ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void resize_fwd_kernel(const ResizeArgs a) {
    float* win = (float*)resize_smem;                       // cap_h x cap_w: the input window
    float* mid = win + a.cap_h * a.cap_w;                   // cap_h x tw: filtered along the rows
    float* wh = mid + a.cap_h * a.tw;                       // th x taps_h
    float* ww = wh + a.th * a.taps_h;                       // tw x taps_w
    int* sh = (int*)(ww + a.tw * a.taps_w);                 // th, th, tw, tw
    int* ch = sh + a.th;
    int* sw = ch + a.th;
    int* cw = sw + a.tw;
    int* bnd = cw + a.tw;                                   // 8: lo, hi, largest count, valid - of the rows, of the columns
    const int tid = threadIdx.x;
    const int tiles = a.tiles_x * a.tiles_y;
    const int plane = blockIdx.x / tiles, tile = blockIdx.x - plane * tiles;
    const int ty = tile / a.tiles_x;
    const int oh0 = ty * a.th, ow0 = (tile - ty * a.tiles_x) * a.tw;
    const int nh = imin(a.th, a.H_out - oh0), nw = imin(a.tw, a.W_out - ow0);
    if (tid < 64) {                                         // wavefront 0: the tile's rows of the H table; wavefront 1: of the W table
        int s = 0, c = 0;
        if (tid < nh) { s = sh[tid] = a.start_h[oh0 + tid]; c = ch[tid] = a.count_h[oh0 + tid]; }
        union_of_ranges(tid, nh, s, c, a.H_in, a.taps_h, bnd);
    } else if (tid < 128) {
        const int l = tid - 64;
        int s = 0, c = 0;
        if (l < nw) { s = sw[l] = a.start_w[ow0 + l]; c = cw[l] = a.count_w[ow0 + l]; }
        union_of_ranges(l, nw, s, c, a.W_in, a.taps_w, bnd + 4);
    }
    __syncthreads();
    const int r0 = bnd[0], c0 = bnd[4], rows = bnd[1] - r0, cols = bnd[5] - c0;
    const bool ok = bnd[3] && bnd[7];
    const bool regs_h = bnd[2] <= FT, regs_w = bnd[6] <= FT;
    float* yp = a.dst + ((long long)plane * a.H_out + oh0) * a.W_out + ow0;
    if (!ok || rows > a.cap_h || cols > a.cap_w) {          // (the same in every thread)
        fill_tile(yp, a.W_out, nh, nw, a.tw_shift, __builtin_nanf(""));
        return;
    }
    for (int i = tid; i < nh * a.taps_h; i += NT) wh[i] = a.w_h[(long long)oh0 * a.taps_h + i];
    for (int i = tid; i < nw * a.taps_w; i += NT) ww[i] = a.w_w[(long long)ow0 * a.taps_w + i];
    stage_window(a.src + ((long long)plane * a.H_in + r0) * a.W_in + c0, a.W_in, win, a.cap_w, rows, cols);
    __syncthreads();
    const int mask = a.tw - 1;
    {                                                       // along the rows: this thread's column ow is the same in every iteration
        const int ow = tid & mask;
        if (ow < nw) {
            const int off = sw[ow] - c0, cnt = cw[ow];
            const float* wp = ww + ow * a.taps_w;
            if (regs_w) {
                float w[FT];
#pragma unroll
                for (int j = 0; j < FT; ++j) w[j] = j < cnt ? wp[j] : 0.f;
#pragma unroll 2
                for (int r = tid >> a.tw_shift; r < rows; r += NT >> a.tw_shift) mid[r * a.tw + ow] = dot_taps(w, win + r * a.cap_w + off, 1, cnt);
            } else {
                for (int r = tid >> a.tw_shift; r < rows; r += NT >> a.tw_shift) {
                    const float* p = win + r * a.cap_w + off;
                    float acc = 0.f;
                    for (int j = 0; j < cnt; ++j) acc = fmaf(wp[j], p[j], acc);
                    mid[r * a.tw + ow] = acc;
                }
            }
        }
    }
    __syncthreads();
    const int c = plane % a.C;
    const float sa = a.scale ? a.scale[c] : 1.0f, sb = a.scale ? a.shift[c] : 0.0f;
#pragma unroll 2
    for (int idx = tid; idx < (nh << a.tw_shift); idx += NT) {
        const int oh = idx >> a.tw_shift, ow = idx & mask;
        if (ow >= nw) continue;
        const float* wp = wh + oh * a.taps_h;
        const float* p = mid + (sh[oh] - r0) * a.tw + ow;
        const int cnt = ch[oh];
        float acc = 0.f;
        if (regs_h) {
            float w[FT];
#pragma unroll
            for (int i = 0; i < FT; ++i) w[i] = i < cnt ? wp[i] : 0.f;
            acc = dot_taps(w, p, a.tw, cnt);
        } else {
            for (int i = 0; i < cnt; ++i) acc = fmaf(wp[i], p[i * a.tw], acc);
        }
        yp[(long long)oh * a.W_out + ow] = a.scale ? fmaf(sa, acc, sb) : acc;
    }
}

// ---- adjoint: dx = a R^T(dy) ----------------------------------------------------------------------------------------------------------------
// weight of output o (row o of the staged table: start s[o], count c[o], weights w[o][taps]) on input pixel i; 0 when o does not read i
__device__ __forceinline__ float tap_weight(const int* s, const int* c, const float* w, int taps, int o, int i) {
    const int k = i - s[o];
    return (k >= 0 && k < c[o] && k < taps) ? w[o * taps + k] : 0.f;
}

__global__ __launch_bounds__(NT) void resize_bwd_kernel(const ResizeArgs a) {
    float* win = (float*)resize_smem;                       // cap_h x cap_w: the window of dy
    float* mid = win + a.cap_h * a.cap_w;                   // cap_h x tw: gathered along the rows
    float* wh = mid + a.cap_h * a.tw;                       // cap_h x taps_h: the table rows of the window's outputs
    float* ww = wh + a.cap_h * a.taps_h;                    // cap_w x taps_w
    int* sh = (int*)(ww + a.cap_w * a.taps_w);              // cap_h, cap_h, cap_w, cap_w
    int* ch = sh + a.cap_h;
    int* sw = ch + a.cap_h;
    int* cw = sw + a.cap_w;
    int* tsh = cw + a.cap_w;                                // th, th, tw, tw: the transposed ranges of the tile's input pixels
    int* tch = tsh + a.th;
    int* tsw = tch + a.th;
    int* tcw = tsw + a.tw;
    int* bnd = tcw + a.tw;                                  // 8: lo, hi, largest count, valid - of the rows, of the columns
    const int tid = threadIdx.x;
    const int tiles = a.tiles_x * a.tiles_y;
    const int plane = blockIdx.x / tiles, tile = blockIdx.x - plane * tiles;
    const int ty = tile / a.tiles_x;
    const int ih0 = ty * a.th, iw0 = (tile - ty * a.tiles_x) * a.tw;
    const int nh = imin(a.th, a.H_in - ih0), nw = imin(a.tw, a.W_in - iw0);
    if (tid < 64) {
        int s = 0, c = 0;
        if (tid < nh) { s = tsh[tid] = a.ts_h[ih0 + tid]; c = tch[tid] = a.tc_h[ih0 + tid]; }
        union_of_ranges(tid, nh, s, c, a.H_out, a.H_out, bnd);
    } else if (tid < 128) {
        const int l = tid - 64;
        int s = 0, c = 0;
        if (l < nw) { s = tsw[l] = a.ts_w[iw0 + l]; c = tcw[l] = a.tc_w[iw0 + l]; }
        union_of_ranges(l, nw, s, c, a.W_out, a.W_out, bnd + 4);
    }
    __syncthreads();
    const int r0 = bnd[0], c0 = bnd[4], rows = bnd[1] - r0, cols = bnd[5] - c0;
    const bool ok = bnd[3] && bnd[7];
    const bool regs_h = bnd[2] <= FT, regs_w = bnd[6] <= FT;
    float* xp = a.dst + ((long long)plane * a.H_in + ih0) * a.W_in + iw0;
    if (!ok || rows > a.cap_h || cols > a.cap_w) {
        fill_tile(xp, a.W_in, nh, nw, a.tw_shift, __builtin_nanf(""));
        return;
    }
    for (int i = tid; i < rows; i += NT) { sh[i] = a.start_h[r0 + i]; ch[i] = a.count_h[r0 + i]; }
    for (int i = tid; i < cols; i += NT) { sw[i] = a.start_w[c0 + i]; cw[i] = a.count_w[c0 + i]; }
    for (int i = tid; i < rows * a.taps_h; i += NT) wh[i] = a.w_h[(long long)r0 * a.taps_h + i];
    for (int i = tid; i < cols * a.taps_w; i += NT) ww[i] = a.w_w[(long long)c0 * a.taps_w + i];
    stage_window(a.src + ((long long)plane * a.H_out + r0) * a.W_out + c0, a.W_out, win, a.cap_w, rows, cols);
    __syncthreads();
    const int mask = a.tw - 1;
    {                                                       // along the rows of dy: input column iw gathers outputs [o0, o1) in order
        const int iw = tid & mask;
        if (iw < nw) {
            const int cnt = tcw[iw], o0 = tsw[iw] - c0, o1 = o0 + cnt;
            if (regs_w) {                                   // this column's weights do not depend on the row
                float w[FT];
#pragma unroll
                for (int u = 0; u < FT; ++u) w[u] = u < cnt ? tap_weight(sw, cw, ww, a.taps_w, o0 + u, iw0 + iw) : 0.f;
#pragma unroll 2
                for (int r = tid >> a.tw_shift; r < rows; r += NT >> a.tw_shift) mid[r * a.tw + iw] = dot_taps(w, win + r * a.cap_w + o0, 1, cnt);
            } else {
                for (int r = tid >> a.tw_shift; r < rows; r += NT >> a.tw_shift) {
                    const float* p = win + r * a.cap_w;
                    float acc = 0.f;
                    for (int o = o0; o < o1; ++o) acc = fmaf(tap_weight(sw, cw, ww, a.taps_w, o, iw0 + iw), p[o], acc);
                    mid[r * a.tw + iw] = acc;
                }
            }
        }
    }
    __syncthreads();
    const float sa = a.scale ? a.scale[plane % a.C] : 1.0f;
#pragma unroll 2
    for (int idx = tid; idx < (nh << a.tw_shift); idx += NT) {
        const int ih = idx >> a.tw_shift, iw = idx & mask;
        if (iw >= nw) continue;
        const int cnt = tch[ih], o0 = tsh[ih] - r0, o1 = o0 + cnt;
        float acc = 0.f;
        if (regs_h) {
            float w[FT];
#pragma unroll
            for (int u = 0; u < FT; ++u) w[u] = u < cnt ? tap_weight(sh, ch, wh, a.taps_h, o0 + u, ih0 + ih) : 0.f;
            acc = dot_taps(w, mid + o0 * a.tw + iw, a.tw, cnt);
        } else {
            for (int o = o0; o < o1; ++o) acc = fmaf(tap_weight(sh, ch, wh, a.taps_h, o, ih0 + ih), mid[o * a.tw + iw], acc);
        }
        xp[(long long)ih * a.W_in + iw] = a.scale ? sa * acc : acc;
    }
}

// ---- nearest ----------------------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(NT) void resize_nearest_kernel(const T* __restrict__ x, T* __restrict__ y, int planes, int H_in, int W_in, int H_out, int W_out,
                                                            const int* __restrict__ index_h, const int* __restrict__ index_w) {
    const int ow = blockIdx.x * 64 + (threadIdx.x & 63), oh = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (ow >= W_out || oh >= H_out) return;
    const int r = imin(imax(index_h[oh], 0), H_in - 1), c = imin(imax(index_w[ow], 0), W_in - 1);
    for (int p = blockIdx.z; p < planes; p += gridDim.z) y[((long long)p * H_out + oh) * W_out + ow] = x[((long long)p * H_in + r) * W_in + c];
}

inline bool aligned(const void* p, uintptr_t a) { return (((uintptr_t)p) & (a - 1)) == 0; }

// Upper bounds of a tile's window from the sizes alone (sc = n_in / n_out, sup = max(sc, 1); every window of the table lies inside
// [c - sup - 0.5, c + sup + 0.5) around c = sc (o + 0.5), before the zero taps are dropped).  Forward, t outputs: the union spans at most
// sc (t - 1) + 2 sup + 1 input pixels.  Adjoint, t input pixels: they are read by the outputs with c inside an interval of t + 2 sup, that is
// at most (t + 2 sup) / sc + 1 outputs.  One more each for the rounding of this arithmetic; the kernels check the real windows.
int span_fwd(int n_in, int n_out, int t) {
    const double sc = (double)n_in / n_out, sup = sc >= 1.0 ? sc : 1.0;
    const double e = sc * (t - 1) + 2.0 * sup + 2.0;
    return e < (double)n_in ? (int)e : n_in;
}
int span_bwd(int n_in, int n_out, int t) {
    const double sc = (double)n_in / n_out, sup = sc >= 1.0 ? sc : 1.0;
    const double e = (t + 2.0 * sup) / sc + 2.0;
    return e < (double)n_out ? (int)e : n_out;
}

const int TILES[][2] = {{64, 64}, {32, 64}, {32, 32}, {16, 32}, {16, 16}, {8, 16}, {8, 8}, {4, 8}, {4, 4}, {2, 4}, {2, 2}, {1, 2}, {1, 1}};

// the largest tile whose LDS need fits; false: none does
bool pick_tile(ResizeArgs& a, bool bwd, size_t& bytes) {
    for (const auto& t : TILES) {
        const int th = t[0], tw = t[1];
        if (!bwd && tw > 32) continue;          // forward: 64 x 64 outputs need 53 KiB for 512 -> 384 and ran at 0.67 x the rate of 32 x 32 (three workgroups per CU)
        const long long ch = bwd ? span_bwd(a.H_in, a.H_out, th) : span_fwd(a.H_in, a.H_out, th);
        const long long cw = bwd ? span_bwd(a.W_in, a.W_out, tw) : span_fwd(a.W_in, a.W_out, tw);
        long long words = ch * cw + ch * tw + 2 * th + 2 * tw + 8;
        words += bwd ? ch * (a.taps_h + 2) + cw * (a.taps_w + 2) : (long long)th * a.taps_h + (long long)tw * a.taps_w;
        if (words * 4 > LDS_BYTES) continue;
        a.th = th; a.tw = tw; a.cap_h = (int)ch; a.cap_w = (int)cw;
        a.tw_shift = 0;
        while ((1 << a.tw_shift) < tw) ++a.tw_shift;
        bytes = (size_t)((words * 4 + 15) & ~15LL);
        return true;
    }
    return false;
}

int launch_bilinear(const char* name, bool bwd, ResizeArgs& a, int planes, void* stream) {
    FM_CHECK_ARG(a.src && a.dst && a.start_h && a.count_h && a.w_h && a.start_w && a.count_w && a.w_w && (!bwd || (a.ts_h && a.tc_h && a.ts_w && a.tc_w)),
                 "%s: null pointer", name);
    FM_CHECK_ARG(planes > 0 && a.C > 0 && a.H_in > 0 && a.W_in > 0 && a.H_out > 0 && a.W_out > 0 && a.H_in <= (1 << 24) && a.W_in <= (1 << 24) &&
                     a.H_out <= (1 << 24) && a.W_out <= (1 << 24) && (double)planes * a.H_in * (double)a.W_in <= 4.0e12 &&
                     (double)planes * a.H_out * (double)a.W_out <= 4.0e12,
                 "%s: bad shape (planes=%d C=%d %dx%d -> %dx%d)", name, planes, a.C, a.H_in, a.W_in, a.H_out, a.W_out);
    FM_CHECK_ARG(a.taps_h >= 1 && a.taps_h <= FM_RESIZE_MAX_TAPS && a.taps_w >= 1 && a.taps_w <= FM_RESIZE_MAX_TAPS, "%s: taps %d, %d (1 .. %d)", name, a.taps_h,
                 a.taps_w, FM_RESIZE_MAX_TAPS);
    FM_CHECK_ARG((a.scale != nullptr) == (a.shift != nullptr) || bwd, "%s: scale and shift come together", name);
    FM_CHECK_ARG(aligned(a.src, 4) && aligned(a.dst, 4) && aligned(a.start_h, 4) && aligned(a.count_h, 4) && aligned(a.w_h, 4) && aligned(a.start_w, 4) &&
                     aligned(a.count_w, 4) && aligned(a.w_w, 4) && aligned(a.ts_h, 4) && aligned(a.tc_h, 4) && aligned(a.ts_w, 4) && aligned(a.tc_w, 4) &&
                     aligned(a.scale, 4) && aligned(a.shift, 4),
                 "%s: misaligned pointer", name);
    size_t bytes = 0;
    FM_CHECK_ARG(pick_tile(a, bwd, bytes), "%s: %dx%d -> %dx%d with %d, %d taps: not even a 1 x 1 tile fits %d bytes of LDS", name, a.H_in, a.W_in, a.H_out, a.W_out,
                 a.taps_h, a.taps_w, LDS_BYTES);
    const int th_n = bwd ? a.H_in : a.H_out, tw_n = bwd ? a.W_in : a.W_out;
    a.tiles_y = (th_n + a.th - 1) / a.th;
    a.tiles_x = (tw_n + a.tw - 1) / a.tw;
    const long long wgs = (long long)planes * a.tiles_x * a.tiles_y;
    FM_CHECK_ARG((long long)a.tiles_x * a.tiles_y <= 0x3fffffffLL && wgs <= 0x7fffffffLL, "%s: too many tiles", name);
    if (bwd) hipLaunchKernelGGL(resize_bwd_kernel, dim3((unsigned)wgs), dim3(NT), bytes, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(resize_fwd_kernel, dim3((unsigned)wgs), dim3(NT), bytes, (hipStream_t)stream, a);
    FM_CHECK_LAUNCH(name);
    return 0;
}

}  // namespace

extern "C" int fm_resize_bilinear_fwd(const void* x, void* y, int planes, int H_in, int W_in, int H_out, int W_out, const void* start_h, const void* count_h,
                                      const void* weights_h, int taps_h, const void* start_w, const void* count_w, const void* weights_w, int taps_w,
                                      const void* scale, const void* shift, int C, void* stream) {
    ResizeArgs a = {};
    a.src = (const float*)x; a.dst = (float*)y;
    a.start_h = (const int*)start_h; a.count_h = (const int*)count_h; a.w_h = (const float*)weights_h; a.taps_h = taps_h;
    a.start_w = (const int*)start_w; a.count_w = (const int*)count_w; a.w_w = (const float*)weights_w; a.taps_w = taps_w;
    a.scale = (const float*)scale; a.shift = (const float*)shift;
    a.C = C; a.H_in = H_in; a.W_in = W_in; a.H_out = H_out; a.W_out = W_out;
    return launch_bilinear("fm_resize_bilinear_fwd", false, a, planes, stream);
}

extern "C" int fm_resize_bilinear_bwd(const void* dy, void* dx, int planes, int H_in, int W_in, int H_out, int W_out, const void* start_h, const void* count_h,
                                      const void* weights_h, int taps_h, const void* t_start_h, const void* t_count_h, const void* start_w,
                                      const void* count_w, const void* weights_w, int taps_w, const void* t_start_w, const void* t_count_w,
                                      const void* scale, int C, void* stream) {
    ResizeArgs a = {};
    a.src = (const float*)dy; a.dst = (float*)dx;
    a.start_h = (const int*)start_h; a.count_h = (const int*)count_h; a.w_h = (const float*)weights_h; a.taps_h = taps_h;
    a.start_w = (const int*)start_w; a.count_w = (const int*)count_w; a.w_w = (const float*)weights_w; a.taps_w = taps_w;
    a.ts_h = (const int*)t_start_h; a.tc_h = (const int*)t_count_h; a.ts_w = (const int*)t_start_w; a.tc_w = (const int*)t_count_w;
    a.scale = (const float*)scale;
    a.C = C; a.H_in = H_in; a.W_in = W_in; a.H_out = H_out; a.W_out = W_out;
    return launch_bilinear("fm_resize_bilinear_bwd", true, a, planes, stream);
}

extern "C" int fm_resize_nearest(const void* x, void* y, int elem_size, int planes, int H_in, int W_in, int H_out, int W_out, const void* index_h,
                                 const void* index_w, void* stream) {
    FM_CHECK_ARG(x && y && index_h && index_w, "fm_resize_nearest: null pointer");
    FM_CHECK_ARG(elem_size == 4 || elem_size == 8, "fm_resize_nearest: elements of %d bytes (4: f32, 8: int64)", elem_size);
    FM_CHECK_ARG(planes > 0 && H_in > 0 && W_in > 0 && H_out > 0 && W_out > 0 && (double)planes * H_in * (double)W_in <= 4.0e12 &&
                     (double)planes * H_out * (double)W_out <= 4.0e12 && (H_out + 3) / 4 <= 65535,
                 "fm_resize_nearest: bad shape (planes=%d %dx%d -> %dx%d)", planes, H_in, W_in, H_out, W_out);
    FM_CHECK_ARG(aligned(x, elem_size) && aligned(y, elem_size) && aligned(index_h, 4) && aligned(index_w, 4), "fm_resize_nearest: misaligned pointer");
    const dim3 grid((unsigned)((W_out + 63) / 64), (unsigned)((H_out + 3) / 4), (unsigned)(planes < 65535 ? planes : 65535));
    hipStream_t st = (hipStream_t)stream;
    if (elem_size == 8)
        hipLaunchKernelGGL(resize_nearest_kernel<long long>, grid, dim3(NT), 0, st, (const long long*)x, (long long*)y, planes, H_in, W_in, H_out, W_out, (const int*)index_h,
                           (const int*)index_w);
    else
        hipLaunchKernelGGL(resize_nearest_kernel<float>, grid, dim3(NT), 0, st, (const float*)x, (float*)y, planes, H_in, W_in, H_out, W_out, (const int*)index_h,
                           (const int*)index_w);
    FM_CHECK_LAUNCH("fm_resize_nearest");
    return 0;
}
