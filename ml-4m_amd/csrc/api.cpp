// Error string + version for the C ABI, and the host-only table builder of the resize kernels (csrc/resize.hip).
#include <math.h>
#include <stdarg.h>
#include <stdio.h>

#include <vector>

#include "common.h"
#include "fourm_hip.h"

static thread_local char g_err[512] = "";

void fm_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" const char* fm_last_error(void) { return g_err; }
extern "C" int fm_abi_version(void) { return FM_ABI_VERSION; }

// ---- resize: one axis as (start, count, weights) per output index ---------------------------------------------------------------------------
// The window of output o in double, F.interpolate's arithmetic (include/fourm_hip.h has the formulas); taps of weight zero at either end are
// dropped.  -> start; w holds the count weights.
static int resize_axis_row(int n_in, int n_out, int mode, int o, std::vector<double>& w) {
    w.clear();
    if (mode == FM_RESIZE_NEAREST) {
        const float scale = (float)n_in / (float)n_out;
        const int i = (int)floorf((float)o * scale);
        w.push_back(1.0);
        return i < n_in - 1 ? i : n_in - 1;
    }
    const double scale = (double)n_in / (double)n_out;
    int start;
    if (mode == FM_RESIZE_BILINEAR) {
        double s = scale * (o + 0.5) - 0.5;
        if (s < 0.0) s = 0.0;
        int i0 = (int)floor(s);
        if (i0 > n_in - 1) i0 = n_in - 1;
        double l1 = s - i0;
        l1 = l1 < 0.0 ? 0.0 : l1 > 1.0 ? 1.0 : l1;
        start = i0;
        if (i0 + 1 > n_in - 1) {
            w.push_back(1.0);                                                       // i1 = i0: both weights land on one pixel
        } else {
            w.push_back(1.0 - l1);
            w.push_back(l1);
        }
    } else {
        const double support = scale >= 1.0 ? scale : 1.0, inv = scale >= 1.0 ? 1.0 / scale : 1.0;
        const double c = scale * (o + 0.5);
        long long xmin = (long long)(c - support + 0.5);
        if (xmin < 0) xmin = 0;
        long long xend = (long long)(c + support + 0.5);
        if (xend > n_in) xend = n_in;
        double total = 0.0;
        for (long long j = 0; j < xend - xmin; ++j) {
            const double t = fabs(((double)(j + xmin) - c + 0.5) * inv);
            const double v = t < 1.0 ? 1.0 - t : 0.0;
            w.push_back(v);
            total += v;
        }
        if (total != 0.0)
            for (double& v : w) v /= total;
        start = (int)xmin;
    }
    size_t lead = 0;
    while (lead + 1 < w.size() && w[lead] == 0.0) ++lead;
    w.erase(w.begin(), w.begin() + lead);
    while (w.size() > 1 && w.back() == 0.0) w.pop_back();
    return start + (int)lead;
}

extern "C" int fm_resize_axis_table(int n_in, int n_out, int mode, int32_t* start, int32_t* count, float* weights, double* weights_f64, int32_t* t_start,
                                    int32_t* t_count) {
    FM_CHECK_ARG(n_in > 0 && n_out > 0 && n_in <= (1 << 24) && n_out <= (1 << 24), "fm_resize_axis_table: sizes %d -> %d (1 .. 2^24 each)", n_in, n_out);
    FM_CHECK_ARG(mode == FM_RESIZE_BILINEAR || mode == FM_RESIZE_BILINEAR_AA || mode == FM_RESIZE_NEAREST, "fm_resize_axis_table: mode %d", mode);
    if (mode == FM_RESIZE_BILINEAR_AA)          // a window is at most 2 support + 1 pixels and at least 2 support - 1 away from the borders: refuse before building it
        FM_CHECK_ARG(n_in <= FM_RESIZE_MAX_TAPS || 2.0 * (double)n_in / (double)n_out - 1.0 <= (double)FM_RESIZE_MAX_TAPS,
                     "fm_resize_axis_table: %d -> %d antialiased needs windows wider than FM_RESIZE_MAX_TAPS = %d pixels", n_in, n_out, FM_RESIZE_MAX_TAPS);
    std::vector<double> w;
    std::vector<int> st(n_out), ct(n_out);
    int taps = 0;
    for (int o = 0; o < n_out; ++o) {
        st[o] = resize_axis_row(n_in, n_out, mode, o, w);
        ct[o] = (int)w.size();
        FM_CHECK_ARG(st[o] >= 0 && ct[o] >= 1 && st[o] + ct[o] <= n_in, "fm_resize_axis_table: window of output %d outside the input", o);
        FM_CHECK_ARG(o == 0 || (st[o] >= st[o - 1] && st[o] + ct[o] >= st[o - 1] + ct[o - 1]), "fm_resize_axis_table: windows are not monotone at output %d", o);
        if (ct[o] > taps) taps = ct[o];
    }
    FM_CHECK_ARG(taps <= FM_RESIZE_MAX_TAPS, "fm_resize_axis_table: %d -> %d needs windows of %d pixels, more than FM_RESIZE_MAX_TAPS = %d", n_in, n_out, taps,
                 FM_RESIZE_MAX_TAPS);
    for (int o = 0; o < n_out; ++o) {
        if (start) start[o] = st[o];
        if (count) count[o] = ct[o];
        if (weights || weights_f64) {
            resize_axis_row(n_in, n_out, mode, o, w);
            for (int k = 0; k < taps; ++k) {
                const double v = k < (int)w.size() ? w[k] : 0.0;
                if (weights) weights[(size_t)o * taps + k] = (float)v;
                if (weights_f64) weights_f64[(size_t)o * taps + k] = v;
            }
        }
    }
    if (t_start || t_count) {
        // input i is read by outputs [first, last]: both do not decrease with i because start and start + count do not decrease with o
        std::vector<int> ts(n_in, 0), tc(n_in, 0);
        for (int o = 0; o < n_out; ++o)
            for (int i = st[o]; i < st[o] + ct[o]; ++i) {
                if (tc[i] == 0) ts[i] = o;
                FM_CHECK_ARG(ts[i] + tc[i] == o, "fm_resize_axis_table: the outputs reading input %d are not contiguous", i);
                ++tc[i];
            }
        int next = n_out;
        for (int i = n_in - 1; i >= 0; --i) {
            if (tc[i] == 0) ts[i] = next;                                           // read by no output: an empty range in order
            next = ts[i];
        }
        for (int i = 0; i < n_in; ++i) {
            if (t_start) t_start[i] = ts[i];
            if (t_count) t_count[i] = tc[i];
        }
    }
    return taps;
}
