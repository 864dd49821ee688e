// HOST: Pillow's coefficient table of one axis (include/fourm_hip.h, "Pillow-exact crops"), the one computation behind fm_pil_axis_table
// (pil_resize.hip: the doubles rounded to 22-bit fixed point for the 8-bit path) and fm_pil_axis_table_f64 (pil_resize16.hip: the doubles
// themselves, for the 16-bit path).  Everything in double in Pillow's operation order; the files that include this are compiled with
// -ffp-contract=off so that no multiply-add is contracted.
#pragma once
#include <stdint.h>

#include <vector>

#include "common.h"
#include "fourm_hip.h"

namespace pil_axis {

inline double bilinear_filter(double x) {
    if (x < 0.0) x = -x;
    if (x < 1.0) return 1.0 - x;
    return 0.0;
}

inline double bicubic_filter(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

// Row o of the table of n_in -> n_out: the doubles k (normalised) and the first input pixel.
inline int filter_row(int n_in, int n_out, int filter, int o, std::vector<double>& k) {
    const double scale = (double)n_in / n_out;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = (filter == FM_PIL_BICUBIC ? 2.0 : 1.0) * fs;
    const double center = (o + 0.5) * scale;
    const double ss = 1.0 / fs;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > n_in) xmax = n_in;
    xmax -= xmin;
    k.clear();
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x) {
        const double arg = (x + xmin - center + 0.5) * ss;
        const double w = filter == FM_PIL_BICUBIC ? bicubic_filter(arg) : bilinear_filter(arg);
        k.push_back(w);
        ww += w;
    }
    for (double& v : k)
        if (ww != 0.0) v /= ww;
    return xmin;
}

// start, count (n_out) and coef (n_out, taps) = convert(k), rows padded with convert(0.0); NULLs allowed.  Returns taps, or -1.
// nearest_closed_form: the index of FM_PIL_NEAREST is int((o + 0.5) * a), Pillow's generic affine transform (the one "I;16" images take),
// not the repeated addition of its 8-bit affine scaler.
template <class T, class Convert>
int table(const char* who, int n_in, int n_out, int filter, bool nearest_closed_form, int32_t* start, int32_t* count, T* coef, Convert convert) {
    FM_CHECK_ARG(n_in > 0 && n_out > 0 && n_in <= (1 << 24) && n_out <= (1 << 24), "%s: sizes %d -> %d (1 .. 2^24 each)", who, n_in, n_out);
    FM_CHECK_ARG(filter == FM_PIL_NEAREST || filter == FM_PIL_BILINEAR || filter == FM_PIL_BICUBIC, "%s: filter %d", who, filter);
    if (filter == FM_PIL_NEAREST || n_in == n_out) {          // one tap of weight 1: the affine scaler's index, or the identity of a pass that keeps its size
        const double a = (double)n_in / n_out;
        double xo = a * 0.5;
        for (int o = 0; o < n_out; ++o) {
            int idx = n_in == n_out ? o : nearest_closed_form ? (int)((o + 0.5) * a) : (int)xo;
            if (idx > n_in - 1) idx = n_in - 1;
            if (start) start[o] = idx;
            if (count) count[o] = 1;
            if (coef) coef[o] = convert(1.0);
            xo += a;
        }
        return 1;
    }
    FM_CHECK_ARG((filter == FM_PIL_BICUBIC ? 4.0 : 2.0) * (double)n_in / (double)n_out + 1.0 <= (double)FM_PIL_MAX_TAPS || n_in <= FM_PIL_MAX_TAPS,
                 "%s: %d -> %d needs windows wider than FM_PIL_MAX_TAPS = %d pixels", who, n_in, n_out, FM_PIL_MAX_TAPS);
    std::vector<double> k;
    int taps = 0;
    for (int o = 0; o < n_out; ++o) {
        const int xmin = filter_row(n_in, n_out, filter, o, k);
        const int cnt = (int)k.size();
        FM_CHECK_ARG(xmin >= 0 && cnt >= 0 && xmin + cnt <= n_in, "%s: window of output %d outside the input", who, o);
        if (cnt > taps) taps = cnt;
    }
    FM_CHECK_ARG(taps >= 1 && taps <= FM_PIL_MAX_TAPS, "%s: %d -> %d has windows of %d pixels (1 .. %d)", who, n_in, n_out, taps, FM_PIL_MAX_TAPS);
    for (int o = 0; o < n_out && (start || count || coef); ++o) {
        const int xmin = filter_row(n_in, n_out, filter, o, k);
        if (start) start[o] = xmin;
        if (count) count[o] = (int)k.size();
        if (coef)
            for (int x = 0; x < taps; ++x) coef[(size_t)o * taps + x] = convert(x < (int)k.size() ? k[x] : 0.0);
    }
    return taps;
}

}  // namespace pil_axis
