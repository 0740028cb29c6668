// The recursive time filter of the filter tape for one point: a cascade of second-order sections stepped once per sample (DESIGN
// section 4q; filtape_filter_kernel of filtape.hip and spd_filtape_filter_host run these routines).  The header is compiled for the
// device, for the host side of the library and, with no HIP header at all, by the sanitizer program of tests/sanitize/.
//
// A section is b0, b1, b2, a1, a2 (a0 = 1) with two values of state, s1 and s2; its zero-frequency gain
//   g = ((b0 + b1) + b2) / ((1 + a1) + a2)
// is formed once on the host (fil_gain).  For filter sample k = 1 the section starts in the steady state of a constant input,
//   y = g x,  s1 = y - b0 x,  s2 = b2 x - a2 y,
// and for k > 1 it is the transposed direct form II, both state updates from the state before the sample:
//   y = b0 x + s1,  s1 <- (b1 x - a1 y) + s2,  s2 <- b2 x - a2 y.
// The sections run in order, each section's y the next one's x.  Every operation is rounded on its own.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SPD_FIL_HD __host__ __device__
#else
#define SPD_FIL_HD
#endif

namespace spd {

constexpr int kFilMaxSections = 4, kFilMaxFilters = 8, kFilMaxPlanes = 32, kFilMaxEntries = 64;
constexpr int kFilMean = 0, kFilCov = 1, kFilLast = 2;  // the ops of the C ABI (SPD_FIL_*)

namespace fil_ops {
// one rounding each: the intrinsics on the device, plain IEEE operations that nothing can contract on the host
SPD_FIL_HD inline double mul(double a, double b) {
#pragma clang fp contract(off)
#if defined(__HIP_DEVICE_COMPILE__)
    return __dmul_rn(a, b);
#else
    return a * b;
#endif
}
SPD_FIL_HD inline double add(double a, double b) {
#pragma clang fp contract(off)
#if defined(__HIP_DEVICE_COMPILE__)
    return __dadd_rn(a, b);
#else
    return a + b;
#endif
}
SPD_FIL_HD inline double sub(double a, double b) {
#pragma clang fp contract(off)
#if defined(__HIP_DEVICE_COMPILE__)
    return __dsub_rn(a, b);
#else
    return a - b;
#endif
}
SPD_FIL_HD inline bool finite(double a) { return __builtin_fabs(a) < __builtin_inf(); }  // (false for NaN)
}  // namespace fil_ops

struct FilSection {
    double b0, b1, b2, a1, a2, g;
};

// (host) all five coefficients are numbers / the poles lie inside the unit circle: |a2| < 1 and |a1| < 1 + a2
inline bool fil_section_finite(const double *c) {
    return fil_ops::finite(c[0]) && fil_ops::finite(c[1]) && fil_ops::finite(c[2]) && fil_ops::finite(c[3]) && fil_ops::finite(c[4]);
}
inline bool fil_section_stable(const double *c) { return __builtin_fabs(c[4]) < 1.0 && __builtin_fabs(c[3]) < 1.0 + c[4]; }
// (host) the section with its zero-frequency gain
inline FilSection fil_section(const double *c) {
    const double num = fil_ops::add(fil_ops::add(c[0], c[1]), c[2]), den = fil_ops::add(fil_ops::add(1.0, c[3]), c[4]);
    return FilSection{c[0], c[1], c[2], c[3], c[4], num / den};
}

// filter sample 1 of one section: -> y; the state is written, not read
SPD_FIL_HD inline double fil_first(const FilSection &c, double x, double &s1, double &s2) {
    const double y = fil_ops::mul(c.g, x);
    s1 = fil_ops::sub(y, fil_ops::mul(c.b0, x));
    s2 = fil_ops::sub(fil_ops::mul(c.b2, x), fil_ops::mul(c.a2, y));
    return y;
}
// a later sample of one section: -> y; both state updates use the state before this sample
SPD_FIL_HD inline double fil_next(const FilSection &c, double x, double &s1, double &s2) {
    const double y = fil_ops::add(fil_ops::mul(c.b0, x), s1);
    s1 = fil_ops::add(fil_ops::sub(fil_ops::mul(c.b1, x), fil_ops::mul(c.a1, y)), s2);
    s2 = fil_ops::sub(fil_ops::mul(c.b2, x), fil_ops::mul(c.a2, y));
    return y;
}

// (host) a scalar series through a cascade from filter sample 1 on: y[i] of x[i], i = 0 ... n - 1
inline void fil_series_host(const FilSection *sections, int n_sections, const double *x, int n, double *y) {
    double s1[kFilMaxSections] = {}, s2[kFilMaxSections] = {};
    for (int i = 0; i < n; ++i) {
        double v = x[i];
        for (int s = 0; s < n_sections; ++s) v = i == 0 ? fil_first(sections[s], v, s1[s], s2[s]) : fil_next(sections[s], v, s1[s], s2[s]);
        y[i] = v;
    }
}

}  // namespace spd
