// Verification scores of an ensemble against a truth member: the arithmetic of one grid point and the order of an entry's weighted
// sums (verif_point_kernel and verif_reduce_kernel of verif.hip and spd_verif_host run these routines).  The
// header is compiled for the device, for the host side of the library and, with no HIP header at all, by the sanitizer program of
// tests/sanitize/.
//
// At a point the truth is y and the ensemble x_1 ... x_r in ascending member index.  Every operation is rounded on its own (no
// contraction; the __d*_rn intrinsics on the device), every sum sequential from its first term:
//   s = x_1;  s = s + x_j (j = 2 ... r);  mean = s / r;  e = mean - y;  se = e e
//   a = (x_1 - mean)^2;  a = a + (x_j - mean)^2 (j = 2 ... r);  v = a / (r - 1)
//   b = |x_1 - y|;  b = b + |x_j - y| (j = 2 ... r)
//   c = 0;  c = c + |x_j - x_k| for j = 1 ... r - 1 (outer), k = j + 1 ... r (inner)
//   crps = b / r - c / (r r);  rank = #{j : x_j < y};  tie = 1 if some x_j == y
// An entry (plane, pattern w) is the four weighted sums of e, se, v, crps over the 4608 points in the projection tape's order
// (projtape.hpp), and r + 2 counts over the points with w != 0: bin `rank` for a point without a tie, bin r + 1 for one with.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SPD_VERIF_HD __host__ __device__
#else
#define SPD_VERIF_HD
#endif

namespace spd {

constexpr int kVerifMax = 64;               // members of the ensemble that is scored
constexpr int kVerifCounts = kVerifMax + 2;  // int32 per entry: hist[0 ... r], ties at r + 1, zero behind
constexpr int kVerifLanes = 256, kVerifPasses = 18, kVerifPoints = kVerifLanes * kVerifPasses;  // the projection tape's lanes and passes

namespace verif_ops {
// one rounding each: the intrinsics on the device, plain IEEE operations that nothing can contract on the host
SPD_VERIF_HD inline double mul(double a, double b) {
#pragma clang fp contract(off)
#if defined(__HIP_DEVICE_COMPILE__)
    return __dmul_rn(a, b);
#else
    return a * b;
#endif
}
SPD_VERIF_HD inline double add(double a, double b) {
#pragma clang fp contract(off)
#if defined(__HIP_DEVICE_COMPILE__)
    return __dadd_rn(a, b);
#else
    return a + b;
#endif
}
SPD_VERIF_HD inline double sub(double a, double b) {
#pragma clang fp contract(off)
#if defined(__HIP_DEVICE_COMPILE__)
    return __dsub_rn(a, b);
#else
    return a - b;
#endif
}
SPD_VERIF_HD inline double div(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __ddiv_rn(a, b);
#else
    return a / b;
#endif
}
SPD_VERIF_HD inline double mag(double a) { return __builtin_fabs(a); }
}  // namespace verif_ops

struct VerifPoint {
    double e, se, v, crps;
    int bin;  // rank, or r + 1 for a tie: the count this point adds to
};

// x(j), j = 0 ... r - 1: the ensemble's values at the point in ascending member index (the device reads a lane's column of the
// LDS, the host a strided array); 2 <= r <= kVerifMax.
template <class X>
SPD_VERIF_HD inline VerifPoint verif_point(const X &x, int r, double y) {
    using namespace verif_ops;
    const double rr = static_cast<double>(r);
    const double x0 = x(0);
    double s = x0, b = mag(sub(x0, y));
    int rank = x0 < y ? 1 : 0;
    bool tie = x0 == y;
#pragma unroll 8
    for (int j = 1; j < r; ++j) {
        const double xj = x(j);
        s = add(s, xj);
        b = add(b, mag(sub(xj, y)));
        rank += xj < y ? 1 : 0;
        tie = tie || xj == y;
    }
    const double mean = div(s, rr);
    const double d0 = sub(x0, mean);
    double a = mul(d0, d0);
#pragma unroll 8
    for (int j = 1; j < r; ++j) {
        const double dj = sub(x(j), mean);
        a = add(a, mul(dj, dj));
    }
    double c = 0.0;
    for (int j = 0; j < r - 1; ++j) {
        const double xj = x(j);
#pragma unroll 8
        for (int k = j + 1; k < r; ++k) c = add(c, mag(sub(xj, x(k))));
    }
    VerifPoint out;
    out.e = sub(mean, y);
    out.se = mul(out.e, out.e);
    out.v = div(a, static_cast<double>(r - 1));
    out.crps = sub(div(b, rr), div(c, mul(rr, rr)));
    out.bin = tie ? r + 1 : rank;
    return out;
}

// The halvings of the projection tape's tree from 128 lane sums down, on the host: tree[256] is overwritten.
inline double verif_fold_host(double *tree) {
    for (int half = kVerifLanes / 2; half > 0; half >>= 1)
        for (int t = 0; t < half; ++t) tree[t] = verif_ops::add(tree[t], tree[t + half]);
    return tree[0];
}

// One entry on the host, as the two kernels form it: x [r][4608], y [4608], w [4608] -> out4 = bias, mse, variance, crps and
// hist [kVerifCounts].  scratch: 4 * 256 doubles.
inline void verif_entry_host(const double *x, int r, const double *y, const double *w, double *out4, int *hist, double *scratch) {
    using namespace verif_ops;
    struct Strided {
        const double *at;
        double operator()(int j) const { return at[static_cast<long>(j) * kVerifPoints]; }
    };
    for (int k = 0; k < kVerifCounts; ++k) hist[k] = 0;
    for (int t = 0; t < kVerifLanes; ++t)
        for (int i = 0; i < kVerifPasses; ++i) {
            const int p = t + kVerifLanes * i;
            const VerifPoint q = verif_point(Strided{x + p}, r, y[p]);
            const double term[4] = {mul(w[p], q.e), mul(w[p], q.se), mul(w[p], q.v), mul(w[p], q.crps)};
            for (int k = 0; k < 4; ++k) scratch[k * kVerifLanes + t] = i == 0 ? term[k] : add(scratch[k * kVerifLanes + t], term[k]);
            if (w[p] != 0.0) ++hist[q.bin];
        }
    for (int k = 0; k < 4; ++k) out4[k] = verif_fold_host(scratch + k * kVerifLanes);
}

}  // namespace spd
