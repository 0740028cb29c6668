// Order statistics of an ensemble at one grid point: minimum, maximum, quantiles and exceedance probabilities over the members
// (qtape_point_kernel of qtape.hip and spd_qtape_host run these routines).  The header is compiled for the
// device, for the host side of the library and, with no HIP header at all, by the sanitizer program of tests/sanitize/.
//
// At a point the members' values are x_0 ... x_(r-1) in ascending member index, and s_0 ... s_(r-1) is their stable ascending
// order: x_j stands before x_k iff x_j < x_k, or neither is less than the other and j < k (np.sort(kind="stable"); it fixes the
// sign bit where -0.0 and +0.0 meet).  An entry (op, param):
//   min  s_0;   max  s_(r-1)
//   quantile q   h = fl(q (r - 1)), lo = floor(h), f = h - lo (exact), hi = min(lo + 1, r - 1), formed once on the host
//                (qtape_item).  f == 0: s_lo, no arithmetic.  Otherwise v = s_lo + f (s_hi - s_lo), each of the three operations
//                rounded on its own, and v = s_hi if v > s_hi: v lies in [s_lo, s_hi] and does not decrease with q.
//   prob_above thr   #{j : x_j > thr} / r;   prob_below thr   #{j : x_j < thr} / r   (strict; one division, one rounding)
// min and max travel as the selections lo = hi = 0 and lo = hi = r - 1 with f = 0.
//
// The order is made in place by an odd-even transposition with strict swaps: phase p = 0 ... r - 1 compares the neighbours
// (i, i + 1), i = p mod 2, p mod 2 + 2, ..., and exchanges them only where the left one is greater.  Equal values (and the two
// zeros) never pass each other, so the result is the stable order; r phases sort any r values.  Both values of a pair are written
// back whether exchanged or not: the control flow does not depend on the data.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SPD_QTAPE_HD __host__ __device__
#else
#define SPD_QTAPE_HD
#endif

#include <cmath>

namespace spd {

constexpr int kQtapeMax = 64;         // members of the ensemble
constexpr int kQtapeMaxEntries = 64;  // entries of a configuration
constexpr int kQtapeLanes = 64, kQtapePoints = 4608;  // lanes (points) of a workgroup of the kernel; points of a plane
// the ops of the C ABI (SPD_Q_* of include/pyspeedy_amd.h)
constexpr int kQtapeMin = 0, kQtapeMaxOp = 1, kQtapeQuantile = 2, kQtapeProbAbove = 3, kQtapeProbBelow = 4;

// One entry as the kernel finds it.  kind 0: the selection (lo, hi, f); 1 / 2: the share of the members above / below thr.
struct QtapeItem {
    int entry;  // its plane in a ring slot
    int kind, lo, hi;
    double f, thr;
};

// (op, param) for r members -> the descriptor; entry is left 0.  The caller has checked op, q and thr.
inline QtapeItem qtape_item(int op, double param, int r) {
#pragma clang fp contract(off)
    QtapeItem it{0, 0, 0, 0, 0.0, 0.0};
    if (op == kQtapeProbAbove || op == kQtapeProbBelow) {
        it.kind = op == kQtapeProbAbove ? 1 : 2;
        it.thr = param;
        return it;
    }
    const double q = op == kQtapeMin ? 0.0 : op == kQtapeMaxOp ? 1.0 : param;
    const double h = q * static_cast<double>(r - 1);
    const double low = std::floor(h);
    it.lo = static_cast<int>(low);
    it.f = h - low;
    it.hi = it.lo + 1 < r - 1 ? it.lo + 1 : r - 1;
    return it;
}

namespace qtape_ops {
// one rounding each: the intrinsics on the device, plain IEEE operations that nothing can contract on the host
SPD_QTAPE_HD inline double mul(double a, double b) {
#pragma clang fp contract(off)
#if defined(__HIP_DEVICE_COMPILE__)
    return __dmul_rn(a, b);
#else
    return a * b;
#endif
}
SPD_QTAPE_HD inline double add(double a, double b) {
#pragma clang fp contract(off)
#if defined(__HIP_DEVICE_COMPILE__)
    return __dadd_rn(a, b);
#else
    return a + b;
#endif
}
SPD_QTAPE_HD inline double sub(double a, double b) {
#pragma clang fp contract(off)
#if defined(__HIP_DEVICE_COMPILE__)
    return __dsub_rn(a, b);
#else
    return a - b;
#endif
}
SPD_QTAPE_HD inline double div(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __ddiv_rn(a, b);
#else
    return a / b;
#endif
}
}  // namespace qtape_ops

// x.get(j) / x.set(j, v), j = 0 ... r - 1: the members' values at the point (the device: a lane's column of the LDS; the host: a
// local array) -> the stable ascending order, in place.
template <class X>
SPD_QTAPE_HD inline void qtape_sort(const X &x, int r) {
    for (int p = 0; p < r; ++p) {
#pragma unroll 4
        for (int i = p & 1; i + 1 < r; i += 2) {
            const double a = x.get(i), b = x.get(i + 1);
            const bool swap = a > b;
            x.set(i, swap ? b : a);
            x.set(i + 1, swap ? a : b);
        }
    }
}

// one entry from the ordered values s = x.get(0 ... r - 1).  (The counts do not depend on the order.)
template <class X>
SPD_QTAPE_HD inline double qtape_value(const X &x, int r, const QtapeItem &it) {
    using namespace qtape_ops;
    if (it.kind == 0) {
        const double lo = x.get(it.lo);
        if (it.f == 0.0) return lo;
        const double hi = x.get(it.hi);
        const double v = add(lo, mul(it.f, sub(hi, lo)));
        return v > hi ? hi : v;
    }
    int n = 0;
    if (it.kind == 1) {
#pragma unroll 8
        for (int j = 0; j < r; ++j) n += x.get(j) > it.thr ? 1 : 0;
    } else {
#pragma unroll 8
        for (int j = 0; j < r; ++j) n += x.get(j) < it.thr ? 1 : 0;
    }
    return div(static_cast<double>(n), static_cast<double>(r));
}

// One plane's entries on the host, as the kernel forms them: x [r][4608] -> out [n][4608], entry k from items[k].
inline void qtape_plane_host(const double *x, int r, const QtapeItem *items, int n, double *out) {
    struct Local {
        double *at;
        double get(int j) const { return at[j]; }
        void set(int j, double v) const { at[j] = v; }
    };
    double column[kQtapeMax];
    for (int p = 0; p < kQtapePoints; ++p) {
        for (int j = 0; j < r; ++j) column[j] = x[static_cast<long>(j) * kQtapePoints + p];
        qtape_sort(Local{column}, r);
        for (int k = 0; k < n; ++k) out[static_cast<long>(k) * kQtapePoints + p] = qtape_value(Local{column}, r, items[k]);
    }
}

}  // namespace spd
