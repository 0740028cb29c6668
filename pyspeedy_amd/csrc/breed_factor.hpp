// Orthonormalised breeding: the small triangular factorisation behind the Gram matrix of a family of bred members (DESIGN
// section 4k; spd_breed_factor_host and breed_factor_kernel of breed.hip run this one routine).
//
// G = R^T R with R upper triangular, then C = target * R^-1.  Every operation is rounded on its own, and the order of the
// operations of an entry is the definition's (include/pyspeedy_amd.h): R_ij = (G_ij - R_1i R_1j - ... - R_(i-1)i R_(i-1)j) / R_ii,
// R_jj = sqrt(G_jj - R_1j^2 - ...), C_jj = target / R_jj, C_ij = -(0 + R_i(i+1) C_(i+1)j + ... + R_ij C_jj) / R_ii.  The entries are
// spread over `lanes` lanes: R row by row with a lane per column (every lane forms the row's diagonal for itself: it decides, the
// same way in all of them, whether the family breaks there), C with a lane per column.  The host runs it with one lane.
#pragma once
#include <hip/hip_runtime.h>

namespace spd {

constexpr int kBreedMaxFamily = 64;  // members of one family that can be orthogonalised; the leading dimension of R and C

namespace breed_ops {
// one rounding each: the __d*_rn intrinsics on the device, plain IEEE operations that nothing can contract on the host
__host__ __device__ inline double mul(double a, double b) {
#pragma clang fp contract(off)
#if defined(__HIP_DEVICE_COMPILE__)
    return __dmul_rn(a, b);
#else
    return a * b;
#endif
}
__host__ __device__ inline double add(double a, double b) {
#pragma clang fp contract(off)
#if defined(__HIP_DEVICE_COMPILE__)
    return __dadd_rn(a, b);
#else
    return a + b;
#endif
}
__host__ __device__ inline double sub(double a, double b) {
#pragma clang fp contract(off)
#if defined(__HIP_DEVICE_COMPILE__)
    return __dsub_rn(a, b);
#else
    return a - b;
#endif
}
__host__ __device__ inline double div(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __ddiv_rn(a, b);
#else
    return a / b;
#endif
}
__host__ __device__ inline double root(double a) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __dsqrt_rn(a);
#else
    return __builtin_sqrt(a);
#endif
}
}  // namespace breed_ops

// a[64][64]: G in the upper triangle (i <= j < r) on entry, R on return.  c[64][64]: C's upper triangle.  Only rows and columns
// below the returned rank are meaningful: the family breaks at the first j whose radicand is not a finite number > 0.  `barrier`
// stands between what one lane writes and another reads.
template <class Barrier>
__host__ __device__ inline int breed_factor(double *a, double *c, int r, double target, int lane, int lanes, Barrier barrier) {
    using namespace breed_ops;
    constexpr int LD = kBreedMaxFamily;
    int rank = r;
    for (int i = 0; i < r; ++i) {
        double d = a[i * LD + i];
        for (int k = 0; k < i; ++k) d = sub(d, mul(a[k * LD + i], a[k * LD + i]));
        if (!(d > 0.0) || !(d < __builtin_inf())) {
            rank = i;
            break;
        }
        const double rii = root(d);
        barrier();  // (every lane has read G_ii)
        if (lane == 0) a[i * LD + i] = rii;
        for (int j = i + 1 + lane; j < r; j += lanes) {
            double acc = a[i * LD + j];
            for (int k = 0; k < i; ++k) acc = sub(acc, mul(a[k * LD + i], a[k * LD + j]));
            a[i * LD + j] = div(acc, rii);
        }
        barrier();
    }
    barrier();
    for (int j = lane; j < rank; j += lanes) {
        c[j * LD + j] = div(target, a[j * LD + j]);
        for (int i = j - 1; i >= 0; --i) {
            double acc = 0.0;
            for (int k = i + 1; k <= j; ++k) acc = add(acc, mul(a[i * LD + k], c[k * LD + j]));
            c[i * LD + j] = div(-acc, a[i * LD + i]);
        }
    }
    barrier();
    return rank;
}

}  // namespace spd
