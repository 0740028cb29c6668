// Nudging: operator-split Newtonian relaxation of the spectral state toward target fields (spd_model_nudge_*,
// include/pyspeedy_amd.h).
//
// After a model step that leaves the step counter at n, for every nudged variable X, level, BOTH time levels and every
// coefficient with total wavenumber l = m + n <= 31:
//   T  = T0 + a * (T1 - T0)        (real and imaginary part separately; left out where the host says T = T0)
//   X' = X + g[l] * (T - X)
// Every operation is rounded on its own: no contraction, so that numpy's x + g * ((t0 + a * (t1 - t0)) - x) gives the same bits.
// Both time levels move alike, which leaves the leapfrog's computational mode alone.  A coefficient with m + n >= 32 is neither
// loaded nor stored: what lies beyond the truncation's halo (triangle.hpp: beyond_halo) stays as it is, bit for bit, and a quiet
// member stays quiet.
// A lane holds one complex coefficient: one 16-byte load of the target (two when it is interpolated) serves both time levels, whose
// 16-byte loads and stores are coalesced along m.  The next step's spectral -> grid launch reads the state at once and the target
// planes are shared by all members: ordinary cached loads and stores.  The interpolation weight and the two slots come by value:
// the device holds no schedule.
#include <hip/hip_runtime.h>

#include "nudge.hpp"
#include "tables.hpp"

namespace spd {

namespace {
constexpr int kT = 256;
constexpr int kBlocks = (NSPEC + kT - 1) / kT;  // 4 blocks over the 992 coefficients; the last one is partial
constexpr int kLmax = TRUNC + 1;                // the largest total wavenumber that is nudged

typedef double double2v __attribute__((ext_vector_type(2)));

// Pointers that come out of the descriptor table are generic to the compiler; they are device-memory addresses.
__device__ __forceinline__ double2v load_global(const double *p) {
    return *(const __attribute__((address_space(1))) double2v *)p;
}
__device__ __forceinline__ void store_global(double *p, double2v v) {
    *(__attribute__((address_space(1))) double2v *)p = v;
}

// blockIdx.x: coefficients, blockIdx.y: plane (descriptor), blockIdx.z: member of the group
__global__ __launch_bounds__(kT) void nudge_kernel(const NudgePlane *__restrict__ planes, const int *__restrict__ mask, int first,
                                                   int s0, int s1, double a) {
#pragma clang fp contract(off)
    const long i = first + static_cast<long>(blockIdx.z);
    if (mask && mask[i] == 0) return;  // (the same for the whole block: nothing of a member that is left alone is loaded)
    const int k = blockIdx.x * kT + threadIdx.x;
    if (k >= NSPEC) return;
    const int n = k / MX, l = k - n * MX + n;
    if (l > kLmax) return;
    const NudgePlane d = planes[blockIdx.y];
    const double g = *(const __attribute__((address_space(1))) double *)(d.gain + l);
    double2v t = load_global(d.target + s0 * d.slot_stride + 2 * k);
    if (s1 != s0) {
        const double2v t1 = load_global(d.target + s1 * d.slot_stride + 2 * k);
        t.x = __dadd_rn(t.x, __dmul_rn(a, __dsub_rn(t1.x, t.x)));
        t.y = __dadd_rn(t.y, __dmul_rn(a, __dsub_rn(t1.y, t.y)));
    }
    double *x0 = d.state + i * d.member_stride + 2 * k, *x1 = x0 + d.level_stride;
    double2v u = load_global(x0), v = load_global(x1);
    u.x = __dadd_rn(u.x, __dmul_rn(g, __dsub_rn(t.x, u.x)));
    u.y = __dadd_rn(u.y, __dmul_rn(g, __dsub_rn(t.y, u.y)));
    v.x = __dadd_rn(v.x, __dmul_rn(g, __dsub_rn(t.x, v.x)));
    v.y = __dadd_rn(v.y, __dmul_rn(g, __dsub_rn(t.y, v.y)));
    store_global(x0, u);
    store_global(x1, v);
}
}  // namespace

hipError_t run_nudge(const NudgePlane *planes, int nplanes, const int *mask, int first, int count, int s0, int s1, double a,
                     hipStream_t s) {
    if (nplanes == 0 || count == 0) return hipSuccess;
    hipLaunchKernelGGL(nudge_kernel, dim3(kBlocks, nplanes, count), dim3(kT), 0, s, planes, mask, first, s0, s1, a);
    return hipGetLastError();
}

}  // namespace spd
