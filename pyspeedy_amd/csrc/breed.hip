// Breeding: rescale the perturbation of a bred member against its control run (spd_model_breed_*, include/pyspeedy_amd.h;
// DESIGN section 4i).
//
// For a bred member p with control c, D = X_p - X_c on time level 1, w_m = 1 for m = 0 and 2 otherwise, over the 527 coefficients
// with m + n <= 31 of a plane (a level of vor, div, t, tr, or ps):
//   E(vor | div, k) = 1/4 sum elm2(m + n) w_m |D|^2        E(t | tr | ps, k) = 1/2 sum w_m |D|^2
//   A = sqrt(sum over the 33 planes of weight * E),  s = target / A,  X_p' = X_c + s * (X_p - X_c) on both time levels.
// Two launches.  breed_norm_kernel: a workgroup per (plane, bred member) reads the plane of both members with 16-byte loads -- a lane
// holds the coefficients k = lane, lane + 256, lane + 512, lane + 768 and adds their terms in that order -- and the 256 lane sums
// go through a tree in the LDS whose shape is fixed; one partial per plane and member is left in device scratch.  Nothing is
// atomic and nothing depends on which members are bred, on the member groups, the rounds or the call length: A is the same bits in
// every plan.  breed_rescale_kernel: shaped like nudge_kernel; every workgroup first adds its member's 33 weighted partials in
// ascending plane order (the reduce at the launch boundary: the partials are complete when this launch starts), forms A and s
// uniformly, and then moves its coefficients.  Every operation is rounded on its own (no contraction, the __d*_rn intrinsics), so
// that numpy's xc + s * (xp - xc) gives the same bits.  A coefficient with m + n >= 32 is neither loaded nor stored: a quiet member
// stays quiet.  Only bred members are written, and a control is never bred: no workgroup reads what another one writes.
#include <hip/hip_runtime.h>

#include "breed.hpp"
#include "tables.hpp"

namespace spd {

namespace {
constexpr int kT = 256;
constexpr int kBlocks = (NSPEC + kT - 1) / kT;  // 4 blocks (or 4 coefficients a lane) over the 992 coefficients
constexpr int kLmax = TRUNC + 1;                // the largest total wavenumber that takes part

typedef double double2v __attribute__((ext_vector_type(2)));

// Pointers that come out of the descriptor table are generic to the compiler; they are device-memory addresses.
__device__ __forceinline__ double2v load_global(const double *p) {
    return *(const __attribute__((address_space(1))) double2v *)p;
}
__device__ __forceinline__ void store_global(double *p, double2v v) {
    *(__attribute__((address_space(1))) double2v *)p = v;
}

// blockIdx.x: plane, blockIdx.y: bred member
__global__ __launch_bounds__(kT) void breed_norm_kernel(const BreedPlane *__restrict__ planes, const BreedPair *__restrict__ pairs,
                                                        const double *__restrict__ elm2, double *__restrict__ partial) {
#pragma clang fp contract(off)
    __shared__ double tree[kT];
    const BreedPlane d = planes[blockIdx.x];
    const BreedPair pr = pairs[blockIdx.y];
    const double *xp = d.state + pr.member * d.member_stride, *xc = d.state + pr.control * d.member_stride;
    double sum = 0.0;
    for (int j = 0; j < kBlocks; ++j) {
        const int k = j * kT + threadIdx.x;
        if (k >= NSPEC) break;
        const int n = k / MX, m = k - n * MX, l = m + n;
        if (l > kLmax) continue;
        const double2v p = load_global(xp + 2 * k), c = load_global(xc + 2 * k);
        const double dx = __dsub_rn(p.x, c.x), dy = __dsub_rn(p.y, c.y);
        double q = __dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy));
        if (m != 0) q = __dmul_rn(2.0, q);
        if (d.kinetic) q = __dmul_rn(elm2[MX * l], q);
        sum = __dadd_rn(sum, q);
    }
    tree[threadIdx.x] = sum;
    __syncthreads();
    for (int half = kT / 2; half > 0; half >>= 1) {
        if (threadIdx.x < half) tree[threadIdx.x] = __dadd_rn(tree[threadIdx.x], tree[threadIdx.x + half]);
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.y * kBreedPlanes + blockIdx.x] = __dmul_rn(d.kinetic ? 0.25 : 0.5, tree[0]);
}

// the amplitude of bred member b from its partials: ascending plane order; a plane of weight zero takes no part
__device__ __forceinline__ double amplitude_of(const BreedPlane *__restrict__ planes, const double *__restrict__ partial, int b) {
#pragma clang fp contract(off)
    double sum = 0.0;
    for (int p = 0; p < kBreedPlanes; ++p) {
        const double w = planes[p].weight;
        if (w != 0.0) sum = __dadd_rn(sum, __dmul_rn(w, partial[b * kBreedPlanes + p]));
    }
    return __dsqrt_rn(sum);
}

// blockIdx.x: coefficients, blockIdx.y: plane, blockIdx.z: bred member
__global__ __launch_bounds__(kT) void breed_rescale_kernel(const BreedPlane *__restrict__ planes, const BreedPair *__restrict__ pairs,
                                                           const double *__restrict__ partial, double target,
                                                           double *__restrict__ amplitude, double *__restrict__ factor) {
#pragma clang fp contract(off)
    const int b = blockIdx.z;
    const BreedPair pr = pairs[b];
    const double a = amplitude_of(planes, partial, b);
    const bool alone = !(a > 0.0) || !(a < __builtin_inf());  // zero or not finite: s = 1 and not one bit of the member moves
    const double s = alone ? 1.0 : __ddiv_rn(target, a);
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
        if (amplitude) amplitude[pr.member] = a;
        if (factor) factor[pr.member] = s;
    }
    if (alone) return;
    const int k = blockIdx.x * kT + threadIdx.x;
    if (k >= NSPEC) return;
    const int n = k / MX, l = k - n * MX + n;
    if (l > kLmax) return;
    const BreedPlane d = planes[blockIdx.y];
    double *p0 = d.state + pr.member * d.member_stride + 2 * k, *p1 = p0 + d.level_stride;
    const double *c0 = d.state + pr.control * d.member_stride + 2 * k, *c1 = c0 + d.level_stride;
    const double2v xc = load_global(c0), yc = load_global(c1);
    double2v x = load_global(p0), y = load_global(p1);
    x.x = __dadd_rn(xc.x, __dmul_rn(s, __dsub_rn(x.x, xc.x)));
    x.y = __dadd_rn(xc.y, __dmul_rn(s, __dsub_rn(x.y, xc.y)));
    y.x = __dadd_rn(yc.x, __dmul_rn(s, __dsub_rn(y.x, yc.x)));
    y.y = __dadd_rn(yc.y, __dmul_rn(s, __dsub_rn(y.y, yc.y)));
    store_global(p0, x);
    store_global(p1, y);
}

// a lane per member
__global__ __launch_bounds__(kT) void breed_amplitude_kernel(const BreedPlane *__restrict__ planes, const int *__restrict__ slot_of, int members,
                                                             const double *__restrict__ partial, double *__restrict__ out) {
    const int i = blockIdx.x * kT + threadIdx.x;
    if (i >= members) return;
    const int b = slot_of[i];
    out[i] = b < 0 ? 0.0 : amplitude_of(planes, partial, b);
}

}  // namespace

constexpr int kMaxZ = 32768;  // (grid.y and grid.z are limited to 65535: many bred members go out in pieces)

hipError_t run_breed_norm(const BreedPlane *planes, const BreedPair *pairs, int nbred, const double *elm2, double *partial, hipStream_t s) {
    for (int z0 = 0; z0 < nbred; z0 += kMaxZ) {
        const int nz = nbred - z0 < kMaxZ ? nbred - z0 : kMaxZ;
        hipLaunchKernelGGL(breed_norm_kernel, dim3(kBreedPlanes, nz), dim3(kT), 0, s, planes, pairs + z0, elm2,
                           partial + static_cast<long>(z0) * kBreedPlanes);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t run_breed_rescale(const BreedPlane *planes, const BreedPair *pairs, int nbred, const double *partial, double target,
                             double *amplitude, double *factor, hipStream_t s) {
    for (int z0 = 0; z0 < nbred; z0 += kMaxZ) {
        const int nz = nbred - z0 < kMaxZ ? nbred - z0 : kMaxZ;
        hipLaunchKernelGGL(breed_rescale_kernel, dim3(kBlocks, kBreedPlanes, nz), dim3(kT), 0, s, planes, pairs + z0,
                           partial + static_cast<long>(z0) * kBreedPlanes, target, amplitude, factor);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t run_breed_amplitude(const BreedPlane *planes, const int *slot_of, int members, const double *partial, double *out, hipStream_t s) {
    if (members == 0) return hipSuccess;
    hipLaunchKernelGGL(breed_amplitude_kernel, dim3((members + kT - 1) / kT), dim3(kT), 0, s, planes, slot_of, members, partial, out);
    return hipGetLastError();
}

}  // namespace spd
