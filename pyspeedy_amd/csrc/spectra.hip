// Spectra by total wavenumber and global means of the spectral state (spd_model_spectra_*, include/pyspeedy_amd.h; the definition:
// DESIGN section 4d).
//
// Everything here is a plain sum over the coefficients the step's spectral_step_kernel has just written: no transform.  A spectral
// field is complex [32 n][31 m] (k = m + 31 n), the total wavenumber of an element is l = m + n, and a bin holds
//     sum over m = 0 ... min(l, 30) of w_m |f(n = l - m, m)|^2,   w_0 = 1, w_m = 2 otherwise
// (half of it is the global area mean of f^2 at that l; the elements with m + n > 31 take no part).  One workgroup per (member,
// level) stages the planes of that level -- vorticity, divergence, temperature, humidity: 4 x 15 872 B -- into the LDS with
// coalesced 16-byte loads; a ninth workgroup per member does the same for ln ps.  Then 32 lanes per quantity walk one diagonal
// each of the LDS copy, m ascending, with plain fp64 adds in one lane: no atomics, no cross-lane reduction, nothing that depends
// on the launch plan, so a sample is the same bits whatever the member groups, the rounds or the call length.  The products and
// the adds are separate statements: under -ffp-contract=on (Makefile) nothing is fused, and without fast-math nothing reordered.
//
// LDS banks: lane l reads element 31 l - 30 m at step m, a 16-byte read at a lane stride of 31 x 16 B = 124 dwords = -4 modulo the
// 64 banks.  A 16-byte LDS read is served in groups of 16 lanes whose lane numbers are all different modulo 16, so the 16 reads of
// a group fall on the 16 different 4-bank slots of the bank row: the walk is free of conflicts with the row left at 31 elements.
#include <hip/hip_runtime.h>

#include "spectra.hpp"
#include "tables.hpp"

namespace spd {

namespace {
constexpr int kT = 128;            // 4 quantities x 32 bins
constexpr int kLevelSlots = KX + 1;  // blockIdx.x: the eight levels, then ln ps
constexpr double kRootHalf = 0.70710678118654752440;
static_assert(kSpectraBins == NX && kT == 4 * kSpectraBins, "a lane per bin, 32 lanes per quantity");
static_assert(4 * NSPEC * 16 <= 64 * 1024, "the four planes of a level fit the static LDS limit");

typedef double double2v __attribute__((ext_vector_type(2)));

__device__ __forceinline__ void stage(double2v *lds, const double *__restrict__ plane) {
    const double2v *src = reinterpret_cast<const double2v *>(plane);
    for (int e = threadIdx.x; e < NSPEC; e += kT) lds[e] = src[e];
}

// the bin l of a staged plane: m ascending, one lane
__device__ __forceinline__ double bin_sum(const double2v *lds, int l) {
    const int last = l < MX - 1 ? l : MX - 1;
    double sum = 0.0;
    for (int m = 0; m <= last; ++m) {
        const double2v c = lds[(l - m) * MX + m];
        const double re2 = c.x * c.x;
        const double im2 = c.y * c.y;
        const double p = re2 + im2;
        const double wp = m == 0 ? p : 2.0 * p;
        sum = sum + wp;
    }
    return sum;
}

// blockIdx.x: level (KX: ln ps), blockIdx.y: member of the launch
__global__ __launch_bounds__(kT) void spectra_kernel(const SpectraArgs a) {
    __shared__ double2v lds[4][NSPEC];
    const int slot = blockIdx.x;
    const long i = a.first + static_cast<long>(blockIdx.y);
    const long o = i - a.out_first;
    const int q = threadIdx.x / kSpectraBins, l = threadIdx.x % kSpectraBins;
    const bool rot = a.mask & (1u << SPECTRA_KE_ROT), dvg = a.mask & (1u << SPECTRA_KE_DIV), tsp = a.mask & (1u << SPECTRA_T),
               qsp = a.mask & (1u << SPECTRA_Q), psp = a.mask & (1u << SPECTRA_LNPS), tmn = a.mask & (1u << SPECTRA_T_MEAN),
               qmn = a.mask & (1u << SPECTRA_Q_MEAN), pmn = a.mask & (1u << SPECTRA_LNPS_MEAN);
    if (slot == KX) {  // ln ps: one plane per member
        if (!psp && !pmn) return;
        const double *src = a.ps + i * (2L * NSPEC * 2);
        if (psp) {
            stage(lds[0], src);
            __syncthreads();
            if (q == 0) a.out[SPECTRA_LNPS][o * kSpectraBins + l] = 0.5 * bin_sum(lds[0], l);
        }
        if (pmn && threadIdx.x == 0) a.out[SPECTRA_LNPS_MEAN][o] = src[0] * kRootHalf;
        return;
    }
    if (!(a.mask & ~((1u << SPECTRA_LNPS) | (1u << SPECTRA_LNPS_MEAN)))) return;
    const long plane = (i * 2L * KX + slot) * (NSPEC * 2L);  // time level 1, this level
    if (rot) stage(lds[0], a.vor + plane);
    if (dvg) stage(lds[1], a.div + plane);
    if (tsp) stage(lds[2], a.t + plane);
    if (qsp) stage(lds[3], a.tr + plane);
    __syncthreads();
    const long at = (o * KX + slot) * kSpectraBins + l;
    if (q == 0 && rot) a.out[SPECTRA_KE_ROT][at] = 0.25 * (a.elm2[MX * l] * bin_sum(lds[0], l));
    if (q == 1 && dvg) a.out[SPECTRA_KE_DIV][at] = 0.25 * (a.elm2[MX * l] * bin_sum(lds[1], l));
    if (q == 2 && tsp) a.out[SPECTRA_T][at] = 0.5 * bin_sum(lds[2], l);
    if (q == 3 && qsp) a.out[SPECTRA_Q][at] = 0.5 * bin_sum(lds[3], l);
    if (tmn && threadIdx.x == 2 * kSpectraBins) a.out[SPECTRA_T_MEAN][o * KX + slot] = a.t[plane] * kRootHalf;
    if (qmn && threadIdx.x == 3 * kSpectraBins) a.out[SPECTRA_Q_MEAN][o * KX + slot] = a.tr[plane] * kRootHalf;
}

// blockIdx.x: sample of the read, blockIdx.y: member of the read; a lane per double of the entry
__global__ __launch_bounds__(256) void spectra_gather_kernel(const double *__restrict__ src, double *__restrict__ dst, int per, long slot_stride,
                                                             int slot0, int capacity, int nt) {
    const long t = blockIdx.x, z = blockIdx.y;
    const long slot = (slot0 + t) % capacity;
    for (int e = threadIdx.x; e < per; e += 256) dst[(z * nt + t) * per + e] = src[slot * slot_stride + z * per + e];
}
}  // namespace

hipError_t run_spectra(const SpectraArgs &args, int count, hipStream_t s) {
    if (count == 0 || args.mask == 0) return hipSuccess;
    hipLaunchKernelGGL(spectra_kernel, dim3(kLevelSlots, count), dim3(kT), 0, s, args);
    return hipGetLastError();
}

hipError_t run_spectra_gather(const double *src, double *dst, int per, long slot_stride, int count, int nt, int slot0, int capacity,
                              hipStream_t s) {
    if (count == 0 || nt == 0 || per == 0) return hipSuccess;
    constexpr int kMaxY = 32768;  // (grid.y is limited to 65535: a read of many members goes out in pieces)
    for (int z0 = 0; z0 < count; z0 += kMaxY) {
        const int ny = count - z0 < kMaxY ? count - z0 : kMaxY;
        hipLaunchKernelGGL(spectra_gather_kernel, dim3(nt, ny), dim3(256), 0, s, src + static_cast<long>(z0) * per,
                           dst + static_cast<long>(z0) * nt * per, per, slot_stride, slot0, capacity, nt);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace spd
