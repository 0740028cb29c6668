// Ensemble mean and spread recorded on the GPU inside multi-step calls (spd_model_enstape_*, include/pyspeedy_amd.h).
//
// A sample is what the tape samples (tape.hip): model.hip runs the same front end into a slab of the ensemble tape's own, and the
// fold kernel below reads what tape_store_kernel reads -- the slab's planes, precnv / precls where the column kernel stores them,
// in their stored precision -- applies the same export_unit and, instead of writing every member's value, folds the members of the
// launch in member order into one partial (mean, M2) with Welford's update.  The value of member j that enters is therefore exactly
// what an fp64 tape holds for it; the reduction is the only new arithmetic.  One partial per group stream and slot (enstape.hpp):
// the mean and M2 that come out depend on the launch plan at round-off level and on nothing else.
// Two points (16 bytes of fp64) per lane, coalesced over the 4608 points of a plane.  No LDS, no atomics, no scratch.
#include <hip/hip_runtime.h>

#include <cmath>

#include "enstape.hpp"
#include "export_unit.hpp"
#include "tables.hpp"

namespace spd {

namespace {
constexpr int NG = IX * IL;
constexpr int kT = 256;
constexpr int kPairs = NG / 2;  // 2304 = 9 blocks of 256 lanes: no partial block
static_assert(NG % 2 == 0 && kPairs % kT == 0, "a plane is a whole number of blocks of point pairs");
// Members whose loads are issued before the first of them is folded.  The walk over the members is a chain (each update needs
// the mean before it), and a launch is a few dozen workgroups on 256 compute units: nothing else hides a load's latency, so without
// batches the walk costs one memory round trip per member.  8 members are 8 x 16 bytes in flight per lane and 32 VGPRs; a group of
// the default plan at 64 members (32 members) is four round trips.
constexpr int kBatch = 8;

typedef double double2v __attribute__((ext_vector_type(2)));
typedef float float2v __attribute__((ext_vector_type(2)));

// Pointers that come out of the descriptor table are generic to the compiler (flat loads and stores); they are device-memory
// addresses, and saying so gives the global forms (as tape.hip).
template <typename T>
__device__ __forceinline__ T stream_load_global(const T *p) {
    return __builtin_nontemporal_load((const __attribute__((address_space(1))) T *)p);
}
template <typename T>
__device__ __forceinline__ T load_global(const T *p) {
    return *(const __attribute__((address_space(1))) T *)p;
}
template <typename T>
__device__ __forceinline__ void store_global(T *p, T v) {
    *(__attribute__((address_space(1))) T *)p = v;
}

__device__ __forceinline__ double2v member_value(const double *p) { return stream_load_global(reinterpret_cast<const double2v *>(p)); }
__device__ __forceinline__ double2v member_value(const float *p) {
    const float2v f = stream_load_global(reinterpret_cast<const float2v *>(p));
    double2v x;
    x.x = static_cast<double>(f.x);
    x.y = static_cast<double>(f.y);
    return x;
}

// The walk: members j = 0 ... count - 1 at base + j * stride, kBatch loads ahead of the first update.  A batch past the last member
// loads that member again instead of branching around the load (a branch per load would wait for each one on its own).
template <typename T>
__device__ __forceinline__ void fold_members(const T *base, long stride, int count, int unit, int n0, double2v &mean, double2v &m2) {
    for (int j0 = 0; j0 < count; j0 += kBatch) {
        double2v x[kBatch];
#pragma unroll
        for (int b = 0; b < kBatch; ++b) {
            const int j = j0 + b < count ? j0 + b : count - 1;
            x[b] = member_value(base + j * stride);
        }
#pragma unroll
        for (int b = 0; b < kBatch; ++b) {
            if (j0 + b < count) {  // Welford's update with member j0 + b as the n-th value of the partial
                const double n = static_cast<double>(n0 + j0 + b + 1);
                const double vx = export_unit(x[b].x, unit), vy = export_unit(x[b].y, unit);
                const double dx = vx - mean.x, dy = vy - mean.y;
                mean.x += dx / n;
                mean.y += dy / n;
                m2.x += dx * (vx - mean.x);
                m2.y += dy * (vy - mean.y);
            }
        }
    }
}

// blockIdx.x: pairs of points, blockIdx.y: plane
__global__ __launch_bounds__(kT) void enstape_fold_kernel(const EnsTapePlane *__restrict__ planes, int nplanes,
                                                          const double *__restrict__ slab, int slab_fields, int first, int count,
                                                          int partial, int n0, int store32) {
    const int p = 2 * (blockIdx.x * kT + threadIdx.x);
    if (p >= NG) return;
    const EnsTapePlane d = planes[blockIdx.y];
    const long at = static_cast<long>(partial) * nplanes * NG + p;
    double2v mean = {0.0, 0.0}, m2 = {0.0, 0.0};
    if (n0 > 0) {  // (the first members of a sample's partial: nothing of it is read -- a lap over the ring needs no device work)
        mean = load_global(reinterpret_cast<const double2v *>(d.mean + at));
        m2 = load_global(reinterpret_cast<const double2v *>(d.m2 + at));
    }
    if (d.slab_plane >= 0)
        fold_members(slab + (static_cast<long>(first) * slab_fields + d.slab_plane) * NG + p, static_cast<long>(slab_fields) * NG, count,
                     d.unit, n0, mean, m2);
    else if (store32)
        fold_members(static_cast<const float *>(d.src) + static_cast<long>(first) * NG + p, static_cast<long>(NG), count, d.unit, n0, mean, m2);
    else
        fold_members(static_cast<const double *>(d.src) + static_cast<long>(first) * NG + p, static_cast<long>(NG), count, d.unit, n0, mean, m2);
    // (plain stores: a later round of the same sample reads the partial back, and so does the read)
    store_global(reinterpret_cast<double2v *>(d.mean + at), mean);
    store_global(reinterpret_cast<double2v *>(d.m2 + at), m2);
}

// blockIdx.x: pairs of points of the variable's planes, blockIdx.y: sample of this launch
__global__ __launch_bounds__(kT) void enstape_read_kernel(const double *__restrict__ mean, const double *__restrict__ m2, long per,
                                                          long partial_stride, int kind, int slot0, int capacity, EnsTapeCounts counts,
                                                          double *__restrict__ dst) {
    const long q = 2 * (static_cast<long>(blockIdx.x) * kT + threadIdx.x);
    if (q >= per) return;
    const int t = blockIdx.y;
    const long slot = (slot0 + static_cast<long>(t)) % capacity;
    double2v mu = {0.0, 0.0}, s = {0.0, 0.0};
    double na = 0.0;
    for (int g = 0; g < kEnsTapeGroups; ++g) {  // Chan's merge of the partials that hold members, in the fixed order g = 0 ... 3
        const int c = counts.n[t][g];
        if (c == 0) continue;
        const long at = (slot * kEnsTapeGroups + g) * partial_stride + q;
        const double2v mb = *reinterpret_cast<const double2v *>(mean + at), sb = *reinterpret_cast<const double2v *>(m2 + at);
        const double nb = static_cast<double>(c);
        if (na == 0.0) {
            mu = mb;
            s = sb;
            na = nb;
            continue;
        }
        const double n = na + nb, w = nb / n, ww = na * nb / n;
        const double dx = mb.x - mu.x, dy = mb.y - mu.y;
        mu.x = mu.x + dx * w;
        mu.y = mu.y + dy * w;
        s.x = (s.x + sb.x) + (dx * dx) * ww;
        s.y = (s.y + sb.y) + (dy * dy) * ww;
        na = n;
    }
    double2v out;
    if (kind == 0) {
        out = mu;
    } else if (kind == 2) {
        out = s;
    } else {  // the unbiased standard deviation (one member: 0 / 0, NaN, as stats_ensemble_kernel)
        out.x = sqrt(s.x / (na - 1.0));
        out.y = sqrt(s.y / (na - 1.0));
    }
    *reinterpret_cast<double2v *>(dst + static_cast<long>(t) * per + q) = out;
}
}  // namespace

hipError_t run_enstape_fold(const EnsTapePlane *planes, int nplanes, const double *slab, int slab_fields, int first, int count,
                            int partial, int n0, int store32, hipStream_t s) {
    if (nplanes == 0 || count == 0) return hipSuccess;
    hipLaunchKernelGGL(enstape_fold_kernel, dim3(kPairs / kT, nplanes), dim3(kT), 0, s, planes, nplanes, slab, slab_fields, first, count,
                       partial, n0, store32);
    return hipGetLastError();
}

hipError_t run_enstape_read(const double *mean, const double *m2, long per, int nplanes, int kind, int nt, int slot0, int capacity,
                            const int *counts, double *dst, hipStream_t s) {
    if (nt == 0 || per == 0) return hipSuccess;
    const long pairs = per / 2;  // (a plane is 4608 points: `per` is even)
    for (int t_base = 0; t_base < nt; t_base += kEnsTapeReadSamples) {  // (the counts of a launch travel by value: a long read goes out in pieces)
        const int ny = nt - t_base < kEnsTapeReadSamples ? nt - t_base : kEnsTapeReadSamples;
        EnsTapeCounts c{};
        for (int t = 0; t < ny; ++t)
            for (int g = 0; g < kEnsTapeGroups; ++g) c.n[t][g] = counts[static_cast<size_t>(t_base + t) * kEnsTapeGroups + g];
        hipLaunchKernelGGL(enstape_read_kernel, dim3(static_cast<unsigned>((pairs + kT - 1) / kT), ny), dim3(kT), 0, s, mean, m2, per,
                           static_cast<long>(nplanes) * NG, kind, (slot0 + t_base) % capacity, capacity, c, dst + static_cast<long>(t_base) * per);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace spd
