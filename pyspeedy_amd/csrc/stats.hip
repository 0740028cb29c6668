// Time-mean statistics accumulated on the GPU inside multi-step calls (spd_model_stats_*, include/pyspeedy_amd.h).
//
// A sample of the prognostic variables is what spd_model_spectral2grid would leave in u_grid ... ps_grid if the call ended at
// that step: model.hip runs the same vort2vel and the same 41-entry export descriptors per member (a second table, built like
// exp_inv_table, whose destinations are a scratch slab instead of the registry's grid arrays), then the accumulate kernel below
// applies the export units with export_units_kernel's fp32 literals and updates the moments.  precnv / precls are read where
// the column kernel stores them, in their stored precision.  Everything is fp64; Welford's update keeps the variance stable
// over long periods.  Streaming kernels: one lane per grid point, coalesced over the 4608 points of a plane.
#include <hip/hip_runtime.h>

#include <cmath>

#include "export_unit.hpp"
#include "stats.hpp"
#include "tables.hpp"

namespace spd {

namespace {
constexpr int NG = IX * IL;
constexpr int kT = 256;

// blockIdx.x: points, blockIdx.y: plane, blockIdx.z: member of the group
__global__ __launch_bounds__(kT) void stats_accumulate_kernel(const StatsPlane *__restrict__ planes, const double *__restrict__ slab,
                                                              int slab_fields, int first, long long n, int store32) {
    const int p = blockIdx.x * kT + threadIdx.x;
    if (p >= NG) return;
    const StatsPlane d = planes[blockIdx.y];
    const long i = first + static_cast<long>(blockIdx.z);
    double x;
    if (d.slab_plane >= 0)
        x = slab[(i * slab_fields + d.slab_plane) * NG + p];
    else if (store32)
        x = static_cast<double>(static_cast<const float *>(d.src)[i * NG + p]);
    else
        x = static_cast<const double *>(d.src)[i * NG + p];
    x = export_unit(x, d.unit);
    double *mean = d.mean + i * d.member_stride + p;
    double *m2 = d.m2 ? d.m2 + i * d.member_stride + p : nullptr;
    if (n == 1) {  // the first sample of a period: nothing is read (reset needs no device work)
        *mean = x;
        if (m2) *m2 = 0.0;
        return;
    }
    const double old = *mean, delta = x - old, now = old + delta / static_cast<double>(n);
    *mean = now;
    if (m2) *m2 = *m2 + delta * (x - now);
}

__global__ __launch_bounds__(kT) void stats_variance_kernel(const double *__restrict__ m2, double *__restrict__ out, long total,
                                                            double denom) {
    const long i = static_cast<long>(blockIdx.x) * kT + threadIdx.x;
    if (i < total) out[i] = m2[i] / denom;
}

// two passes over the members (mean first, then the squared deviations from it): coalesced over points
__global__ __launch_bounds__(kT) void stats_ensemble_kernel(const double *__restrict__ mean, int M, long points, int want_std,
                                                            double *__restrict__ out) {
    const long i = static_cast<long>(blockIdx.x) * kT + threadIdx.x;
    if (i >= points) return;
    double sum = 0.0;
    for (int j = 0; j < M; ++j) sum += mean[j * points + i];
    const double mu = sum / M;
    if (!want_std) {
        out[i] = mu;
        return;
    }
    double ss = 0.0;
    for (int j = 0; j < M; ++j) {
        const double d = mean[j * points + i] - mu;
        ss += d * d;
    }
    out[i] = sqrt(ss / (M - 1));  // (one member: 0 / 0, NaN, as torch.std of one value)
}
}  // namespace

hipError_t run_stats_accumulate(const StatsPlane *planes, int nplanes, const double *slab, int slab_fields, int first, int count,
                                long long n, int store32, hipStream_t s) {
    if (nplanes == 0 || count == 0) return hipSuccess;
    hipLaunchKernelGGL(stats_accumulate_kernel, dim3((NG + kT - 1) / kT, nplanes, count), dim3(kT), 0, s, planes, slab, slab_fields,
                       first, n, store32);
    return hipGetLastError();
}

hipError_t run_stats_variance(const double *m2, double *out, long total, long long n, hipStream_t s) {
    if (total == 0) return hipSuccess;
    hipLaunchKernelGGL(stats_variance_kernel, dim3(static_cast<unsigned>((total + kT - 1) / kT)), dim3(kT), 0, s, m2, out, total,
                       static_cast<double>(n - 1));
    return hipGetLastError();
}

hipError_t run_stats_ensemble(const double *mean, int M, long points, int std, double *out, hipStream_t s) {
    if (points == 0) return hipSuccess;
    hipLaunchKernelGGL(stats_ensemble_kernel, dim3(static_cast<unsigned>((points + kT - 1) / kT)), dim3(kT), 0, s, mean, M, points,
                       std, out);
    return hipGetLastError();
}

}  // namespace spd
