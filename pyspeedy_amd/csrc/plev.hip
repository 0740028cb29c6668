// Pressure-level interpolation of the grid-space fields and mean sea-level pressure (spd_model_plev_*, include/pyspeedy_amd.h;
// the definition: DESIGN section 4b).
//
// A streaming kernel: a lane owns one column of one member (coalesced over the 4608 points of a plane), loads ps, and the eight
// levels of each variable it needs once, and writes every requested (variable, target level) plane plus mslp.  The eight levels
// of a variable stay in registers: the layer that holds a target pressure is found by walking the layers with the loop unrolled
// and selecting (a runtime index into them would put them in scratch memory).  sigl and the layer reciprocals are compile-time
// constants; ln p_j comes from the host, so a lane takes one log (of ps) and an exp only below the lowest full level (the raw path
// of a statistics sample first forms ps exactly as export_units_kernel does: one more exp, and the same bits as the other path).
#include <hip/hip_runtime.h>

#include <cmath>

#include "plev.hpp"
#include "vertical_consts.hpp"

namespace spd {

namespace {
constexpr int NG = IX * IL;
constexpr int kT = 256;

struct LayerRecip {
    double r[KX - 1];
    constexpr LayerRecip() : r{} {
        for (int k = 0; k < KX - 1; ++k) r[k] = 1.0 / (vc::sigl[k + 1] - vc::sigl[k]);
    }
};
constexpr LayerRecip kRecip{};

__device__ __forceinline__ void load8(double (&x)[KX], const double *__restrict__ base) {
#pragma unroll
    for (int k = 0; k < KX; ++k) x[k] = base[static_cast<long>(k) * NG];
}

// X[k] + w (X[k+1] - X[k]) of the layer the flags select (ge[k]: s >= sigl[k], k = 1 ... 6)
__device__ __forceinline__ double layer_value(const double (&x)[KX], const bool (&ge)[KX - 1], double w) {
    double lo = x[0], hi = x[1];
#pragma unroll
    for (int k = 1; k < KX - 1; ++k) {
        lo = ge[k] ? x[k] : lo;
        hi = ge[k] ? x[k + 1] : hi;
    }
    return lo + w * (hi - lo);
}

// blockIdx.x: points, blockIdx.y: member of the launch
__global__ __launch_bounds__(kT) void plev_kernel(const PlevArgs a) {
    const int p = blockIdx.x * kT + threadIdx.x;
    if (p >= NG) return;
    const long i = a.first + static_cast<long>(blockIdx.y);
    const bool want_u = a.mask & (1 << PLEV_U), want_v = a.mask & (1 << PLEV_V), want_t = a.mask & (1 << PLEV_T),
               want_q = a.mask & (1 << PLEV_Q), want_z = a.mask & (1 << PLEV_Z), want_mslp = a.mask & (1 << PLEV_MSLP);
    double u[KX] = {}, v[KX] = {}, t[KX] = {}, q[KX] = {}, z[KX] = {};
    if (want_u) load8(u, a.in[PLEV_U] + i * a.in_stride[PLEV_U] + p);
    if (want_v) load8(v, a.in[PLEV_V] + i * a.in_stride[PLEV_V] + p);
    if (want_t || want_z)
        load8(t, a.in[PLEV_T] + i * a.in_stride[PLEV_T] + p);
    else if (want_mslp)
        t[KX - 1] = a.in[PLEV_T][i * a.in_stride[PLEV_T] + static_cast<long>(KX - 1) * NG + p];
    if (want_q) load8(q, a.in[PLEV_Q] + i * a.in_stride[PLEV_Q] + p);
    if (want_z) load8(z, a.in[PLEV_Z] + i * a.in_stride[PLEV_Z] + p);
    const double ps_in = a.ps[i * a.ps_stride + p];
    double ps = ps_in;
    if (a.raw) {  // the export units of export_units_kernel (surface.hip), same literals and operations: from here on both paths
                  // hold the same bits, so a sampled field is bitwise the one spd_model_plev_compute gives at that step
#pragma unroll
        for (int k = 0; k < KX; ++k) {
            q[k] = q[k] * static_cast<double>(1.0e-3f);
            z[k] = z[k] / static_cast<double>(9.81f);
        }
        ps = static_cast<double>(1.e+5f) * exp(ps_in);
    }
    const double lnps = log(ps);
    if (want_mslp) {
        const double ts = t[KX - 1] * exp(-plevc::kappa * vc::sigl[KX - 1]);
        const double zs = a.phis0[i * NG + p] / phc::grav;
        a.out[PLEV_MSLP][i * a.out_stride[PLEV_MSLP] + p] = ps * pow(1.0 + plevc::gamma * zs / ts, 1.0 / plevc::kappa);
    }
    for (int j = 0; j < a.n; ++j) {
        const double s = a.lnp[j] - lnps;
        const long o = static_cast<long>(j) * NG + p;
        bool ge[KX - 1];
        double sg = vc::sigl[0], rv = kRecip.r[0];
#pragma unroll
        for (int k = 1; k < KX - 1; ++k) {
            ge[k] = s >= vc::sigl[k];
            sg = ge[k] ? vc::sigl[k] : sg;
            rv = ge[k] ? kRecip.r[k] : rv;
        }
        ge[0] = true;
        const double w = (s - sg) * rv;
        const bool top = s < vc::sigl[0], below = s > vc::sigl[KX - 1];
        if (want_u) a.out[PLEV_U][i * a.out_stride[PLEV_U] + o] = top ? u[0] : below ? u[KX - 1] : layer_value(u, ge, w);
        if (want_v) a.out[PLEV_V][i * a.out_stride[PLEV_V] + o] = top ? v[0] : below ? v[KX - 1] : layer_value(v, ge, w);
        if (want_q) a.out[PLEV_Q][i * a.out_stride[PLEV_Q] + o] = top ? q[0] : below ? q[KX - 1] : layer_value(q, ge, w);
        if (want_t || want_z) {
            double tj, zj;
            if (below) {  // constant lapse rate below the lowest full level, and its hydrostatic integral
                tj = t[KX - 1] * exp(plevc::kappa * (s - vc::sigl[KX - 1]));
                zj = z[KX - 1] - (tj - t[KX - 1]) / plevc::gamma;
            } else if (top) {  // isothermal above the top full level
                tj = t[0];
                zj = z[0] + plevc::rog * t[0] * (vc::sigl[0] - s);
            } else {
                tj = layer_value(t, ge, w);
                zj = layer_value(z, ge, w);
            }
            if (want_t) a.out[PLEV_T][i * a.out_stride[PLEV_T] + o] = tj;
            if (want_z) a.out[PLEV_Z][i * a.out_stride[PLEV_Z] + o] = zj;
        }
    }
}
}  // namespace

hipError_t run_plev(const PlevArgs &args, int count, hipStream_t s) {
    if (count == 0 || args.mask == 0) return hipSuccess;
    hipLaunchKernelGGL(plev_kernel, dim3((NG + kT - 1) / kT, count), dim3(kT), 0, s, args);
    return hipGetLastError();
}

}  // namespace spd
