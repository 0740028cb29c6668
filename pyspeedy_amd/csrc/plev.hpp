// Pressure-level fields and mean sea-level pressure from the sigma-level grid fields (plev.hip holds the kernel, the
// configuration and the C ABI: spd_model_plev_* of include/pyspeedy_amd.h; the definition is DESIGN section 4b).
#pragma once
#include <hip/hip_runtime.h>

#include "tables.hpp"

namespace spd {

constexpr int kPlevMaxLevels = 32;
// variables of the kernel, in the order of PlevArgs::in / out (sigma-level input -> pressure-level output)
enum PlevVar { PLEV_U = 0, PLEV_V, PLEV_T, PLEV_Q, PLEV_Z, PLEV_MSLP, PLEV_NVARS };

// R, g, gamma of the definition: the library's own constants (physical_constants.f90:18-32, fp32 literals widened); gamma in K/m
namespace plevc {
constexpr double gamma = phc::gamma_km / 1000.0;
constexpr double kappa = phc::rgas * gamma / phc::grav;  // R gamma / g
constexpr double rog = phc::rgas / phc::grav;            // R / g
}  // namespace plevc

// One launch: members [first, first + count), every requested variable at every target level.  All arrays are planes of 4608
// doubles; `stride` is the distance in doubles between two members, consecutive levels of a variable are 4608 doubles apart.
struct PlevArgs {
    const double *in[5];   // u, v, T, q, Z: level 0 (top) of member 0; read only where `mask` needs them
    long in_stride[5];
    const double *ps;      // surface pressure of member 0 (raw: ln(ps / p0))
    long ps_stride;
    const double *phis0;   // [M][4608] truncated surface geopotential, m^2/s^2 (mslp only)
    double *out[PLEV_NVARS];  // [member][n][4608] (mslp: [member][4608])
    long out_stride[PLEV_NVARS];
    int mask;              // bit v: variable v is computed
    int raw;               // 1: the inputs are the export transforms' raw output (q g/kg, Z m^2/s^2, ln(ps / p0)): the export units
                           // are applied here with export_units_kernel's fp32 literals; 0: they are in export units already
    int n;                 // target levels
    int first;
    double lnp[kPlevMaxLevels];  // ln(p_j / Pa), from the host
};

hipError_t run_plev(const PlevArgs &args, int count, hipStream_t s);

}  // namespace spd
