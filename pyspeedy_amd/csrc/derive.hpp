// Derived grid-space fields from the sigma-level grid fields: vertical velocity, relative humidity, potential temperature,
// column integrals, and the pressure-level forms of those and of vorticity and divergence (derive.hip holds the kernel and
// the C ABI: spd_model_derive_* of include/pyspeedy_amd.h; the definition is DESIGN section 4m).
#pragma once
#include <hip/hip_runtime.h>

#include "plev.hpp"
#include "tables.hpp"

namespace spd {

// outputs of the kernel, in the order of DeriveArgs::out (catalogue id = kDeriveFirst + DeriveVar, model_state.hpp)
enum DeriveVar {
    DRV_OMEGA = 0, DRV_RH, DRV_THETA, DRV_TCWV, DRV_IVTU, DRV_IVTV, DRV_KE,
    DRV_OMEGA_P, DRV_VOR_P, DRV_DIV_P, DRV_RH_P, DRV_THETA_P, DRV_NVARS
};
// sigma-level inputs of eight planes, in the order of DeriveArgs::in
enum DeriveIn { DIN_U = 0, DIN_V, DIN_T, DIN_Q, DIN_VOR, DIN_DIV, DIN_N };
// further inputs, as bits behind the DeriveIn ones in a needs mask
constexpr int kDinPs = 1 << DIN_N, kDinGrad = 1 << (DIN_N + 1);

constexpr int kDerivePlevMask = 1 << DRV_OMEGA_P | 1 << DRV_VOR_P | 1 << DRV_DIV_P | 1 << DRV_RH_P | 1 << DRV_THETA_P;
// the two instantiations of the kernel: {omega, its pressure-level form} and the rest
constexpr int kDeriveOmegaMask = 1 << DRV_OMEGA | 1 << DRV_OMEGA_P;
inline constexpr int derive_levels(int v, int n) {
    return v >= DRV_OMEGA_P ? n : (v >= DRV_TCWV ? 1 : KX);
}
// what each output reads (bits of DeriveIn, kDinPs, kDinGrad); ps always
constexpr int kDeriveNeeds[DRV_NVARS] = {
    1 << DIN_U | 1 << DIN_V | 1 << DIN_DIV | kDinPs | kDinGrad,  // omega_grid
    1 << DIN_T | 1 << DIN_Q | kDinPs,                            // rh_grid
    1 << DIN_T | kDinPs,                                         // theta_grid
    1 << DIN_Q | kDinPs,                                         // tcwv
    1 << DIN_Q | 1 << DIN_U | kDinPs,                            // ivt_u
    1 << DIN_Q | 1 << DIN_V | kDinPs,                            // ivt_v
    1 << DIN_U | 1 << DIN_V | kDinPs,                            // ke_col
    1 << DIN_U | 1 << DIN_V | 1 << DIN_DIV | kDinPs | kDinGrad,  // omega_plev
    1 << DIN_VOR | kDinPs,                                       // vor_plev
    1 << DIN_DIV | kDinPs,                                       // div_plev
    1 << DIN_T | 1 << DIN_Q | kDinPs,                            // rh_plev
    1 << DIN_T | kDinPs};                                        // theta_plev

// One launch: members [first, first + count), every output of `mask`.  All arrays are planes of 4608 doubles; `stride` is the
// distance in doubles between two members, consecutive levels of a field are 4608 doubles apart.
struct DeriveArgs {
    const double *in[DIN_N];  // u, v, T, q, vor, div: level 0 (top) of member 0; read only where `mask` needs them
    long in_stride[DIN_N];
    const double *ps;         // surface pressure of member 0, Pa (raw: ln(ps / p0))
    const double *px, *py;    // x and y component of grad ln ps of member 0 (omega only)
    long ps_stride, px_stride, py_stride;
    double *out[DRV_NVARS];   // [member][levels][4608]
    long out_stride[DRV_NVARS];
    int mask;                 // bit v: output v is computed
    int raw;                  // 1: the inputs are the export transforms' raw output (q g/kg, ln(ps / p0)): the export units are
                              // applied here with export_units_kernel's fp32 literals; 0: they are in export units already
    int n;                    // target levels
    int first;
    double lnp[kPlevMaxLevels];  // ln(p_j / Pa), from the host
};

hipError_t run_derive(const DeriveArgs &args, int count, hipStream_t s);

}  // namespace spd
