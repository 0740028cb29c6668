// Derived grid-space fields (spd_model_derive_*, include/pyspeedy_amd.h; the definition: DESIGN section 4m): the vertical
// velocity of the model's own continuity equation, relative humidity, potential temperature, the column integrals of water
// vapour, its transport and kinetic energy, and the pressure-level forms of omega, vorticity, divergence, rh and theta.
//
// A streaming kernel of plev_kernel's shape: a lane owns one column of one member (coalesced over the 4608 points of a plane),
// loads the eight levels of each input its outputs need once, all loads before the first use, and writes every requested plane.
// Columns stay in registers: sums and the sigma-dot recursion are unrolled, a pressure level picks its layer by unrolled
// selects (plev_layer.hpp).  Two instantiations, so that neither holds more than it needs: {omega_grid, omega_plev} with u, v,
// div and grad ln ps, and the rest with u, v, T, q, vor, div.  Branches on the mask are uniform.  No atomics, no LDS.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "derive.hpp"
#include "model_state.hpp"
#include "plev_layer.hpp"
#include "vertical_consts.hpp"

namespace spd {

hipError_t run_spec2grid_table(const DeviceTables &T, const FieldDesc *table, int nfields, hipStream_t st);

namespace {
constexpr int kT = 256;

using plevl::clamped_value;
using plevl::load8;

// humidity.f90:44-76 for one point (fp32 literals widened as physics.hip's qsat_point does), p = sigma ps in units of p0; g/kg
__device__ __forceinline__ double qsat_point(double ta, double p) {
    const double e0 = 6.108e-3, c1 = 17.269f, c2 = 21.875f, t0 = 273.16f, t1 = 35.86f, t2 = 7.66f;
    const double e = (ta >= t0) ? e0 * exp(c1 * (ta - t0) / (ta - t1)) : e0 * exp(c2 * (ta - t0) / (ta - t2));
    return 622.0f * e / (p - 0.378f * e);
}

// surface pressure in Pa (raw: from ln(ps / p0) exactly as export_units_kernel forms it)
__device__ __forceinline__ double surface_pressure(double ps_in, int raw) { return raw ? static_cast<double>(1.e+5f) * exp(ps_in) : ps_in; }

// G = 0: omega_grid, omega_plev; G = 1: every other output.  blockIdx.x: points, blockIdx.y: member of the launch
template <int G>
__global__ __launch_bounds__(kT) void derive_kernel(const DeriveArgs a) {
    const int p = blockIdx.x * kT + threadIdx.x;
    if (p >= NG) return;
    const long i = a.first + static_cast<long>(blockIdx.y);
    auto want = [&](int v) { return (a.mask >> v & 1) != 0; };
    auto in = [&](int x) { return a.in[x] + i * a.in_stride[x] + p; };
    auto out = [&](int v) { return a.out[v] + i * a.out_stride[v] + p; };
    if constexpr (G == 0) {
        double u[KX], v[KX], d[KX];
        load8(u, in(DIN_U));
        load8(v, in(DIN_V));
        load8(d, in(DIN_DIV));
        const double ps_in = a.ps[i * a.ps_stride + p], px = a.px[i * a.px_stride + p], py = a.py[i * a.py_stride + p];
        __builtin_amdgcn_sched_barrier(0);  // (all 27 loads are in flight before the first value is used)
        const double ps = surface_pressure(ps_in, a.raw);
        // the model's discrete continuity equation (tendencies.f90:152-164; dyn_column.hpp), on the sampled time level
        double ubar = u[0] * vc::dhs[0], vbar = v[0] * vc::dhs[0], dbar = d[0] * vc::dhs[0];
#pragma unroll
        for (int k = 1; k < KX; ++k) {
            ubar = ubar + u[k] * vc::dhs[k];
            vbar = vbar + v[k] * vc::dhs[k];
            dbar = dbar + d[k] * vc::dhs[k];
        }
        const double dlnps = -ubar * px - vbar * py - dbar;
        double om[KX], sd = 0.0;
#pragma unroll
        for (int k = 0; k < KX; ++k) {
            const double puv = (u[k] - ubar) * px + (v[k] - vbar) * py;
            const double sd_next = sd - vc::dhs[k] * (puv + d[k] - dbar);
            om[k] = ps * (vc::fsg[k] * (dlnps + u[k] * px + v[k] * py) + 0.5 * (sd + sd_next));
            sd = sd_next;
        }
        if (want(DRV_OMEGA)) {
#pragma unroll
            for (int k = 0; k < KX; ++k) out(DRV_OMEGA)[static_cast<long>(k) * NG] = om[k];
        }
        if (want(DRV_OMEGA_P)) {
            const double lnps = log(ps);
            for (int j = 0; j < a.n; ++j) out(DRV_OMEGA_P)[static_cast<long>(j) * NG] = clamped_value(om, plevl::find_layer(a.lnp[j] - lnps));
        }
    } else {
        const bool want_rh = want(DRV_RH) || want(DRV_RH_P), want_th = want(DRV_THETA) || want(DRV_THETA_P);
        const bool want_ke = want(DRV_KE), want_ivtu = want(DRV_IVTU), want_ivtv = want(DRV_IVTV), want_tcwv = want(DRV_TCWV);
        const bool want_vor = want(DRV_VOR_P), want_div = want(DRV_DIV_P);
        double u[KX] = {}, v[KX] = {}, t[KX] = {}, q[KX] = {}, vor[KX] = {}, dv[KX] = {};
        if (want_ke || want_ivtu) load8(u, in(DIN_U));
        if (want_ke || want_ivtv) load8(v, in(DIN_V));
        if (want_rh || want_th) load8(t, in(DIN_T));
        if (want_rh || want_tcwv || want_ivtu || want_ivtv) load8(q, in(DIN_Q));
        if (want_vor) load8(vor, in(DIN_VOR));
        if (want_div) load8(dv, in(DIN_DIV));
        const double ps_in = a.ps[i * a.ps_stride + p];
        __builtin_amdgcn_sched_barrier(0);  // (every load is in flight before the first value is used)
        const double ps = surface_pressure(ps_in, a.raw);
        if (a.raw) {
#pragma unroll
            for (int k = 0; k < KX; ++k) q[k] = q[k] * static_cast<double>(1.0e-3f);
        }
        const double psg = ps / phc::grav;
        if (want_tcwv) {
            double s = q[0] * vc::dhs[0];
#pragma unroll
            for (int k = 1; k < KX; ++k) s = s + q[k] * vc::dhs[k];
            *out(DRV_TCWV) = psg * s;
        }
        if (want_ivtu) {
            double s = q[0] * u[0] * vc::dhs[0];
#pragma unroll
            for (int k = 1; k < KX; ++k) s = s + q[k] * u[k] * vc::dhs[k];
            *out(DRV_IVTU) = psg * s;
        }
        if (want_ivtv) {
            double s = q[0] * v[0] * vc::dhs[0];
#pragma unroll
            for (int k = 1; k < KX; ++k) s = s + q[k] * v[k] * vc::dhs[k];
            *out(DRV_IVTV) = psg * s;
        }
        if (want_ke) {
            double s = 0.5 * (u[0] * u[0] + v[0] * v[0]) * vc::dhs[0];
#pragma unroll
            for (int k = 1; k < KX; ++k) s = s + 0.5 * (u[k] * u[k] + v[k] * v[k]) * vc::dhs[k];
            *out(DRV_KE) = psg * s;
        }
        double rh[KX] = {}, th[KX] = {};
        if (want_rh) {
            const double psn = ps / phc::p0;  // in units of p0, and q in g/kg, as the model's formula takes them
#pragma unroll
            for (int k = 0; k < KX; ++k) rh[k] = (q[k] * 1000.0) / qsat_point(t[k], vc::fsg[k] * psn);
            if (want(DRV_RH)) {
#pragma unroll
                for (int k = 0; k < KX; ++k) out(DRV_RH)[static_cast<long>(k) * NG] = rh[k];
            }
        }
        if (want_th) {
#pragma unroll
            for (int k = 0; k < KX; ++k) th[k] = t[k] * pow(phc::p0 / (vc::fsg[k] * ps), phc::akap);
            if (want(DRV_THETA)) {
#pragma unroll
                for (int k = 0; k < KX; ++k) out(DRV_THETA)[static_cast<long>(k) * NG] = th[k];
            }
        }
        if (a.mask & kDerivePlevMask) {
            const double lnps = log(ps);
            for (int j = 0; j < a.n; ++j) {
                const plevl::Layer layer = plevl::find_layer(a.lnp[j] - lnps);
                const long o = static_cast<long>(j) * NG;
                if (want_vor) out(DRV_VOR_P)[o] = clamped_value(vor, layer);
                if (want_div) out(DRV_DIV_P)[o] = clamped_value(dv, layer);
                if (want(DRV_RH_P)) out(DRV_RH_P)[o] = clamped_value(rh, layer);
                if (want(DRV_THETA_P)) out(DRV_THETA_P)[o] = clamped_value(th, layer);
            }
        }
    }
}
}  // namespace

hipError_t run_derive(const DeriveArgs &args, int count, hipStream_t s) {
    if (count == 0 || args.mask == 0) return hipSuccess;
    const dim3 grid((NG + kT - 1) / kT, count);
    if (args.mask & kDeriveOmegaMask) hipLaunchKernelGGL(derive_kernel<0>, grid, dim3(kT), 0, s, args);
    if (args.mask & ~kDeriveOmegaMask) hipLaunchKernelGGL(derive_kernel<1>, grid, dim3(kT), 0, s, args);
    return hipGetLastError();
}

}  // namespace spd

// ---- host side: the C ABI (spd_model_derive_*) ----

namespace {
constexpr int kDeriveNames = 2 + DRV_NVARS;
const char *const kDeriveList = "(" SPD_DERIVED_NAMES ")";
// vor_grid, div_grid: 0, 1; the kernel's outputs: 2 + DeriveVar; anything else: -1
int derive_id(const char *name) {
    const int id = name ? stats_id(name) : -1;
    if (id < 0) return -1;
    if (id == kVorGrid || id == kVorGrid + 1) return id - kVorGrid;
    return cat_kind(id) == CAT_DERIVE ? 2 + (id - kDeriveFirst) : -1;
}
bool derive_on_plev(int v) { return v >= 2 && (kDerivePlevMask >> (v - 2) & 1); }
int derive_name_levels(int v, int n) { return v < 2 ? KX : derive_levels(v - 2, n); }
}  // namespace

extern "C" {

int spd_model_derive_compute(spd_model_handle m, const char *const *names, int n_names, int first, int count, int refresh, void *stream) {
    const char *who = "spd_model_derive_compute";
    // (the arguments first, in the header's order: nothing in this block needs the device or a model)
    if (n_names < 0 || (n_names > 0 && !names)) return m_fail(SPD_E_ARG, std::string(who) + ": bad list of variable names");
    int asked = 0;
    for (int k = 0; k < n_names; ++k) {
        const int v = derive_id(names[k]);
        if (v < 0) return m_fail(SPD_E_ARG, std::string(who) + ": unknown variable '" + (names[k] ? names[k] : "(null)") + "' " + kDeriveList);
        if (asked >> v & 1) return m_fail(SPD_E_ARG, std::string(who) + ": variable '" + names[k] + "' named twice");
        asked |= 1 << v;
    }
    if (int rc = member_range(m, first, count, who)) return rc;
    const int n = m->plev.n;
    if (n_names == 0)  // every name that can be computed: the pressure-level ones only where target levels are configured
        for (int v = 0; v < kDeriveNames; ++v)
            if (n > 0 || !derive_on_plev(v)) asked |= 1 << v;
    for (int k = 0; k < n_names; ++k)
        if (n == 0 && derive_on_plev(derive_id(names[k])))
            return levels_first(who, names[k]);
    M_HIP(hipSetDevice(m->ctx->device));
    spd_model::Derive &dr = m->derive;
    const size_t M = static_cast<size_t>(m->M);
    const int mask = asked >> 2;  // of the kernel
    int needs = 0;
    for (int v = 0; v < DRV_NVARS; ++v)
        if (mask >> v & 1) needs |= kDeriveNeeds[v];
    const bool xf = (asked & 3) || (needs & (1 << DIN_VOR | 1 << DIN_DIV | kDinGrad));
    // the result arrays; vor_grid and div_grid are the destinations of the transforms below as well, whoever needs them
    for (int v = 0; v < kDeriveNames; ++v) {
        const int levels = derive_name_levels(v, n);
        if (!((asked >> v & 1) || (v < 2 && xf)) || dr.cap[v] >= levels) continue;
        if (int rc = dalloc(m, M * levels * NG, &dr.out[v])) return rc;
        dr.cap[v] = levels;
    }
    if (xf && !dr.table) {  // vor, div and grad ln ps of every member: 18 transforms each, as the step's own entries form them
        if (int rc = dalloc(m, 2 * M * NG, &dr.grad)) return rc;
        double *raw = nullptr;
        static_assert(sizeof(FieldDesc) % sizeof(double) == 0, "the table is carved in doubles");
        if (int rc = dalloc(m, M * 18 * (sizeof(FieldDesc) / sizeof(double)), &raw)) return rc;
        std::vector<FieldDesc> host;
        host.reserve(M * 18);
        auto spec = [](double *base, size_t field) { return base + field * NSPEC * C; };
        for (size_t i = 0; i < M; ++i) {
            for (int k = 0; k < KX; ++k) host.push_back({spec(m->P.vor, i * 16 + k), dr.out[0] + (i * KX + k) * NG, 1, 0});
            for (int k = 0; k < KX; ++k) host.push_back({spec(m->P.div, i * 16 + k), dr.out[1] + (i * KX + k) * NG, 1, 0});
            host.push_back({spec(m->P.ps, i * 2), dr.grad + i * NG, 2, 3, nullptr});
            host.push_back({spec(m->P.ps, i * 2), dr.grad + (M + i) * NG, 2, 4, nullptr});
        }
        M_HIP(hipMemcpy(raw, host.data(), host.size() * sizeof(FieldDesc), hipMemcpyHostToDevice));
        dr.table = reinterpret_cast<FieldDesc *>(raw);
    }
    if (count == 0) return SPD_OK;
    if (refresh && (needs & (1 << DIN_U | 1 << DIN_V | 1 << DIN_T | 1 << DIN_Q | kDinPs)))
        if (int rc = spd_model_spectral2grid(m, first, count, stream)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = hipSuccess;
    if (xf) e = run_spec2grid_table(m->ctx->dev, dr.table + static_cast<size_t>(first) * 18, count * 18, s);
    if (e == hipSuccess && mask) {
        DeriveArgs a{};
        const double *in[DIN_N] = {m->u_grid, m->v_grid, m->t_grid, m->q_grid, dr.out[0], dr.out[1]};
        for (int x = 0; x < DIN_N; ++x) {
            a.in[x] = in[x];
            a.in_stride[x] = static_cast<long>(KX) * NG;
        }
        a.ps = m->ps_grid;
        a.px = dr.grad;
        a.py = dr.grad ? dr.grad + M * NG : nullptr;
        a.ps_stride = a.px_stride = a.py_stride = NG;
        for (int v = 0; v < DRV_NVARS; ++v) {
            a.out[v] = dr.out[2 + v];
            a.out_stride[v] = static_cast<long>(derive_levels(v, n)) * NG;
        }
        a.mask = mask;
        a.raw = 0;
        a.n = n;
        a.first = first;
        std::copy(m->plev.lnp, m->plev.lnp + kPlevMaxLevels, a.lnp);
        e = run_derive(a, count, s);
    }
    if (e != hipSuccess) return m_fail(SPD_E_DEVICE, std::string(who) + ": " + hipGetErrorString(e));
    for (int v = 0; v < kDeriveNames; ++v) dr.have[v] = dr.have[v] || (asked >> v & 1);
    return SPD_OK;
}

int spd_model_derive_read(spd_model_handle m, const char *name, int first, int count, void *dst_device, size_t dst_bytes, void *stream) {
    const char *who = "spd_model_derive_read";
    if (!name || !dst_device) return m_fail(SPD_E_ARG, std::string(who) + ": null argument");
    const int v = derive_id(name);
    if (v < 0) return m_fail(SPD_E_ARG, std::string(who) + ": unknown variable '" + name + "' " + kDeriveList);
    if (int rc = member_range(m, first, count, who)) return rc;
    const spd_model::Derive &dr = m->derive;
    if (derive_on_plev(v) && m->plev.n == 0)
        return levels_first(who, name);
    if (!dr.have[v]) return m_fail(SPD_E_ARG, std::string(who) + ": '" + name + "' has not been computed (spd_model_derive_compute)");
    const size_t per = static_cast<size_t>(derive_name_levels(v, m->plev.n)) * NG, need = static_cast<size_t>(count) * per * sizeof(double);
    if (dst_bytes < need) return m_fail(SPD_E_SIZE, std::string(who) + ": destination too small (" + std::to_string(need) + " bytes needed)");
    if (count == 0) return SPD_OK;
    M_HIP(hipSetDevice(m->ctx->device));
    M_HIP(hipMemcpyAsync(dst_device, dr.out[v] + static_cast<size_t>(first) * per, need, hipMemcpyDeviceToDevice,
                         static_cast<hipStream_t>(stream)));
    return SPD_OK;
}

}  // extern "C"
