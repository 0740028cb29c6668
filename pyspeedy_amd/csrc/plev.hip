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

#include "model_state.hpp"
#include "plev.hpp"
#include "plev_layer.hpp"
#include "vertical_consts.hpp"

namespace spd {

namespace {
constexpr int kT = 256;

using plevl::layer_value;
using plevl::load8;

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
        const plevl::Layer layer = plevl::find_layer(s);
        const bool(&ge)[KX - 1] = layer.ge;
        const double w = layer.w;
        const bool top = layer.top, below = layer.below;
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

// ---- host side: the configuration and the C ABI (spd_model_plev_*) ----

static int plev_id(const char *name) {
    const int id = name ? stats_id(name) : -1;
    return id >= 0 && cat_kind(id) == CAT_PLEV ? id - kPlevFirst : -1;
}

extern "C" {

int spd_model_plev_configure(spd_model_handle m, const double *levels_pa, int n) {
    const char *who = "spd_model_plev_configure";
    if (n < 0 || (n > 0 && !levels_pa)) return m_fail(SPD_E_ARG, std::string(who) + ": bad list of levels");
    if (n > kPlevMaxLevels) return m_fail(SPD_E_ARG, std::string(who) + ": at most " + std::to_string(kPlevMaxLevels) + " levels");
    for (int j = 0; j < n; ++j)
        if (!(levels_pa[j] > 0.0) || !std::isfinite(levels_pa[j]))
            return m_fail(SPD_E_ARG, std::string(who) + ": level " + std::to_string(j) + " is not a positive pressure (Pa)");
    bool up = true, down = true;
    for (int j = 1; j < n; ++j) {
        up = up && levels_pa[j] > levels_pa[j - 1];
        down = down && levels_pa[j] < levels_pa[j - 1];
    }
    if (!up && !down) return m_fail(SPD_E_ARG, std::string(who) + ": the levels must be strictly increasing or strictly decreasing");
    if (!m) return m_fail(SPD_E_ARG, std::string(who) + ": null model");
    if (int rc = usable(m, who)) return rc;
    if (m->stats.on && m->stats.holds_plev())
        return m_fail(SPD_E_ARG, std::string(who) + ": statistics of a pressure-level variable are configured; switch them off first "
                                                    "(spd_model_stats_configure)");
    if (m->tape.on && m->tape.holds_plev())
        return m_fail(SPD_E_ARG, std::string(who) + ": the tape holds a pressure-level variable; switch it off first (spd_model_tape_configure)");
    if (m->enstape.on && m->enstape.holds_plev())
        return m_fail(SPD_E_ARG, std::string(who) + ": the ensemble tape holds a pressure-level variable; switch it off first "
                                                    "(spd_model_enstape_configure)");
    if (m->wintape.on && m->wintape.holds_plev())
        return m_fail(SPD_E_ARG, std::string(who) + ": the window tape holds a pressure-level variable; switch it off first "
                                                    "(spd_model_wintape_configure)");
    if (m->projtape.on && m->projtape.holds_plev())
        return m_fail(SPD_E_ARG, std::string(who) + ": the projection tape holds a pressure-level variable; switch it off first "
                                                    "(spd_model_projtape_configure)");
    if (m->tracktape.on && m->tracktape.holds_plev())
        return m_fail(SPD_E_ARG, std::string(who) + ": the track tape holds a pressure-level variable; switch it off first "
                                                    "(spd_model_tracktape_configure)");
    if (m->filtape.on && m->filtape.holds_plev())
        return m_fail(SPD_E_ARG, std::string(who) + ": the filter tape holds a pressure-level variable; switch it off first "
                                                    "(spd_model_filtape_off)");
    if (m->verif.on && m->verif.holds_plev())
        return m_fail(SPD_E_ARG, std::string(who) + ": the verification tape holds a pressure-level variable; switch it off first "
                                                    "(spd_model_verif_off)");
    if (m->qtape.on && m->qtape.holds_plev())
        return m_fail(SPD_E_ARG, std::string(who) + ": the quantile tape holds a pressure-level variable; switch it off first "
                                                    "(spd_model_qtape_off)");
    spd_model::Plev &pl = m->plev;
    pl.n = n;
    for (int j = 0; j < kPlevMaxLevels; ++j) {
        pl.levels[j] = j < n ? levels_pa[j] : 0.0;
        pl.lnp[j] = j < n ? std::log(levels_pa[j]) : 0.0;
    }
    for (bool &h : pl.have) h = false;  // (results of the previous levels are not handed out under the new ones)
    for (int v = 0; v < DRV_NVARS; ++v)
        if (kDerivePlevMask >> v & 1) m->derive.have[2 + v] = false;
    return SPD_OK;
}

int spd_model_plev_levels(spd_model_handle m, double *out, int cap) {
    if (!m) return m_fail(SPD_E_ARG, "spd_model_plev_levels: null model");
    if (cap < 0 || (cap > 0 && !out)) return m_fail(SPD_E_ARG, "spd_model_plev_levels: bad destination");
    for (int j = 0; j < m->plev.n && j < cap; ++j) out[j] = m->plev.levels[j];
    return m->plev.n;
}

int spd_model_plev_compute(spd_model_handle m, const char *const *names, int n_names, int first, int count, int refresh, void *stream) {
    const char *who = "spd_model_plev_compute";
    if (n_names < 0 || (n_names > 0 && !names)) return m_fail(SPD_E_ARG, std::string(who) + ": bad list of variable names");
    int mask = n_names == 0 ? (1 << PLEV_NVARS) - 1 : 0;
    for (int k = 0; k < n_names; ++k) {
        const int id = plev_id(names[k]);
        if (id < 0)
            return m_fail(SPD_E_ARG, std::string(who) + ": unknown variable '" + (names[k] ? names[k] : "(null)") +
                                         "' (u_plev, v_plev, t_plev, q_plev, z_plev, mslp)");
        mask |= 1 << id;
    }
    if (int rc = member_range(m, first, count, who)) return rc;
    spd_model::Plev &pl = m->plev;
    if (pl.n == 0) return m_fail(SPD_E_ARG, std::string(who) + ": no target levels configured (spd_model_plev_configure)");
    M_HIP(hipSetDevice(m->ctx->device));
    const size_t M = static_cast<size_t>(m->M);
    for (int v = 0; v < PLEV_NVARS; ++v) {
        const int levels = v == PLEV_MSLP ? 1 : pl.n;
        if (!(mask >> v & 1) || pl.cap[v] >= levels) continue;
        if (int rc = dalloc(m, M * levels * NG, &pl.out[v])) return rc;
        pl.cap[v] = levels;
    }
    if (count == 0) return SPD_OK;
    if (refresh)
        if (int rc = spd_model_spectral2grid(m, first, count, stream)) return rc;
    PlevArgs a{};
    const double *in[5] = {m->u_grid, m->v_grid, m->t_grid, m->q_grid, m->phi_grid};
    for (int x = 0; x < 5; ++x) {
        a.in[x] = in[x];
        a.in_stride[x] = static_cast<long>(KX) * NG;
    }
    a.ps = m->ps_grid;
    a.ps_stride = NG;
    a.phis0 = m->pa.phis0;
    for (int v = 0; v < PLEV_NVARS; ++v) {
        a.out[v] = pl.out[v];
        a.out_stride[v] = static_cast<long>(v == PLEV_MSLP ? 1 : pl.n) * NG;
    }
    a.mask = mask;
    a.raw = 0;
    a.n = pl.n;
    a.first = first;
    std::copy(pl.lnp, pl.lnp + kPlevMaxLevels, a.lnp);
    const hipError_t e = run_plev(a, count, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return m_fail(SPD_E_DEVICE, std::string(who) + ": " + hipGetErrorString(e));
    for (int v = 0; v < PLEV_NVARS; ++v) pl.have[v] = pl.have[v] || (mask >> v & 1);
    return SPD_OK;
}

int spd_model_plev_read(spd_model_handle m, const char *name, int first, int count, void *dst_device, size_t dst_bytes, void *stream) {
    const char *who = "spd_model_plev_read";
    if (!name || !dst_device) return m_fail(SPD_E_ARG, std::string(who) + ": null argument");
    const int v = plev_id(name);
    if (v < 0) return m_fail(SPD_E_ARG, std::string(who) + ": unknown variable '" + name + "' (u_plev, v_plev, t_plev, q_plev, z_plev, mslp)");
    if (int rc = member_range(m, first, count, who)) return rc;
    const spd_model::Plev &pl = m->plev;
    if (pl.n == 0) return m_fail(SPD_E_ARG, std::string(who) + ": no target levels configured (spd_model_plev_configure)");
    if (!pl.have[v]) return m_fail(SPD_E_ARG, std::string(who) + ": '" + name + "' has not been computed at these levels (spd_model_plev_compute)");
    const size_t per = static_cast<size_t>(v == PLEV_MSLP ? 1 : pl.n) * NG, need = static_cast<size_t>(count) * per * sizeof(double);
    if (dst_bytes < need) return m_fail(SPD_E_SIZE, std::string(who) + ": destination too small (" + std::to_string(need) + " bytes needed)");
    if (count == 0) return SPD_OK;
    M_HIP(hipSetDevice(m->ctx->device));
    M_HIP(hipMemcpyAsync(dst_device, pl.out[v] + static_cast<size_t>(first) * per, need, hipMemcpyDeviceToDevice,
                         static_cast<hipStream_t>(stream)));
    return SPD_OK;
}

}  // extern "C"
