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

#include "global_mem.hpp"
#include "model_state.hpp"
#include "nudge.hpp"
#include "tables.hpp"

namespace spd {

namespace {
constexpr int kT = 256;
constexpr int kBlocks = (NSPEC + kT - 1) / kT;  // 4 blocks over the 992 coefficients; the last one is partial
constexpr int kLmax = TRUNC + 1;                // the largest total wavenumber that is nudged

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
    const double g = load_global(d.gain + l);
    double2v t = load_pair(d.target + s0 * d.slot_stride + 2 * k);
    if (s1 != s0) {
        const double2v t1 = load_pair(d.target + s1 * d.slot_stride + 2 * k);
        t.x = __dadd_rn(t.x, __dmul_rn(a, __dsub_rn(t1.x, t.x)));
        t.y = __dadd_rn(t.y, __dmul_rn(a, __dsub_rn(t1.y, t.y)));
    }
    double *x0 = d.state + i * d.member_stride + 2 * k, *x1 = x0 + d.level_stride;
    double2v u = load_pair(x0), v = load_pair(x1);
    u.x = __dadd_rn(u.x, __dmul_rn(g, __dsub_rn(t.x, u.x)));
    u.y = __dadd_rn(u.y, __dmul_rn(g, __dsub_rn(t.y, u.y)));
    v.x = __dadd_rn(v.x, __dmul_rn(g, __dsub_rn(t.x, v.x)));
    v.y = __dadd_rn(v.y, __dmul_rn(g, __dsub_rn(t.y, v.y)));
    store_pair(x0, u);
    store_pair(x1, v);
}
}  // namespace

hipError_t run_nudge(const NudgePlane *planes, int nplanes, const int *mask, int first, int count, int s0, int s1, double a,
                     hipStream_t s) {
    if (nplanes == 0 || count == 0) return hipSuccess;
    hipLaunchKernelGGL(nudge_kernel, dim3(kBlocks, nplanes, count), dim3(kT), 0, s, planes, mask, first, s0, s1, a);
    return hipGetLastError();
}

}  // namespace spd

// ---- host side: the target of a step, the configuration and the C ABI (spd_model_nudge_*); the step loop calls run_nudge itself ----

namespace {
constexpr int kNudgeNames = 5, kNudgeGains = 32, kNudgeRows = 8;  // gains: [n_names][8][32]; ps reads row 0 of its eight
const char *const kNudgeName[kNudgeNames] = {"vor", "div", "t", "tr", "ps"};
const char *const kNudgeOff = "no nudging configured (spd_model_nudge_configure)";
int nudge_name_id(const char *name) {
    for (int v = 0; name && v < kNudgeNames; ++v)
        if (std::strcmp(name, kNudgeName[v]) == 0) return v;
    return -1;
}
int nudge_levels(int id) { return id == 4 ? 1 : 8; }
}  // namespace

NudgeAt spd::nudge_at(const std::vector<int> &stamps, int n) {
    const int last = static_cast<int>(stamps.size()) - 1;
    if (n <= stamps[0]) return {0, 0, 0.0};
    if (n >= stamps[last]) return {last, last, 0.0};
    const int hi = static_cast<int>(std::upper_bound(stamps.begin(), stamps.end(), n) - stamps.begin()), lo = hi - 1;
    if (n == stamps[lo]) return {lo, lo, 0.0};
    return {lo, hi, static_cast<double>(static_cast<long long>(n) - stamps[lo]) / static_cast<double>(static_cast<long long>(stamps[hi]) - stamps[lo])};
}

extern "C" {

int spd_model_nudge_configure(spd_model_handle m, const char *const *names, int n_names, const double *gains, const int32_t *member_mask,
                              int capacity, int in_loop) {
    const char *who = "spd_model_nudge_configure";
    // (the arguments first, in the header's order: nothing below needs the device)
    if (n_names < 0 || n_names > kNudgeNames || (n_names > 0 && !names)) return m_fail(SPD_E_ARG, std::string(who) + ": bad list of names");
    std::vector<int> ids;
    for (int k = 0; k < n_names; ++k) {
        const int id = nudge_name_id(names[k]);
        if (id < 0)
            return m_fail(SPD_E_ARG, std::string(who) + ": unknown variable '" + (names[k] ? names[k] : "(null)") + "' (vor, div, t, tr, ps)");
        ids.push_back(id);
    }
    for (int k = 0; k < n_names; ++k)
        for (int j = 0; j < k; ++j)
            if (ids[j] == ids[k]) return m_fail(SPD_E_ARG, std::string(who) + ": '" + names[k] + "' named twice");
    if (n_names > 0) {
        if (!gains) return m_fail(SPD_E_ARG, std::string(who) + ": null gains");
        for (int k = 0; k < n_names; ++k)
            for (int lev = 0; lev < nudge_levels(ids[k]); ++lev)
                for (int l = 0; l < kNudgeGains; ++l) {
                    const double g = gains[(static_cast<size_t>(k) * kNudgeRows + lev) * kNudgeGains + l];
                    if (!std::isfinite(g) || g < 0.0 || g > 1.0)
                        return m_fail(SPD_E_ARG, std::string(who) + ": the gain of '" + names[k] + "' at level " + std::to_string(lev) +
                                                     ", wavenumber " + std::to_string(l) + " is not a finite number in [0, 1]");
                }
        if (capacity < 1) return m_fail(SPD_E_ARG, std::string(who) + ": capacity must be at least 1");
        if (in_loop != 0 && in_loop != 1) return m_fail(SPD_E_ARG, std::string(who) + ": in_loop must be 0 or 1");
    }
    if (int rc = configure_allowed(m, who)) return rc;
    for (int i = 0; n_names > 0 && member_mask && i < m->M; ++i)
        if (member_mask[i] != 0 && member_mask[i] != 1)
            return m_fail(SPD_E_ARG, std::string(who) + ": the mask entry of member " + std::to_string(i) + " is neither 0 nor 1");
    spd_model::Nudge &nd = m->nudge;
    if (int rc = retire(m, nd)) return rc;
    if (n_names == 0) return SPD_OK;  // off
    spd_model::Nudge next;
    next.capacity = capacity;
    next.in_loop = in_loop != 0;
    next.names = ids;
    // the planes some gain of which is not zero: [name in the caller's order][level]
    struct Row {
        int id, lev;
        const double *gain;
    };
    std::vector<Row> rows;
    size_t target_doubles = 0;
    for (int k = 0; k < n_names; ++k) {
        next.offset[ids[k]] = target_doubles;
        const size_t per_slot = static_cast<size_t>(nudge_levels(ids[k])) * NSPEC * C;
        if (static_cast<size_t>(capacity) > (static_cast<size_t>(-1) / 16) / per_slot)
            return m_fail(SPD_E_ARG, std::string(who) + ": the target slots' size does not fit size_t");
        target_doubles += static_cast<size_t>(capacity) * per_slot;
        for (int lev = 0; lev < nudge_levels(ids[k]); ++lev) {
            const double *g = gains + (static_cast<size_t>(k) * kNudgeRows + lev) * kNudgeGains;
            if (std::any_of(g, g + kNudgeGains, [](double x) { return x != 0.0; })) rows.push_back({ids[k], lev, g});
        }
    }
    // one allocation: target slots | gain rows | plane descriptors | member mask
    const size_t targets = sample_up(target_doubles * sizeof(double)), gain_bytes = sample_up(rows.size() * kNudgeGains * sizeof(double));
    const size_t desc = sample_up(rows.size() * sizeof(NudgePlane)), mask_bytes = member_mask ? sample_up(sizeof(int) * m->M) : 0;
    const size_t total = targets + gain_bytes + desc + mask_bytes;
    void *p = nullptr;
    if (hipMalloc(&p, total) != hipSuccess) {  // nudging is off; the model is as usable as before
        (void)hipGetLastError();
        return m_fail(SPD_E_DEVICE, std::string(who) + ": cannot allocate the target slots (" + std::to_string(total) + " bytes asked for: " +
                                        std::to_string(capacity) + " slots); nudging is off");
    }
    Carve carve{static_cast<char *>(p)};
    next.alloc = p;
    next.targets = carve.take<double>(targets);
    double *gain_dev = carve.take<double>(gain_bytes);
    next.planes = carve.take<NudgePlane>(desc);
    next.mask = member_mask ? carve.take<int>(mask_bytes) : nullptr;
    std::vector<NudgePlane> host_planes;
    std::vector<double> host_gains;
    double *const base[kNudgeNames] = {m->P.vor, m->P.div, m->P.t, m->P.tr, m->P.ps};
    for (const Row &r : rows) {
        const size_t levels = static_cast<size_t>(nudge_levels(r.id)), plane = static_cast<size_t>(r.lev) * NSPEC * C;
        NudgePlane d{};
        d.state = base[r.id] + plane;
        d.target = next.targets + next.offset[r.id] + plane;
        d.gain = gain_dev + host_gains.size();
        d.member_stride = static_cast<long>(2 * levels * NSPEC * C);
        d.level_stride = static_cast<long>(levels * NSPEC * C);
        d.slot_stride = static_cast<long>(levels * NSPEC * C);
        host_planes.push_back(d);
        host_gains.insert(host_gains.end(), r.gain, r.gain + kNudgeGains);
    }
    hipError_t e = hipMemset(next.targets, 0, targets);
    if (e == hipSuccess && !rows.empty()) e = hipMemcpy(gain_dev, host_gains.data(), host_gains.size() * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess && !rows.empty()) e = hipMemcpy(next.planes, host_planes.data(), host_planes.size() * sizeof(NudgePlane), hipMemcpyHostToDevice);
    if (e == hipSuccess && member_mask) e = hipMemcpy(next.mask, member_mask, sizeof(int) * m->M, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return upload_failed(who, e, p);
    next.nplanes = static_cast<int>(host_planes.size());
    next.on = true;
    nd = std::move(next);
    return SPD_OK;
}

int spd_model_nudge_set_times(spd_model_handle m, const int32_t *steps, int n) {
    const char *who = "spd_model_nudge_set_times";
    if (n < 0 || (n > 0 && !steps)) return m_fail(SPD_E_ARG, std::string(who) + ": bad list of steps");
    for (int k = 1; k < n; ++k)
        if (steps[k] <= steps[k - 1]) return m_fail(SPD_E_ARG, std::string(who) + ": the stamps must be strictly ascending (slot " + std::to_string(k) + ")");
    if (!m) return m_fail(SPD_E_ARG, std::string(who) + ": null model");
    spd_model::Nudge &nd = m->nudge;
    if (!nd.on) return m_fail(SPD_E_ARG, std::string(who) + ": " + kNudgeOff);
    if (m->steps_pending) return m_fail(SPD_E_ARG, std::string(who) + ": a checked multi-step call is in flight; end it first");
    if (n > nd.capacity)
        return m_fail(SPD_E_ARG, std::string(who) + ": " + std::to_string(n) + " stamps for " + std::to_string(nd.capacity) + " slots");
    nd.stamps.assign(steps, steps + n);  // (host state only: the steps already issued carry their slots and weight by value)
    nd.in_use = n;
    return SPD_OK;
}

int spd_model_nudge_set_target(spd_model_handle m, int slot, const char *name, const void *host, size_t bytes) {
    const char *who = "spd_model_nudge_set_target";
    if (!name || !host) return m_fail(SPD_E_ARG, std::string(who) + ": null argument");
    const int id = nudge_name_id(name);
    if (id < 0) return m_fail(SPD_E_ARG, std::string(who) + ": unknown variable '" + name + "' (vor, div, t, tr, ps)");
    if (!m) return m_fail(SPD_E_ARG, std::string(who) + ": null model");
    if (int rc = usable(m, who)) return rc;
    const spd_model::Nudge &nd = m->nudge;
    if (!nd.on) return m_fail(SPD_E_ARG, std::string(who) + ": " + kNudgeOff);
    if (std::find(nd.names.begin(), nd.names.end(), id) == nd.names.end())
        return m_fail(SPD_E_ARG, std::string(who) + ": '" + name + "' is not among the configured names");
    if (slot < 0 || slot >= nd.capacity)
        return m_fail(SPD_E_ARG, std::string(who) + ": slot " + std::to_string(slot) + " of " + std::to_string(nd.capacity));
    const size_t need = static_cast<size_t>(nudge_levels(id)) * NSPEC * C * sizeof(double);
    if (bytes != need) return m_fail(SPD_E_SIZE, std::string(who) + ": a slot of '" + name + "' needs exactly " + std::to_string(need) + " bytes");
    if (m->steps_pending) return m_fail(SPD_E_ARG, std::string(who) + ": a checked multi-step call is in flight; end it first");
    M_HIP(hipSetDevice(m->ctx->device));
    // a blocking copy on the null stream, which does not order against the streams the steps were issued on (as spd_model_set)
    M_HIP(hipDeviceSynchronize());
    M_HIP(hipMemcpy(nd.targets + nd.offset[id] + static_cast<size_t>(slot) * (need / sizeof(double)), host, need, hipMemcpyHostToDevice));
    return SPD_OK;
}

int spd_model_nudge_apply(spd_model_handle m, int first, int count, void *stream) {
    const char *who = "spd_model_nudge_apply";
    if (int rc = member_range(m, first, count, who)) return rc;
    spd_model::Nudge &nd = m->nudge;
    if (!nd.on) return m_fail(SPD_E_ARG, std::string(who) + ": " + kNudgeOff);
    if (!m->initialized) return m_fail(SPD_E_ARG, std::string(who) + ": model state not initialized");
    if (m->steps_pending) return m_fail(SPD_E_ARG, std::string(who) + ": a checked multi-step call is in flight; end it first");
    if (nd.in_use == 0) return m_fail(SPD_E_ARG, std::string(who) + ": no target slot is in use (spd_model_nudge_set_times)");
    M_HIP(hipSetDevice(m->ctx->device));
    if (int rc = settle_deferred_check(m)) return rc;  // (a range check that was put off looks at the state as it is NOW)
    if (nd.nplanes == 0 || count == 0) return SPD_OK;
    m->phi_ahead = false;  // the temperature changes under the look-ahead geopotential; phi itself is the next step's to recompute
    const NudgeAt at = nudge_at(nd.stamps, m->current_step);
    const hipError_t e = run_nudge(nd.planes, nd.nplanes, nd.mask, first, count, at.s0, at.s1, at.a, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return m_fail(SPD_E_DEVICE, std::string(who) + ": " + hipGetErrorString(e));
    }
    ++nd.applied;
    return SPD_OK;
}

int spd_model_nudge_info(spd_model_handle m, int *n_names, int *capacity, int *in_use, int *in_loop, long long *applied) {
    if (!m) return m_fail(SPD_E_ARG, "spd_model_nudge_info: null model");
    const spd_model::Nudge &nd = m->nudge;  // (a model without nudging: all zero)
    if (n_names) *n_names = static_cast<int>(nd.names.size());
    if (capacity) *capacity = nd.capacity;
    if (in_use) *in_use = nd.in_use;
    if (in_loop) *in_loop = nd.in_loop ? 1 : 0;
    if (applied) *applied = nd.applied;
    return SPD_OK;
}

}  // extern "C"
