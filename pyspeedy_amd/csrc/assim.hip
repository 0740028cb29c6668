// Assimilation: a serial ensemble square-root filter (Whitaker & Hamill 2002) over the masked members, with at most 64 scalar
// observations taken through projection-tape weight maps (spd_model_assim_*, include/pyspeedy_amd.h).
//
// An event is four kinds of launch on one stream.  (1) The observation-space ensemble: the projection tape's front end and
// projtape_kernel, unchanged, for the masked members, into a one-slot ring [M][E]; assim_gather_kernel picks the masked members'
// rows out of it as Y [E][r].  (2) assim_weights_kernel: one workgroup forms W [r][r] in the LDS by the serial square-root update,
// entry after entry (assim_weights.hpp, which spd_assim_weights_host compiles for the host), and leaves W [64][64], zero beyond r,
// and the ring slot in device memory.  (3) assim_transform_kernel: X'_(a_j) = sum_i W_ij X_(a_i) on both time levels of the 33
// planes for the coefficients with m + n <= 31, the sum in ascending i from its first term, every operation rounded on its own
// (no contraction, the __d*_rn intrinsics), so that the numpy restatement gives the same bits.  A workgroup owns 64 coefficients
// of one plane and time level for all r members: its four waves load every member once into the LDS, and behind one barrier each
// wave forms its share of the output members, eight at a time, and stores them, so no workgroup reads what another writes.  W is
// uniform: scalar loads.  A coefficient with m + n >= 32 and a member outside the mask are neither loaded nor stored.
#include <hip/hip_runtime.h>

#include "assim.hpp"
#include "assim_weights.hpp"
#include "global_mem.hpp"
#include "model_state.hpp"
#include "tables.hpp"

namespace spd {

namespace {
constexpr int kT = 256;
constexpr int kW = 64;    // coefficients of a transform workgroup: a lane per coefficient in each of its waves
constexpr int kXT = 256;  // lanes of a transform workgroup: four waves on the same 64 coefficients
constexpr int kChunks = (NSPEC + kW - 1) / kW;
constexpr int kLmax = TRUNC + 1;  // the largest total wavenumber that takes part
constexpr int kLD = kAssimMax;    // the leading dimension of W in device memory
constexpr int kLDS = kAssimMax + 1;  // ... and in the LDS: a lane per row reads W[k][i] for 64 k at once without a bank conflict

// The observations of one event, by value: yo[e] (NaN: missing) and the error variances.
struct AssimObs {
    double yo[kAssimMax], var[kAssimMax];
};

// Y[e][i] = yraw[a_i][e]: the masked members' rows of the one-slot projection ring, entry-major
__global__ __launch_bounds__(kT) void assim_gather_kernel(const double *__restrict__ yraw, const int *__restrict__ members, int E, int r,
                                                          double *__restrict__ Y) {
    for (int x = threadIdx.x; x < E * r; x += kT) {
        const int e = x / r, i = x - e * r;
        Y[x] = yraw[static_cast<long>(members[i]) * E + e];
    }
}

// One workgroup.  W lives in the LDS while the entries are taken one after the other; W_out [64][64] (zero beyond r) and the
// ring slot [E][4] are left in device memory.
__global__ __launch_bounds__(kT) void assim_weights_kernel(const double *__restrict__ Y, int E, int r, AssimObs obs, double rho,
                                                           double *__restrict__ W_out, double *__restrict__ ring_slot) {
    __shared__ double w[kAssimMax * kLDS], vec[4 * kAssimMax], yo[kAssimMax], var[kAssimMax];
    if (r < 2 || r > kAssimMax || E < 1 || E > kAssimMax) return;
    for (int e = threadIdx.x; e < E; e += kT) yo[e] = obs.yo[e], var[e] = obs.var[e];
    __syncthreads();
    assim_weights(Y, r, E, r, yo, var, rho, w, kLDS, vec, ring_slot, static_cast<int>(threadIdx.x), kT, [] { __syncthreads(); });
    for (int x = threadIdx.x; x < kLD * kLD; x += kT) {
        const int i = x / kLD, j = x - i * kLD;
        W_out[x] = i < r && j < r ? w[i * kLDS + j] : 0.0;
    }
}

// blockIdx.x: 64 coefficients, blockIdx.y: 2 * plane + time level.  Dynamic LDS: r rows of 64 x 16 bytes.  The four waves of a
// workgroup share the rows: wave w loads the members w, w + 4, ... and, behind the barrier, forms the output members of the blocks
// of eight 8 w, 8 w + 32, ...  (The rows set the LDS and so the workgroups per CU; four waves on them use all four SIMDs.)
__global__ __launch_bounds__(kXT) void assim_transform_kernel(const AssimPlane *__restrict__ planes, const int *__restrict__ members, int r,
                                                             const double *__restrict__ W) {
#pragma clang fp contract(off)
    constexpr int kJ = 8;
    extern __shared__ double2v xs[];  // [r][kW]
    const int lane = threadIdx.x & (kW - 1), wave = threadIdx.x / kW;
    const int k = blockIdx.x * kW + lane;
    if (r < 1 || r > kLD) return;
    const int n = k / MX, l = k - n * MX + n;
    const bool inside = k < NSPEC && l <= kLmax;
    const AssimPlane d = planes[blockIdx.y >> 1];
    double *base = d.state + (blockIdx.y & 1) * d.level_stride + 2 * k;
    if (inside)
        for (int i = wave; i < r; i += kXT / kW) xs[i * kW + lane] = load_pair(base + members[i] * d.member_stride);
    __syncthreads();
    if (!inside) return;
    for (int j0 = kJ * wave; j0 < r; j0 += kJ * (kXT / kW)) {  // (a column at or beyond r is formed from zeros of W and stored nowhere)
        double2v acc[kJ];
        const double2v x0 = xs[lane];
#pragma unroll
        for (int b = 0; b < kJ; ++b) acc[b].x = __dmul_rn(W[j0 + b], x0.x), acc[b].y = __dmul_rn(W[j0 + b], x0.y);
        for (int i = 1; i < r; ++i) {
            const double2v xi = xs[i * kW + lane];
#pragma unroll
            for (int b = 0; b < kJ; ++b) {
                const double wij = W[i * kLD + j0 + b];
                acc[b].x = __dadd_rn(acc[b].x, __dmul_rn(wij, xi.x)), acc[b].y = __dadd_rn(acc[b].y, __dmul_rn(wij, xi.y));
            }
        }
#pragma unroll
        for (int b = 0; b < kJ; ++b)
            if (j0 + b < r) store_pair(base + members[j0 + b] * d.member_stride, acc[b]);
    }
}
}  // namespace

static hipError_t run_assim_transform(const AssimPlane *planes, const int *members, int r, const double *W, hipStream_t s) {
    hipLaunchKernelGGL(assim_transform_kernel, dim3(kChunks, 2 * kAssimPlanes), dim3(kXT), static_cast<size_t>(r) * kW * sizeof(double2v), s, planes,
                       members, r, W);
    return hipGetLastError();
}

}  // namespace spd

// ---- host side: the step loop's event, the configuration and the C ABI (spd_model_assim_*, spd_assim_*) ----

namespace {
constexpr int kAssimMaxPatterns = 64;
const char *const kAssimOff = "no assimilation configured (spd_model_assim_configure)";
const char *const kAssimInvalid = "the assimilation ring is invalid until spd_model_assim_reset";

// the 33 planes of the spectral state, as breeding lists them
std::vector<AssimPlane> assim_planes(const spd_model *m) {
    std::vector<AssimPlane> planes;
    double *const base[5] = {m->P.vor, m->P.div, m->P.t, m->P.tr, m->P.ps};
    for (int v = 0; v < 5; ++v) {
        const size_t levels = v == 4 ? 1 : 8;
        for (size_t k = 0; k < levels; ++k)
            planes.push_back({base[v] + k * NSPEC * C, static_cast<long>(2 * levels * NSPEC * C), static_cast<long>(levels * NSPEC * C)});
    }
    return planes;
}

// the observation-space ensemble of the state as it stands: front end and projection kernel for the masked members, then Y [E][r]
hipError_t assim_observe(spd_model *m, double *Y, hipStream_t s) {
    const spd_model::Assim &as = m->assim;
    const int E = static_cast<int>(as.entries.size());
    hipError_t e = hipSuccess;
    for (const auto &range : as.set.ranges) {
        if (e == hipSuccess) e = sample_front(m, as, range.first, range.second, s);
        if (e == hipSuccess)
            e = run_projtape_sample(as.planes, as.nplanes, as.items, as.weights, as.slab, as.slab_fields, as.yraw, E, range.first, range.second,
                                    m->stored32 ? 1 : 0, s);
    }
    if (e == hipSuccess) {
        hipLaunchKernelGGL(assim_gather_kernel, dim3(1), dim3(kT), 0, s, as.yraw, as.member_list, E, as.r, Y);
        e = hipGetLastError();
    }
    return e;
}

// the checks of an observation table of E entries per row
int assim_check_observations(const char *who, const int32_t *steps, int n_rows, const double *yo, const double *var, int n_entries) {
    if (n_rows < 0) return m_fail(SPD_E_ARG, std::string(who) + ": n_rows must not be negative");
    if (n_entries < 1 || n_entries > kAssimMax)
        return m_fail(SPD_E_ARG, std::string(who) + ": n_entries must be 1 ... " + std::to_string(kAssimMax) + ", got " + std::to_string(n_entries));
    if (n_rows > 0 && (!steps || !yo || !var)) return m_fail(SPD_E_ARG, std::string(who) + ": null argument");
    for (int t = 1; t < n_rows; ++t)
        if (steps[t] <= steps[t - 1])
            return m_fail(SPD_E_ARG, std::string(who) + ": the step stamps must be strictly ascending (row " + std::to_string(t) + ": " +
                                         std::to_string(steps[t]) + " after " + std::to_string(steps[t - 1]) + ")");
    for (int t = 0; t < n_rows; ++t)
        for (int e = 0; e < n_entries; ++e) {
            const double v = var[static_cast<size_t>(t) * n_entries + e], y = yo[static_cast<size_t>(t) * n_entries + e];
            if (!std::isfinite(v) || !(v > 0.0))
                return m_fail(SPD_E_ARG, std::string(who) + ": the error variance of row " + std::to_string(t) + ", entry " + std::to_string(e) +
                                             " is not a finite number > 0");
            if (std::isinf(y))
                return m_fail(SPD_E_ARG, std::string(who) + ": the observation of row " + std::to_string(t) + ", entry " + std::to_string(e) +
                                             " is infinite (NaN marks a missing one)");
        }
    return SPD_OK;
}
}  // namespace

int spd::assim_event(spd_model *m, hipStream_t s, const char *who, bool in_loop) {
    spd_model::Assim &as = m->assim;
    const auto at = std::lower_bound(as.obs_steps.begin(), as.obs_steps.end(), m->current_step);
    if (at == as.obs_steps.end() || *at != m->current_step) {
        if (!in_loop) return m_fail(SPD_E_ARG, std::string(who) + ": no row of observations is stamped with the current step (" +
                                                   std::to_string(m->current_step) + ")");
        ++as.skipped;
        return SPD_OK;
    }
    if (int rc = settle_deferred_check(m)) return rc;
    m->surf_cache_valid = m->phi_ahead = false;
    const size_t E = as.entries.size(), row = static_cast<size_t>(at - as.obs_steps.begin());
    AssimObs obs{};
    std::copy(as.obs_yo.begin() + row * E, as.obs_yo.begin() + (row + 1) * E, obs.yo);
    std::copy(as.obs_var.begin() + row * E, as.obs_var.begin() + (row + 1) * E, obs.var);
    double *slot = as.data + static_cast<size_t>(as.ring.slot(as.ring.taken + 1)) * E * 4;
    hipError_t e = assim_observe(m, as.Y, s);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(assim_weights_kernel, dim3(1), dim3(kT), 0, s, as.Y, static_cast<int>(E), as.r, obs, as.inflation, as.W, slot);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = run_assim_transform(as.xplanes, as.member_list, as.r, as.W, s);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return m_fail(SPD_E_DEVICE, std::string(who) + ": assimilation: " + hipGetErrorString(e));
    }
    ++as.ring.taken;
    as.ring.stamp(as.ring.taken, m->current_step, m->cal);
    ++as.applied;
    return SPD_OK;
}

extern "C" {

int spd_assim_check(const double *weights, int n_patterns, const char *const *names, const int *levels, const int *patterns, int n_entries,
                    const int32_t *mask, int members, int every, int capacity, double inflation, int in_loop) {
    const char *who = "spd_model_assim_configure";
    if (every < 1) return m_fail(SPD_E_ARG, std::string(who) + ": every must be at least 1");
    if (capacity < 1) return m_fail(SPD_E_ARG, std::string(who) + ": capacity must be at least 1");
    if (!std::isfinite(inflation) || !(inflation >= 1.0)) return m_fail(SPD_E_ARG, std::string(who) + ": inflation must be a finite number >= 1");
    if (in_loop != 0 && in_loop != 1) return m_fail(SPD_E_ARG, std::string(who) + ": in_loop must be 0 or 1");
    if (n_patterns < 1 || n_patterns > kAssimMaxPatterns)
        return m_fail(SPD_E_ARG, std::string(who) + ": n_patterns must be 1 ... " + std::to_string(kAssimMaxPatterns) + ", got " +
                                     std::to_string(n_patterns));
    if (n_entries < 1 || n_entries > kAssimMax)
        return m_fail(SPD_E_ARG, std::string(who) + ": n_entries must be 1 ... " + std::to_string(kAssimMax) + ", got " + std::to_string(n_entries));
    if (!weights) return m_fail(SPD_E_ARG, std::string(who) + ": null weights");
    if (!names || !levels || !patterns) return m_fail(SPD_E_ARG, std::string(who) + ": bad list of entries");
    if (int rc = check_weight_maps(who, weights, n_patterns)) return rc;
    for (int k = 0; k < n_entries; ++k) {
        const int id = entry_id(who, names[k], "u_grid, v_grid, t_grid, q_grid, phi_grid, ps_grid, u_plev, v_plev, t_plev, q_plev, z_plev, mslp)" SPD_DERIVED_TAIL);
        if (id < 0) return SPD_E_ARG;
        if (cat_kind(id) == CAT_PRECIP)
            return m_fail(SPD_E_ARG, std::string(who) + ": '" + names[k] + "' (entry " + std::to_string(k) +
                                         ") cannot be assimilated: precnv and precls are outputs of the column physics, not functions of the state");
        if (int rc = check_entry_level(who, k, names[k], id, levels[k])) return rc;
        if (int rc = check_entry_pattern(who, k, names[k], patterns[k], n_patterns)) return rc;
    }
    // (the member mask needs the member count: checked once the model is known)
    return mask ? check_member_mask(who, mask, members, kAssimMax, "an analysis takes") : SPD_OK;
}

int spd_model_assim_configure(spd_model_handle m, const double *weights, int n_patterns, const char *const *names, const int *levels,
                              const int *patterns, int n_entries, const int32_t *mask, int every, int capacity, double inflation, int in_loop) {
    const char *who = "spd_model_assim_configure";
    // (the arguments first, in the header's order: nothing in the first block needs the device or a model)
    if (int rc = spd_assim_check(weights, n_patterns, names, levels, patterns, n_entries, nullptr, 0, every, capacity, inflation, in_loop)) return rc;
    if (!mask) return m_fail(SPD_E_ARG, std::string(who) + ": null member mask");
    if (int rc = configure_allowed(m, who)) return rc;
    if (int rc = spd_assim_check(weights, n_patterns, names, levels, patterns, n_entries, mask, m->M, every, capacity, inflation, in_loop)) return rc;
    std::vector<PatternEntry> entries;
    for (int k = 0; k < n_entries; ++k) entries.push_back({stats_id(names[k]), levels[k], patterns[k]});
    if (int rc = check_plev_entries(m, who, names, entries)) return rc;
    if (in_loop && m->breed.on && m->breed.in_loop)
        return m_fail(SPD_E_ARG, std::string(who) + ": in-loop assimilation cannot be configured while in-loop breeding (spd_model_breed_configure) is: "
                                                    "both cut the call at their own steps; switch one of them off or to in_loop = 0");
    spd_model::Assim &as = m->assim;
    if (int rc = retire(m, as)) return rc;
    spd_model::Assim next;
    next.in_loop = in_loop != 0;
    next.every = every;
    next.inflation = inflation;
    next.npatterns = n_patterns;
    next.set = member_set(mask, m->M);
    next.r = static_cast<int>(next.set.members.size());
    const size_t M = static_cast<size_t>(m->M), slots = static_cast<size_t>(capacity), E = static_cast<size_t>(n_entries);
    // the sample plan and the projection kernel's lists, as the projection tape builds them
    const EntryPlanes table = entry_planes(entries);
    SamplePlan plan;
    plan_sample(m, table.ids, next, plan);
    const std::vector<AssimPlane> xplanes = assim_planes(m);
    // one allocation: ring | patterns | slab | tables[2] | plane descriptors | entry list | yraw | Y | W | member list | transform planes
    const size_t per_slot = E * 4 * sizeof(double);
    if (slots > (static_cast<size_t>(-1) / 2) / per_slot) return m_fail(SPD_E_ARG, std::string(who) + ": the ring's size does not fit size_t");
    const size_t ring = sample_up(slots * per_slot), maps = sample_up(static_cast<size_t>(n_patterns) * NG * sizeof(double));
    const size_t desc = sample_up(table.distinct.size() * sizeof(ProjTapePlane)), list = sample_up(E * sizeof(ProjTapeItem));
    const size_t yraw = sample_up(M * E * sizeof(double)), ybytes = sample_up(E * kAssimMax * sizeof(double));
    const size_t wbytes = sample_up(kAssimMax * kAssimMax * sizeof(double)), mbytes = sample_up(kAssimMax * sizeof(int));
    const size_t xbytes = sample_up(xplanes.size() * sizeof(AssimPlane));
    const size_t total = ring + maps + plan.slab_bytes + 2 * plan.table_bytes + desc + list + yraw + ybytes + wbytes + mbytes + xbytes;
    void *p = nullptr;
    if (hipMalloc(&p, total) != hipSuccess) {  // assimilation is off; the model is as usable as before
        (void)hipGetLastError();
        return m_fail(SPD_E_DEVICE, std::string(who) + ": cannot allocate the assimilation (" + std::to_string(total) + " bytes asked for); it is off");
    }
    Carve carve{static_cast<char *>(p)};
    next.alloc = p;
    next.data = carve.take<double>(ring);
    next.weights = carve.take<double>(maps);
    carve_front(carve, plan, next);
    next.planes = carve.take<ProjTapePlane>(desc);
    next.items = carve.take<ProjTapeItem>(list);
    next.yraw = carve.take<double>(yraw);
    next.Y = carve.take<double>(ybytes);
    next.W = carve.take<double>(wbytes);
    next.member_list = carve.take<int>(mbytes);
    next.xplanes = carve.take<AssimPlane>(xbytes);
    hipError_t e = hipMemset(p, 0, total);
    std::vector<SampleSource> sources;  // (per plane of plan.vars, in their order)
    if (e == hipSuccess) e = build_sample_front(m, plan, next, sources);
    std::vector<ProjTapePlane> host_planes;
    std::vector<ProjTapeItem> host_items;
    for (size_t q = 0; q < table.distinct.size(); ++q) {
        ProjTapePlane d{};  // (precnv / precls are refused: every plane comes from the slab)
        d.source = plane_source(plan, sources, table.distinct[q].first, table.distinct[q].second);
        d.first = static_cast<int>(host_items.size());
        table.each_entry_of(q, [&](int k) { host_items.push_back({entries[k].pattern, k}); });
        d.count = static_cast<int>(host_items.size()) - d.first;
        host_planes.push_back(d);
    }
    if (e == hipSuccess) e = hipMemcpy(next.weights, weights, static_cast<size_t>(n_patterns) * NG * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(next.planes, host_planes.data(), host_planes.size() * sizeof(ProjTapePlane), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(next.items, host_items.data(), host_items.size() * sizeof(ProjTapeItem), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(next.member_list, next.set.members.data(), next.set.members.size() * sizeof(int), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(next.xplanes, xplanes.data(), xplanes.size() * sizeof(AssimPlane), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return upload_failed(who, e, p);
    next.nplanes = static_cast<int>(host_planes.size());
    next.entries = std::move(entries);
    next.ring = SampleRing(capacity, 6);
    next.on = true;
    as = std::move(next);
    return SPD_OK;
}

int spd_model_assim_off(spd_model_handle m) {
    const char *who = "spd_model_assim_off";
    if (int rc = configure_allowed(m, who)) return rc;
    return retire(m, m->assim);
}

int spd_model_assim_set_observations(spd_model_handle m, const int32_t *steps, int n_rows, const double *yo, const double *var, int n_entries) {
    const char *who = "spd_model_assim_set_observations";
    if (int rc = assim_check_observations(who, steps, n_rows, yo, var, n_entries)) return rc;
    if (int rc = configure_allowed(m, who)) return rc;
    spd_model::Assim &as = m->assim;
    if (!as.on) return m_fail(SPD_E_ARG, std::string(who) + ": " + kAssimOff);
    if (static_cast<size_t>(n_entries) != as.entries.size())
        return m_fail(SPD_E_ARG, std::string(who) + ": n_entries is " + std::to_string(n_entries) + ", the configuration has " +
                                     std::to_string(as.entries.size()) + " entries");
    const size_t n = static_cast<size_t>(n_rows) * n_entries;
    as.obs_steps.assign(steps, steps + n_rows);
    as.obs_yo.assign(yo, yo + n);
    as.obs_var.assign(var, var + n);
    return SPD_OK;
}

int spd_model_assim_apply(spd_model_handle m, void *stream) {
    const char *who = "spd_model_assim_apply";
    if (!m) return m_fail(SPD_E_ARG, std::string(who) + ": null model");
    if (int rc = state_call_allowed(m, who, m->assim.on, kAssimOff)) return rc;
    M_HIP(hipSetDevice(m->ctx->device));
    return assim_event(m, static_cast<hipStream_t>(stream), who, false);
}

int spd_model_assim_compute(spd_model_handle m, void *dst_device, size_t dst_bytes, void *stream) {
    const char *who = "spd_model_assim_compute";
    if (!m) return m_fail(SPD_E_ARG, std::string(who) + ": null model");
    if (int rc = state_call_allowed(m, who, m->assim.on, kAssimOff)) return rc;
    const spd_model::Assim &as = m->assim;
    const size_t need = as.entries.size() * as.r * sizeof(double);
    if (int rc = destination_fits(who, dst_device, dst_bytes, need, sizeof(double))) return rc;
    M_HIP(hipSetDevice(m->ctx->device));
    const hipError_t e = assim_observe(m, static_cast<double *>(dst_device), static_cast<hipStream_t>(stream));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return m_fail(SPD_E_DEVICE, std::string(who) + ": " + hipGetErrorString(e));
    }
    return SPD_OK;
}

int spd_model_assim_transform(spd_model_handle m, const int32_t *members, int r, const double *w, void *stream) {
    const char *who = "spd_model_assim_transform";
    if (r < 1 || r > kAssimMax) return m_fail(SPD_E_ARG, std::string(who) + ": r must be 1 ... " + std::to_string(kAssimMax) + ", got " + std::to_string(r));
    if (!members || !w) return m_fail(SPD_E_ARG, std::string(who) + ": null argument");
    for (int i = 0; i < r; ++i)
        for (int j = 0; j < r; ++j)
            if (!std::isfinite(w[i * r + j]))
                return m_fail(SPD_E_ARG, std::string(who) + ": W[" + std::to_string(i) + "][" + std::to_string(j) + "] is not finite");
    for (int i = 0; i < r; ++i)
        for (int j = 0; j < i; ++j)
            if (members[i] == members[j]) return m_fail(SPD_E_ARG, std::string(who) + ": member " + std::to_string(members[i]) + " is named twice");
    if (!m) return m_fail(SPD_E_ARG, std::string(who) + ": null model");
    if (int rc = state_call_allowed(m, who, true, kAssimOff)) return rc;
    for (int i = 0; i < r; ++i)
        if (members[i] < 0 || members[i] >= m->M)
            return m_fail(SPD_E_ARG, std::string(who) + ": member " + std::to_string(members[i]) + " is out of range (0 ... " + std::to_string(m->M - 1) + ")");
    M_HIP(hipSetDevice(m->ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    spd_model::AssimTransform &xf = m->assim_xf;
    if (!xf.alloc) {
        const std::vector<AssimPlane> xplanes = assim_planes(m);
        const size_t xbytes = sample_up(xplanes.size() * sizeof(AssimPlane)), mbytes = sample_up(kAssimMax * sizeof(int));
        const size_t wbytes = sample_up(kAssimMax * kAssimMax * sizeof(double));
        void *p = nullptr;
        if (hipMalloc(&p, xbytes + mbytes + wbytes) != hipSuccess) {
            (void)hipGetLastError();
            return m_fail(SPD_E_DEVICE, std::string(who) + ": cannot allocate the transform's tables");
        }
        Carve carve{static_cast<char *>(p)};
        spd_model::AssimTransform next;
        next.alloc = p;
        next.xplanes = carve.take<AssimPlane>(xbytes);
        next.member_list = carve.take<int>(mbytes);
        next.W = carve.take<double>(wbytes);
        const hipError_t e = hipMemcpy(next.xplanes, xplanes.data(), xplanes.size() * sizeof(AssimPlane), hipMemcpyHostToDevice);
        if (e != hipSuccess) return upload_failed(who, e, p);
        xf = next;
    }
    if (int rc = settle_deferred_check(m)) return rc;
    m->surf_cache_valid = m->phi_ahead = false;
    std::vector<double> padded(kAssimMax * kAssimMax, 0.0);
    std::vector<int> list(kAssimMax, 0);
    for (int i = 0; i < r; ++i) {
        list[i] = members[i];
        for (int j = 0; j < r; ++j) padded[i * kAssimMax + j] = w[i * r + j];
    }
    // (behind whatever still reads the tables of an earlier call on this stream; the host waits until its own copies are taken)
    M_HIP(hipMemcpyAsync(xf.W, padded.data(), padded.size() * sizeof(double), hipMemcpyHostToDevice, s));
    M_HIP(hipMemcpyAsync(xf.member_list, list.data(), list.size() * sizeof(int), hipMemcpyHostToDevice, s));
    M_HIP(hipStreamSynchronize(s));
    const hipError_t e = run_assim_transform(xf.xplanes, xf.member_list, r, xf.W, s);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return m_fail(SPD_E_DEVICE, std::string(who) + ": " + hipGetErrorString(e));
    }
    return SPD_OK;
}

int spd_model_assim_read(spd_model_handle m, int t0, int nt, void *dst_device, size_t dst_bytes, void *stream) {
    const char *who = "spd_model_assim_read";
    if (!m) return m_fail(SPD_E_ARG, std::string(who) + ": null model");
    const spd_model::Assim &as = m->assim;
    if (int rc = read_allowed(m, who, as.on, kAssimOff, as.validity, kAssimInvalid)) return rc;
    if (int rc = held_range(who, as.ring, t0, nt, "event")) return rc;
    const size_t per = as.entries.size() * 4, need = static_cast<size_t>(nt) * per * sizeof(double);
    if (int rc = destination_fits(who, dst_device, dst_bytes, need, sizeof(double))) return rc;
    // (one block per slot: the E x 4 values)
    return gather_slots(m, who, as.data, per, per, 1, t0, nt, as.ring, dst_device, stream);
}

int spd_model_assim_weights(spd_model_handle m, void *w_device, size_t w_bytes, void *y_device, size_t y_bytes, void *stream) {
    const char *who = "spd_model_assim_weights";
    if (!m) return m_fail(SPD_E_ARG, std::string(who) + ": null model");
    const spd_model::Assim &as = m->assim;
    if (int rc = read_allowed(m, who, as.on, kAssimOff, as.validity, kAssimInvalid)) return rc;
    if (as.applied == 0) return m_fail(SPD_E_ARG, std::string(who) + ": no event has been executed since spd_model_assim_configure");
    const size_t wneed = static_cast<size_t>(kAssimMax) * kAssimMax * sizeof(double), yneed = as.entries.size() * as.r * sizeof(double);
    if (int rc = destination_fits(who, w_device, w_bytes, wneed, sizeof(double))) return rc;
    if (int rc = destination_fits(who, y_device, y_bytes, yneed, sizeof(double))) return rc;
    M_HIP(hipSetDevice(m->ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    M_HIP(hipMemcpyAsync(w_device, as.W, wneed, hipMemcpyDeviceToDevice, s));
    M_HIP(hipMemcpyAsync(y_device, as.Y, yneed, hipMemcpyDeviceToDevice, s));
    return SPD_OK;
}

int spd_model_assim_rows(spd_model_handle m, int32_t *rows, int max_rows) {
    return ring_rows(m, "spd_model_assim_rows", &spd_model::assim, kAssimOff, rows, max_rows);
}

int spd_model_assim_reset(spd_model_handle m) {
    if (int rc = ring_reset(m, "spd_model_assim_reset", &spd_model::assim, kAssimOff)) return rc;
    m->assim.skipped = 0;
    return SPD_OK;
}

int spd_model_assim_info(spd_model_handle m, int *r, int *n_entries, int *every, int *capacity, long long *taken, long long *skipped, int *in_loop,
                         long long *applied) {
    if (!m) return m_fail(SPD_E_ARG, "spd_model_assim_info: null model");
    const spd_model::Assim &as = m->assim;  // (a model without assimilation: all zero)
    if (r) *r = as.r;
    if (n_entries) *n_entries = static_cast<int>(as.entries.size());
    if (every) *every = as.every;
    if (capacity) *capacity = as.ring.capacity;
    if (taken) *taken = as.ring.taken;
    if (skipped) *skipped = as.skipped;
    if (in_loop) *in_loop = as.in_loop ? 1 : 0;
    if (applied) *applied = as.applied;
    return SPD_OK;
}

int spd_assim_weights_host(const double *y, int n_entries, int r, const double *yo, const double *var, double inflation, double *w_out,
                           double *stats_out) {
    const char *who = "spd_assim_weights_host";
    if (!y || !yo || !var || !w_out || !stats_out) return m_fail(SPD_E_ARG, std::string(who) + ": null argument");
    if (r < 2 || r > kAssimMax) return m_fail(SPD_E_ARG, std::string(who) + ": r must be 2 ... " + std::to_string(kAssimMax) + ", got " + std::to_string(r));
    if (n_entries < 1 || n_entries > kAssimMax)
        return m_fail(SPD_E_ARG, std::string(who) + ": n_entries must be 1 ... " + std::to_string(kAssimMax) + ", got " + std::to_string(n_entries));
    std::vector<double> vec(4 * kAssimMax, 0.0);
    spd::assim_weights(y, r, n_entries, r, yo, var, inflation, w_out, r, vec.data(), stats_out, 0, 1, [] {});
    return SPD_OK;
}

}  // extern "C"
