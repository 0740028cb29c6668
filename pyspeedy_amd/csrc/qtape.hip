// The quantile tape: minimum, maximum, quantiles and exceedance probabilities over a masked ensemble at every grid point, formed on
// the GPU at a join of the member groups and kept as planes in a ring (spd_model_qtape_*, include/pyspeedy_amd.h; the arithmetic is
// qtape_point.hpp, the definition DESIGN section 4o).
//
// An event is the sample front end for the member ranges that cover the mask, then one launch on the same stream:
// qtape_point_kernel, one workgroup of one wavefront per 64 points of a distinct plane, a lane per point.  The lane gathers the r
// members' values -- what an fp64 tape of that name holds: export_unit on the slab's value, or on precnv / precls read where the
// column kernel stores them, widened -- eight loads in flight at a time, into a column of its own in the LDS, [64][64] doubles =
// 32 KiB: the layout of verif_point_kernel (verif.hip) at a quarter of its width, whose gather also loads a truth member and is
// therefore not shared.  A wavefront's access to member j is 512 contiguous bytes without a bank conflict, and no lane touches
// another's column (no barrier).  The sort below moves 64 KiB per lane through the LDS: with verif_point_kernel's 256 lanes and
// 128 KiB per workgroup, 18 workgroups per plane put four wavefronts behind one CU's LDS and leave most CUs idle; 72 workgroups of
// one wavefront per plane spread over the CUs, each with an LDS to itself (measured, the two shapes alternated in one session at
// 64 members: 0.226 against 0.240 ms per event, profiles/qtape_perf.txt).
//
// The column is then put into its stable ascending order IN PLACE (qtape_sort: an odd-even transposition with strict swaps,
// r phases of r / 2 neighbour pairs, both values of a pair written back whether exchanged or not, so the control flow is uniform
// over the wavefront and independent of the data).  A selection by rank would leave the column alone, but every entry of the plane
// would then have to find its two ranks again among the r members or keep them in registers indexed at run time.  With the column
// in order an entry is two LDS reads at wavefront-uniform indices, however many entries share the plane, and a probability is one
// pass of r compares.  (A rank pass that scatters into a second column, which 64 lanes would leave room for, halves the LDS traffic;
// it is not built: DESIGN section 4o.)  Each entry's value goes straight into its plane of the ring slot, coalesced.  No barrier,
// no atomic, no scratch memory; nothing here writes into the model.
#include <hip/hip_runtime.h>

#include "global_mem.hpp"
#include "model_state.hpp"
#include "qtape.hpp"
#include "spectra.hpp"
#include "tables.hpp"

namespace spd {

namespace {
constexpr int kT = kQtapeLanes;
constexpr int kTiles = NG / kT;  // workgroups per plane
constexpr int kLoads = 8;        // members whose loads are in flight together
static_assert(NG == kQtapePoints && NG % kT == 0, "a plane is a whole number of tiles");
static_assert(kQtapeMax * kT * sizeof(double) <= 160 * 1024, "the members' columns fit the LDS of a CU");

// a lane's column of the LDS: member j of its point
struct QtapeColumn {
    double *at;
    __device__ __forceinline__ double get(int j) const { return at[j * kT]; }
    __device__ __forceinline__ void set(int j, double v) const { at[j * kT] = v; }
};

// The r members of one point into the lane's column: `plane` is the point in member 0's plane as it is stored (precnv / precls:
// float while the model stores them so), `stride` the elements between two members.  kLoads members' loads are issued together,
// then widened, converted and stored; the decision where the plane lies is taken once, outside (with_sample_plane).
struct QtapeGather {
    template <class T>
    __device__ __forceinline__ int operator()(const T *plane, long stride, const int *const &members, const int &r, const int &unit, const long &p,
                                              double *const &column) const {
        const T *at = plane + p;
        for (int j0 = 0; j0 < r; j0 += kLoads) {
            T raw[kLoads];
#pragma unroll
            for (int b = 0; b < kLoads; ++b) raw[b] = load_global(at + members[j0 + b < r ? j0 + b : r - 1] * stride);
#pragma unroll
            for (int b = 0; b < kLoads; ++b)
                if (j0 + b < r) column[(j0 + b) * kT] = export_unit(static_cast<double>(raw[b]), unit);
        }
        return 0;
    }
};

// blockIdx.x: 64 points, blockIdx.y: distinct plane.  out: [E][4608] of one ring slot (or the caller's buffer of _compute).
__global__ __launch_bounds__(kT) void qtape_point_kernel(const QtapePlane *__restrict__ planes, const QtapeItem *__restrict__ items,
                                                         const int *__restrict__ members, int r, const double *__restrict__ slab, int slab_fields,
                                                         int store32, double *__restrict__ out) {
#pragma clang fp contract(off)
    __shared__ double col[kQtapeMax * kT];
    if (r < 2 || r > kQtapeMax) return;
    const QtapePlane d = planes[blockIdx.y];
    const int t = threadIdx.x;
    const long p = static_cast<long>(blockIdx.x) * kT + t;
    double *const column = col + t;
    const int *const list = members;
    with_sample_plane(d.src, slab, slab_fields, store32 != 0, 0L, QtapeGather{}, list, r, d.src.unit, p, column);
    const QtapeColumn x{column};
    qtape_sort(x, r);
    for (int i = 0; i < d.count; ++i) {
        const QtapeItem it = items[d.first + i];
        store_global(out + static_cast<long>(it.entry) * NG + p, qtape_value(x, r, it));
    }
}
}  // namespace

}  // namespace spd

// ---- host side: the event, the configuration and the C ABI (spd_model_qtape_*, spd_qtape_*) ----

namespace {
const char *const kQtapeOff = "no quantile tape configured (spd_model_qtape_configure)";
const char *const kQtapeInvalid = "the quantile tape is invalid until spd_model_qtape_reset";

// the E planes of the state as it stands into out [E][4608]: front end, point kernel
hipError_t qtape_planes(spd_model *m, double *out, hipStream_t s) {
    const spd_model::Qtape &qt = m->qtape;
    hipError_t e = hipSuccess;
    for (const auto &range : qt.set.ranges)
        if (e == hipSuccess) e = sample_front(m, qt, range.first, range.second, s);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(qtape_point_kernel, dim3(kTiles, qt.nplanes), dim3(kT), 0, s, qt.planes, qt.items, qt.member_list, qt.r, qt.slab,
                           qt.slab_fields, m->stored32 ? 1 : 0, out);
        e = hipGetLastError();
    }
    return e;
}
static_assert(SPD_Q_MIN == kQtapeMin && SPD_Q_MAX == kQtapeMaxOp && SPD_Q_QUANTILE == kQtapeQuantile && SPD_Q_PROB_ABOVE == kQtapeProbAbove &&
                  SPD_Q_PROB_BELOW == kQtapeProbBelow,
              "the ops of the C ABI are the header's");
}  // namespace

int spd::qtape_event(spd_model *m, hipStream_t s, const char *who) {
    spd_model::Qtape &qt = m->qtape;
    const long long n = qt.ring.taken + 1;
    const size_t per_slot = qt.entries.size() * NG;
    const hipError_t e = qtape_planes(m, qt.data + static_cast<size_t>(qt.ring.slot(n)) * per_slot, s);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return m_fail(SPD_E_DEVICE, std::string(who) + ": quantile tape: " + hipGetErrorString(e));
    }
    qt.ring.taken = n;
    qt.ring.stamp(n, m->current_step, m->cal);
    ++qt.applied;
    return SPD_OK;
}

extern "C" {

int spd_qtape_check(const char *const *names, const int *levels, const int *ops, const double *params, int n_entries, const int32_t *mask,
                    int members, int every, int capacity, int in_loop) {
    const char *who = "spd_model_qtape_configure";
    if (every < 1) return m_fail(SPD_E_ARG, std::string(who) + ": every must be at least 1");
    if (capacity < 1) return m_fail(SPD_E_ARG, std::string(who) + ": capacity must be at least 1");
    if (in_loop != 0 && in_loop != 1) return m_fail(SPD_E_ARG, std::string(who) + ": in_loop must be 0 or 1");
    if (n_entries < 1 || n_entries > kQtapeMaxEntries)
        return m_fail(SPD_E_ARG, std::string(who) + ": n_entries must be 1 ... " + std::to_string(kQtapeMaxEntries) + ", got " +
                                     std::to_string(n_entries));
    if (!names || !levels || !ops || !params) return m_fail(SPD_E_ARG, std::string(who) + ": bad list of entries");
    for (int k = 0; k < n_entries; ++k) {
        const int id = entry_id(who, names[k], SPD_CATALOGUE_LIST);
        if (id < 0) return SPD_E_ARG;
        if (int rc = check_entry_level(who, k, names[k], id, levels[k])) return rc;
        const std::string entry = entry_text(k, names[k]);
        if (ops[k] < SPD_Q_MIN || ops[k] > SPD_Q_PROB_BELOW)
            return m_fail(SPD_E_ARG, std::string(who) + ": unknown op " + std::to_string(ops[k]) + " of " + entry +
                                         " (SPD_Q_MIN 0, SPD_Q_MAX 1, SPD_Q_QUANTILE 2, SPD_Q_PROB_ABOVE 3, SPD_Q_PROB_BELOW 4)");
        if (ops[k] == SPD_Q_QUANTILE && !(params[k] >= 0.0 && params[k] <= 1.0))  // (a NaN fails both comparisons)
            return m_fail(SPD_E_ARG, std::string(who) + ": the quantile " + std::to_string(params[k]) + " of " + entry + " is not within 0 ... 1");
        if ((ops[k] == SPD_Q_PROB_ABOVE || ops[k] == SPD_Q_PROB_BELOW) && !std::isfinite(params[k]))
            return m_fail(SPD_E_ARG, std::string(who) + ": the threshold of " + entry + " is not finite");
    }
    // (the member mask needs the member count: checked once the model is known)
    return mask ? check_member_mask(who, mask, members, kQtapeMax, "the order statistics take") : SPD_OK;
}

int spd_model_qtape_configure(spd_model_handle m, const char *const *names, const int *levels, const int *ops, const double *params, int n_entries,
                              const int32_t *mask, int every, int capacity, int in_loop) {
    const char *who = "spd_model_qtape_configure";
    // (the arguments first, in the header's order: nothing in the first block needs the device or a model)
    if (int rc = spd_qtape_check(names, levels, ops, params, n_entries, nullptr, 0, every, capacity, in_loop)) return rc;
    if (!mask) return m_fail(SPD_E_ARG, std::string(who) + ": null member mask");
    if (int rc = configure_allowed(m, who)) return rc;
    if (int rc = spd_qtape_check(names, levels, ops, params, n_entries, mask, m->M, every, capacity, in_loop)) return rc;
    std::vector<spd_model::Qtape::Entry> entries;
    for (int k = 0; k < n_entries; ++k) entries.push_back({stats_id(names[k]), levels[k], ops[k], params[k]});
    if (int rc = check_plev_entries(m, who, names, entries)) return rc;
    spd_model::Qtape &qt = m->qtape;
    if (int rc = retire(m, qt)) return rc;
    spd_model::Qtape next;
    next.in_loop = in_loop != 0;
    next.every = every;
    next.set = member_set(mask, m->M);
    next.r = static_cast<int>(next.set.members.size());
    const size_t slots = static_cast<size_t>(capacity), E = static_cast<size_t>(n_entries);
    // the sample plan and the distinct planes with their entries, as the projection tape builds them
    const EntryPlanes table = entry_planes(entries);
    SamplePlan plan;
    plan_sample(m, table.ids, next, plan);
    const size_t P = table.distinct.size();
    // one allocation: ring | slab | tables[2] | planes | entry descriptors | member list
    const size_t per_slot = E * NG * sizeof(double);
    if (slots > (static_cast<size_t>(-1) / 2) / per_slot) return m_fail(SPD_E_ARG, std::string(who) + ": the ring's size does not fit size_t");
    const size_t ring = sample_up(slots * per_slot);
    const size_t desc = sample_up(P * sizeof(QtapePlane)), list = sample_up(E * sizeof(QtapeItem)), mbytes = sample_up(kQtapeMax * sizeof(int));
    const size_t total = ring + plan.slab_bytes + 2 * plan.table_bytes + desc + list + mbytes;
    void *p = nullptr;
    if (hipMalloc(&p, total) != hipSuccess) {  // the quantile tape is off; the model is as usable as before
        (void)hipGetLastError();
        return m_fail(SPD_E_DEVICE, std::string(who) + ": cannot allocate the quantile tape (" + std::to_string(total) +
                                        " bytes asked for); it is off");
    }
    Carve carve{static_cast<char *>(p)};
    next.alloc = p;
    next.data = carve.take<double>(ring);
    carve_front(carve, plan, next);
    next.planes = carve.take<QtapePlane>(desc);
    next.items = carve.take<QtapeItem>(list);
    next.member_list = carve.take<int>(mbytes);
    // (the ring is written before it is read: only what lies behind it is cleared)
    hipError_t e = hipMemset(static_cast<char *>(p) + ring, 0, total - ring);
    std::vector<SampleSource> sources;  // (per plane of plan.vars, in their order)
    if (e == hipSuccess) e = build_sample_front(m, plan, next, sources);
    std::vector<QtapePlane> host_planes;
    std::vector<QtapeItem> host_items;
    for (size_t q = 0; q < P; ++q) {
        QtapePlane plane{plane_source(plan, sources, table.distinct[q].first, table.distinct[q].second), static_cast<int>(host_items.size()), 0};
        table.each_entry_of(q, [&](int k) {
            QtapeItem it = qtape_item(entries[k].op, entries[k].param, next.r);
            it.entry = k;
            host_items.push_back(it);
            ++plane.count;
        });
        host_planes.push_back(plane);
    }
    if (e == hipSuccess) e = hipMemcpy(next.planes, host_planes.data(), host_planes.size() * sizeof(QtapePlane), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(next.items, host_items.data(), host_items.size() * sizeof(QtapeItem), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(next.member_list, next.set.members.data(), next.set.members.size() * sizeof(int), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return upload_failed(who, e, p);
    next.nplanes = static_cast<int>(host_planes.size());
    next.entries = std::move(entries);
    next.ring = SampleRing(capacity, 6);
    next.on = true;
    qt = std::move(next);
    return SPD_OK;
}

int spd_model_qtape_off(spd_model_handle m) {
    const char *who = "spd_model_qtape_off";
    if (int rc = configure_allowed(m, who)) return rc;
    return retire(m, m->qtape);
}

int spd_model_qtape_reset(spd_model_handle m) { return ring_reset(m, "spd_model_qtape_reset", &spd_model::qtape, kQtapeOff); }

int spd_model_qtape_apply(spd_model_handle m, void *stream) {
    const char *who = "spd_model_qtape_apply";
    if (!m) return m_fail(SPD_E_ARG, std::string(who) + ": null model");
    if (int rc = state_call_allowed(m, who, m->qtape.on, kQtapeOff)) return rc;
    M_HIP(hipSetDevice(m->ctx->device));
    return qtape_event(m, static_cast<hipStream_t>(stream), who);
}

int spd_model_qtape_compute(spd_model_handle m, void *dst_device, size_t dst_bytes, void *stream) {
    const char *who = "spd_model_qtape_compute";
    if (!m) return m_fail(SPD_E_ARG, std::string(who) + ": null model");
    if (int rc = state_call_allowed(m, who, m->qtape.on, kQtapeOff)) return rc;
    if (int rc = destination_fits(who, dst_device, dst_bytes, m->qtape.entries.size() * NG * sizeof(double), sizeof(double))) return rc;
    M_HIP(hipSetDevice(m->ctx->device));
    const hipError_t e = qtape_planes(m, static_cast<double *>(dst_device), static_cast<hipStream_t>(stream));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return m_fail(SPD_E_DEVICE, std::string(who) + ": " + hipGetErrorString(e));
    }
    return SPD_OK;
}

int spd_model_qtape_read(spd_model_handle m, int entry, int t0, int nt, void *dst_device, size_t dst_bytes, void *stream) {
    const char *who = "spd_model_qtape_read";
    if (!m) return m_fail(SPD_E_ARG, std::string(who) + ": null model");
    const spd_model::Qtape &qt = m->qtape;
    if (int rc = read_allowed(m, who, qt.on, kQtapeOff, qt.validity, kQtapeInvalid)) return rc;
    const int E = static_cast<int>(qt.entries.size());
    if (entry < 0 || entry >= E)
        return m_fail(SPD_E_ARG, std::string(who) + ": entry " + std::to_string(entry) + " is out of range (0 ... " + std::to_string(E - 1) + ")");
    if (int rc = held_range(who, qt.ring, t0, nt, "event")) return rc;
    if (int rc = destination_fits(who, dst_device, dst_bytes, static_cast<size_t>(nt) * NG * sizeof(double), sizeof(double))) return rc;
    // (one "member" whose values are the entry's plane: a strided device copy)
    return gather_slots(m, who, qt.data + static_cast<size_t>(entry) * NG, NG, static_cast<size_t>(E) * NG, 1, t0, nt, qt.ring, dst_device, stream);
}

int spd_model_qtape_rows(spd_model_handle m, int32_t *rows, int max_rows) {
    return ring_rows(m, "spd_model_qtape_rows", &spd_model::qtape, kQtapeOff, rows, max_rows);
}

int spd_model_qtape_info(spd_model_handle m, int *r, int *n_entries, int *every, int *capacity, long long *taken, int *in_loop, long long *applied) {
    if (!m) return m_fail(SPD_E_ARG, "spd_model_qtape_info: null model");
    const spd_model::Qtape &qt = m->qtape;  // (a model without a quantile tape: all zero)
    if (r) *r = qt.r;
    if (n_entries) *n_entries = static_cast<int>(qt.entries.size());
    if (every) *every = qt.every;
    if (capacity) *capacity = qt.ring.capacity;
    if (taken) *taken = qt.ring.taken;
    if (in_loop) *in_loop = qt.in_loop ? 1 : 0;
    if (applied) *applied = qt.applied;
    return SPD_OK;
}

int spd_qtape_host(const double *x, int r, const int *ops, const double *params, int n_entries, double *out) {
    const char *who = "spd_qtape_host";
    if (!x || !ops || !params || !out) return m_fail(SPD_E_ARG, std::string(who) + ": null argument");
    if (r < 2 || r > kQtapeMax) return m_fail(SPD_E_ARG, std::string(who) + ": r must be 2 ... " + std::to_string(kQtapeMax) + ", got " + std::to_string(r));
    if (n_entries < 1 || n_entries > kQtapeMaxEntries)
        return m_fail(SPD_E_ARG, std::string(who) + ": n_entries must be 1 ... " + std::to_string(kQtapeMaxEntries) + ", got " +
                                     std::to_string(n_entries));
    std::vector<QtapeItem> items;
    for (int k = 0; k < n_entries; ++k) {
        if (ops[k] < SPD_Q_MIN || ops[k] > SPD_Q_PROB_BELOW) return m_fail(SPD_E_ARG, std::string(who) + ": unknown op " + std::to_string(ops[k]));
        if (ops[k] == SPD_Q_QUANTILE && !(params[k] >= 0.0 && params[k] <= 1.0))
            return m_fail(SPD_E_ARG, std::string(who) + ": the quantile " + std::to_string(params[k]) + " is not within 0 ... 1");
        if (ops[k] > SPD_Q_QUANTILE && !std::isfinite(params[k])) return m_fail(SPD_E_ARG, std::string(who) + ": the threshold is not finite");
        items.push_back(qtape_item(ops[k], params[k], r));
        items.back().entry = k;
    }
    spd::qtape_plane_host(x, r, items.data(), n_entries, out);
    return SPD_OK;
}

}  // extern "C"
