// The verification tape: scores of a masked ensemble against a truth member of the same model, formed on the GPU at a join of the
// member groups and kept as scalar series (spd_model_verif_*, include/pyspeedy_amd.h; the arithmetic is verif_point.hpp, the
// definition DESIGN section 4n).
//
// An event is the sample front end for the member ranges that cover the mask and the truth, then two launches on the same stream.
// (1) verif_point_kernel, one workgroup per 256 points of a distinct plane, a lane per point: the lane gathers the truth and the r
// members' values -- what an fp64 tape of that name holds: export_unit on the slab's value, or on precnv / precls read where the
// column kernel stores them, widened -- eight loads in flight at a time, into a column of its own in the LDS, [64][256] doubles =
// 128 KiB.  The column is indexed by the run-time r and by the double loop of the CRPS; a register array would have to be walked
// with compile-time indices, which for the pair loop means 2016 unrolled terms per r or scratch memory.  In the LDS a wavefront's
// read of x_j is 512 contiguous bytes without a bank conflict, no lane reads another's column (no barrier), and the one
// workgroup per CU that 128 KiB allow is all a launch of a few dozen workgroups asks for.  The lane then runs verif_point and leaves
// e, se, v, crps and its histogram bin in a scratch [plane][4][4608] / [plane][4608].  (2) verif_reduce_kernel, one workgroup per
// entry: each lane forms the four lane sums of w times the scratch side by side in the projection tape's order, wavefront k folds
// sum k with the projection tape's own fold (projtape_fold), and the bins of the points with w != 0 are counted with LDS atomics
// and stored.  Every product and sum is rounded on its own (no contraction, the __d*_rn intrinsics).  Nothing here writes into
// the model, and no atomic touches device memory.
#include <hip/hip_runtime.h>

#include "global_mem.hpp"
#include "model_state.hpp"
#include "tables.hpp"
#include "verif.hpp"

namespace spd {

namespace {
constexpr int kT = kVerifLanes;
constexpr int kPer = kVerifPasses;
constexpr int kTiles = NG / kT;  // workgroups of the point kernel per plane
constexpr int kLoads = 8;        // members whose loads are in flight together
static_assert(NG == kVerifPoints, "a plane is 18 passes of 256 lanes");
static_assert(kVerifMax * kT * sizeof(double) <= 160 * 1024, "the members' columns fit the LDS of a CU");

// a lane's column of the LDS: member j of its point
struct LdsColumn {
    const double *at;
    __device__ __forceinline__ double operator()(int j) const { return at[j * kT]; }
};

// The truth and the r members of one point into the lane's column: `plane` is the point in member 0's plane as it is stored
// (precnv / precls: float while the model stores them so), `stride` the elements between two members.  kLoads members' loads are
// issued together, then widened, converted and stored; the decision where the plane lies is taken once, outside (with_sample_plane).
struct VerifGather {
    template <class T>
    __device__ __forceinline__ int operator()(const T *plane, long stride, const int *const &members, const int &r, const int &truth, const int &unit,
                                              const long &p, double *const &column, double &y) const {
        const T *at = plane + p;
        const T yraw = load_global(at + truth * stride);
        for (int j0 = 0; j0 < r; j0 += kLoads) {
            T raw[kLoads];
#pragma unroll
            for (int b = 0; b < kLoads; ++b) raw[b] = load_global(at + members[j0 + b < r ? j0 + b : r - 1] * stride);
#pragma unroll
            for (int b = 0; b < kLoads; ++b)
                if (j0 + b < r) column[(j0 + b) * kT] = export_unit(static_cast<double>(raw[b]), unit);
        }
        y = export_unit(static_cast<double>(yraw), unit);
        return 0;
    }
};

// blockIdx.x: 256 points, blockIdx.y: distinct plane
__global__ __launch_bounds__(kT) void verif_point_kernel(const SampleSource *__restrict__ planes, const int *__restrict__ members, int r, int truth,
                                                         const double *__restrict__ slab, int slab_fields, int store32, double *__restrict__ point,
                                                         int *__restrict__ bin) {
#pragma clang fp contract(off)
    __shared__ double col[kVerifMax * kT];
    if (r < 2 || r > kVerifMax) return;
    const SampleSource d = planes[blockIdx.y];
    const int t = threadIdx.x;
    const long p = static_cast<long>(blockIdx.x) * kT + t;
    double *const column = col + t;
    const int *const list = members;
    double y;
    with_sample_plane(d, slab, slab_fields, store32 != 0, 0L, VerifGather{}, list, r, truth, d.unit, p, column, y);
    const VerifPoint q = verif_point(LdsColumn{column}, r, y);
    double *out = point + static_cast<long>(blockIdx.y) * 4 * NG + p;
    store_global(out, q.e);
    store_global(out + NG, q.se);
    store_global(out + 2 * NG, q.v);
    store_global(out + 3 * NG, q.crps);
    store_global(bin + static_cast<long>(blockIdx.y) * NG + p, q.bin);
}

// blockIdx.x: entry; blockIdx.y: 0 the scores of the entry, 1 (phase 0 of an event) the blank second half of the slot.
// scores: [2][E][4], counts: [2][E][66] of the slot's phase that is written (the blank half lies behind it).
__global__ __launch_bounds__(kT) void verif_reduce_kernel(const VerifItem *__restrict__ items, const double *__restrict__ weights,
                                                          const double *__restrict__ point, const int *__restrict__ bin, int n_entries,
                                                          double *__restrict__ scores, int *__restrict__ counts) {
#pragma clang fp contract(off)
    __shared__ double tree[4][kT];
    __shared__ int hist[kVerifCounts];
    const int t = threadIdx.x, e = blockIdx.x;
    if (blockIdx.y == 1) {
        if (t < 4) store_global(scores + (static_cast<long>(n_entries) + e) * 4 + t, __builtin_nan(""));
        if (t < kVerifCounts) store_global(counts + (static_cast<long>(n_entries) + e) * kVerifCounts + t, -1);
        return;
    }
    const VerifItem item = items[e];
    const double *w = weights + static_cast<long>(item.pattern) * NG + t;
    const double *src = point + static_cast<long>(item.plane) * 4 * NG + t;
    const int *b = bin + static_cast<long>(item.plane) * NG + t;
    if (t < kVerifCounts) hist[t] = 0;
    double wv[kPer], s[4];
    int bv[kPer];
#pragma unroll
    for (int i = 0; i < kPer; ++i) wv[i] = load_global(w + kT * i), bv[i] = load_global(b + kT * i);
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k] = __dmul_rn(wv[0], load_global(src + k * NG));
#pragma unroll
    for (int i = 1; i < kPer; ++i) {
#pragma unroll
        for (int k = 0; k < 4; ++k) s[k] = __dadd_rn(s[k], __dmul_rn(wv[i], load_global(src + k * NG + kT * i)));
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) tree[k][t] = s[k];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kPer; ++i)
        if (wv[i] != 0.0 && static_cast<unsigned>(bv[i]) < static_cast<unsigned>(kVerifCounts)) atomicAdd(&hist[bv[i]], 1);
    const int wave = t >> 6, lane = t & 63;
    const double v = projtape_fold(tree[wave], lane);
    if (lane == 0) store_global(scores + static_cast<long>(e) * 4 + wave, v);
    __syncthreads();
    if (t < kVerifCounts) store_global(counts + static_cast<long>(e) * kVerifCounts + t, hist[t]);
}
}  // namespace

}  // namespace spd

// ---- host side: the event, the configuration and the C ABI (spd_model_verif_*, spd_verif_*) ----

namespace {
constexpr int kVerifMaxPatterns = 64, kVerifMaxEntries = 256;
const char *const kVerifOff = "no verification tape configured (spd_model_verif_configure)";
const char *const kVerifInvalid = "the verification tape is invalid until spd_model_verif_reset";

// the scores of the state as it stands: front end, point kernel, reduce kernel.  scores / counts: [E][4] / [E][66] of one phase;
// blank: the same extent behind them is filled with NaN / -1.
hipError_t verif_scores(spd_model *m, double *scores, int *counts, bool blank, hipStream_t s) {
    const spd_model::Verif &vf = m->verif;
    const int E = static_cast<int>(vf.entries.size());
    hipError_t e = hipSuccess;
    for (const auto &range : vf.set.ranges)
        if (e == hipSuccess) e = sample_front(m, vf, range.first, range.second, s);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(verif_point_kernel, dim3(kTiles, vf.nplanes), dim3(kT), 0, s, vf.planes, vf.member_list, vf.r, vf.truth, vf.slab,
                           vf.slab_fields, m->stored32 ? 1 : 0, vf.point, vf.bin);
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        hipLaunchKernelGGL(verif_reduce_kernel, dim3(E, blank ? 2 : 1), dim3(kT), 0, s, vf.items, vf.weights, vf.point, vf.bin, E, scores, counts);
        e = hipGetLastError();
    }
    return e;
}
}  // namespace

int spd::verif_event(spd_model *m, hipStream_t s, const char *who, int phase) {
    spd_model::Verif &vf = m->verif;
    const size_t E = vf.entries.size();
    const long long n = phase == 0 ? vf.ring.taken + 1 : vf.ring.taken;
    const size_t half = static_cast<size_t>(vf.ring.slot(n)) * 2 + static_cast<size_t>(phase);
    const hipError_t e = verif_scores(m, vf.data + half * E * 4, vf.counts + half * E * kVerifCounts, phase == 0, s);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return m_fail(SPD_E_DEVICE, std::string(who) + ": verification: " + hipGetErrorString(e));
    }
    if (phase == 0) {
        ++vf.ring.taken;
        vf.ring.stamp(vf.ring.taken, m->current_step, m->cal);
        ++vf.applied;
    }
    vf.ring.row(n)[6] = phase;
    return SPD_OK;
}

extern "C" {

int spd_verif_check(const double *weights, int n_patterns, const char *const *names, const int *levels, const int *patterns, int n_entries,
                    const int32_t *mask, int members, int truth, int every, int capacity, int in_loop) {
    const char *who = "spd_model_verif_configure";
    if (every < 1) return m_fail(SPD_E_ARG, std::string(who) + ": every must be at least 1");
    if (capacity < 1) return m_fail(SPD_E_ARG, std::string(who) + ": capacity must be at least 1");
    if (in_loop != 0 && in_loop != 1) return m_fail(SPD_E_ARG, std::string(who) + ": in_loop must be 0 or 1");
    if (n_patterns < 1 || n_patterns > kVerifMaxPatterns)
        return m_fail(SPD_E_ARG, std::string(who) + ": n_patterns must be 1 ... " + std::to_string(kVerifMaxPatterns) + ", got " +
                                     std::to_string(n_patterns));
    if (n_entries < 1 || n_entries > kVerifMaxEntries)
        return m_fail(SPD_E_ARG, std::string(who) + ": n_entries must be 1 ... " + std::to_string(kVerifMaxEntries) + ", got " +
                                     std::to_string(n_entries));
    if (!weights) return m_fail(SPD_E_ARG, std::string(who) + ": null weights");
    if (!names || !levels || !patterns) return m_fail(SPD_E_ARG, std::string(who) + ": bad list of entries");
    if (int rc = check_weight_maps(who, weights, n_patterns)) return rc;
    for (int k = 0; k < n_entries; ++k) {
        const int id = entry_id(who, names[k], SPD_CATALOGUE_LIST);
        if (id < 0) return SPD_E_ARG;
        if (int rc = check_entry_level(who, k, names[k], id, levels[k])) return rc;
        if (int rc = check_entry_pattern(who, k, names[k], patterns[k], n_patterns)) return rc;
    }
    if (!mask) return SPD_OK;  // (the member mask needs the member count: checked once the model is known)
    if (int rc = check_member_mask(who, mask, members, kVerifMax, "the scores take")) return rc;
    if (truth < 0 || truth >= members)
        return m_fail(SPD_E_ARG, std::string(who) + ": the truth member " + std::to_string(truth) + " is out of range (0 ... " +
                                     std::to_string(members - 1) + ")");
    if (mask[truth])
        return m_fail(SPD_E_ARG, std::string(who) + ": the truth member " + std::to_string(truth) + " is masked in: the truth lies outside the ensemble");
    return SPD_OK;
}

int spd_model_verif_configure(spd_model_handle m, const double *weights, int n_patterns, const char *const *names, const int *levels,
                              const int *patterns, int n_entries, const int32_t *mask, int truth, int every, int capacity, int in_loop) {
    const char *who = "spd_model_verif_configure";
    // (the arguments first, in the header's order: nothing in the first block needs the device or a model)
    if (int rc = spd_verif_check(weights, n_patterns, names, levels, patterns, n_entries, nullptr, 0, truth, every, capacity, in_loop)) return rc;
    if (!mask) return m_fail(SPD_E_ARG, std::string(who) + ": null member mask");
    if (int rc = configure_allowed(m, who)) return rc;
    if (int rc = spd_verif_check(weights, n_patterns, names, levels, patterns, n_entries, mask, m->M, truth, every, capacity, in_loop)) return rc;
    std::vector<PatternEntry> entries;
    for (int k = 0; k < n_entries; ++k) entries.push_back({stats_id(names[k]), levels[k], patterns[k]});
    if (int rc = check_plev_entries(m, who, names, entries)) return rc;
    spd_model::Verif &vf = m->verif;
    if (int rc = retire(m, vf)) return rc;
    spd_model::Verif next;
    next.in_loop = in_loop != 0;
    next.every = every;
    next.npatterns = n_patterns;
    next.truth = truth;
    next.set = member_set(mask, m->M, truth);  // (the front end prepares the truth's planes as well)
    next.r = static_cast<int>(next.set.members.size());
    const size_t slots = static_cast<size_t>(capacity), E = static_cast<size_t>(n_entries);
    // the sample plan and the distinct planes, as the projection tape builds them; the entries stay in the caller's order
    const EntryPlanes table = entry_planes(entries);
    SamplePlan plan;
    plan_sample(m, table.ids, next, plan);
    std::vector<VerifItem> host_items;
    for (size_t k = 0; k < E; ++k) host_items.push_back({table.plane_of[k], entries[k].pattern});
    const size_t P = table.distinct.size();
    // one allocation: score ring | count ring | patterns | slab | tables[2] | plane sources | entry list | member list | point | bin
    const size_t per_slot = 2 * E * 4 * sizeof(double), per_slot_counts = 2 * E * kVerifCounts * sizeof(int);
    if (slots > (static_cast<size_t>(-1) / 2) / per_slot_counts) return m_fail(SPD_E_ARG, std::string(who) + ": the ring's size does not fit size_t");
    const size_t ring = sample_up(slots * per_slot), cring = sample_up(slots * per_slot_counts);
    const size_t maps = sample_up(static_cast<size_t>(n_patterns) * NG * sizeof(double));
    const size_t desc = sample_up(P * sizeof(SampleSource)), list = sample_up(E * sizeof(VerifItem)), mbytes = sample_up(kVerifMax * sizeof(int));
    const size_t pbytes = sample_up(P * 4 * NG * sizeof(double)), bbytes = sample_up(P * NG * sizeof(int));
    const size_t total = ring + cring + maps + plan.slab_bytes + 2 * plan.table_bytes + desc + list + mbytes + pbytes + bbytes;
    void *p = nullptr;
    if (hipMalloc(&p, total) != hipSuccess) {  // the verification tape is off; the model is as usable as before
        (void)hipGetLastError();
        return m_fail(SPD_E_DEVICE, std::string(who) + ": cannot allocate the verification tape (" + std::to_string(total) +
                                        " bytes asked for); it is off");
    }
    Carve carve{static_cast<char *>(p)};
    next.alloc = p;
    next.data = carve.take<double>(ring);
    next.counts = carve.take<int>(cring);
    next.weights = carve.take<double>(maps);
    carve_front(carve, plan, next);
    next.planes = carve.take<SampleSource>(desc);
    next.items = carve.take<VerifItem>(list);
    next.member_list = carve.take<int>(mbytes);
    next.point = carve.take<double>(pbytes);
    next.bin = carve.take<int>(bbytes);
    hipError_t e = hipMemset(p, 0, total);
    std::vector<SampleSource> sources;  // (per plane of plan.vars, in their order)
    if (e == hipSuccess) e = build_sample_front(m, plan, next, sources);
    std::vector<SampleSource> host_planes;
    for (const auto &key : table.distinct) host_planes.push_back(plane_source(plan, sources, key.first, key.second));
    if (e == hipSuccess) e = hipMemcpy(next.weights, weights, static_cast<size_t>(n_patterns) * NG * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(next.planes, host_planes.data(), host_planes.size() * sizeof(SampleSource), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(next.items, host_items.data(), host_items.size() * sizeof(VerifItem), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(next.member_list, next.set.members.data(), next.set.members.size() * sizeof(int), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return upload_failed(who, e, p);
    next.nplanes = static_cast<int>(host_planes.size());
    next.entries = std::move(entries);
    next.ring = SampleRing(capacity, 7);
    next.on = true;
    vf = std::move(next);
    return SPD_OK;
}

int spd_model_verif_off(spd_model_handle m) {
    const char *who = "spd_model_verif_off";
    if (int rc = configure_allowed(m, who)) return rc;
    return retire(m, m->verif);
}

int spd_model_verif_reset(spd_model_handle m) { return ring_reset(m, "spd_model_verif_reset", &spd_model::verif, kVerifOff); }

int spd_model_verif_apply(spd_model_handle m, void *stream) {
    const char *who = "spd_model_verif_apply";
    if (!m) return m_fail(SPD_E_ARG, std::string(who) + ": null model");
    if (int rc = state_call_allowed(m, who, m->verif.on, kVerifOff)) return rc;
    M_HIP(hipSetDevice(m->ctx->device));
    return verif_event(m, static_cast<hipStream_t>(stream), who, 0);
}

int spd_model_verif_compute(spd_model_handle m, void *scores_device, size_t scores_bytes, void *hist_device, size_t hist_bytes, void *stream) {
    const char *who = "spd_model_verif_compute";
    if (!m) return m_fail(SPD_E_ARG, std::string(who) + ": null model");
    if (int rc = state_call_allowed(m, who, m->verif.on, kVerifOff)) return rc;
    const size_t E = m->verif.entries.size();
    if (int rc = destination_fits(who, scores_device, scores_bytes, E * 4 * sizeof(double), sizeof(double))) return rc;
    if (int rc = destination_fits(who, hist_device, hist_bytes, E * kVerifCounts * sizeof(int32_t), sizeof(int32_t))) return rc;
    M_HIP(hipSetDevice(m->ctx->device));
    const hipError_t e = verif_scores(m, static_cast<double *>(scores_device), static_cast<int *>(hist_device), false, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return m_fail(SPD_E_DEVICE, std::string(who) + ": " + hipGetErrorString(e));
    }
    return SPD_OK;
}

// the events [t0, t0 + nt) of one of the two rings, `per` doubles a slot, into device memory
static int verif_gather(spd_model_handle m, const char *who, const void *ring, size_t per, size_t align, int t0, int nt, void *dst_device,
                        size_t dst_bytes, void *stream) {
    const spd_model::Verif &vf = m->verif;
    if (int rc = read_allowed(m, who, vf.on, kVerifOff, vf.validity, kVerifInvalid)) return rc;
    if (int rc = held_range(who, vf.ring, t0, nt, "event")) return rc;
    if (int rc = destination_fits(who, dst_device, dst_bytes, static_cast<size_t>(nt) * per * sizeof(double), align)) return rc;
    return gather_slots(m, who, static_cast<const double *>(ring), per, per, 1, t0, nt, vf.ring, dst_device, stream);
}

int spd_model_verif_read(spd_model_handle m, int t0, int nt, void *dst_device, size_t dst_bytes, void *stream) {
    const char *who = "spd_model_verif_read";
    if (!m) return m_fail(SPD_E_ARG, std::string(who) + ": null model");
    return verif_gather(m, who, m->verif.data, 2 * m->verif.entries.size() * 4, sizeof(double), t0, nt, dst_device, dst_bytes, stream);
}

int spd_model_verif_hist(spd_model_handle m, int t0, int nt, void *dst_device, size_t dst_bytes, void *stream) {
    const char *who = "spd_model_verif_hist";
    if (!m) return m_fail(SPD_E_ARG, std::string(who) + ": null model");
    // (66 int32 are 33 doubles: the counts of a slot move as the bit patterns of 2 E 33 doubles)
    static_assert(kVerifCounts % 2 == 0, "an entry's counts are a whole number of doubles");
    return verif_gather(m, who, m->verif.counts, 2 * m->verif.entries.size() * (kVerifCounts / 2), sizeof(double), t0, nt, dst_device, dst_bytes,
                        stream);
}

int spd_model_verif_rows(spd_model_handle m, int32_t *rows, int max_rows) {
    return ring_rows(m, "spd_model_verif_rows", &spd_model::verif, kVerifOff, rows, max_rows);
}

int spd_model_verif_info(spd_model_handle m, int *r, int *truth, int *n_entries, int *every, int *capacity, long long *taken, int *in_loop,
                         long long *applied) {
    if (!m) return m_fail(SPD_E_ARG, "spd_model_verif_info: null model");
    const spd_model::Verif &vf = m->verif;  // (a model without a verification tape: all zero, truth -1)
    if (r) *r = vf.r;
    if (truth) *truth = vf.truth;
    if (n_entries) *n_entries = static_cast<int>(vf.entries.size());
    if (every) *every = vf.every;
    if (capacity) *capacity = vf.ring.capacity;
    if (taken) *taken = vf.ring.taken;
    if (in_loop) *in_loop = vf.in_loop ? 1 : 0;
    if (applied) *applied = vf.applied;
    return SPD_OK;
}

int spd_verif_host(const double *x, int r, const double *y, const double *w, double *out4, int32_t *hist66) {
    const char *who = "spd_verif_host";
    if (!x || !y || !w || !out4 || !hist66) return m_fail(SPD_E_ARG, std::string(who) + ": null argument");
    if (r < 2 || r > kVerifMax) return m_fail(SPD_E_ARG, std::string(who) + ": r must be 2 ... " + std::to_string(kVerifMax) + ", got " + std::to_string(r));
    std::vector<double> scratch(4 * kVerifLanes, 0.0);
    int hist[kVerifCounts];
    spd::verif_entry_host(x, r, y, w, out4, hist, scratch.data());
    for (int k = 0; k < kVerifCounts; ++k) hist66[k] = hist[k];
    return SPD_OK;
}

}  // extern "C"
