// Weighted sums of the state's grid-space fields, formed on the GPU behind the sampled steps of a multi-step call and kept as
// scalar series (spd_model_projtape_*, include/pyspeedy_amd.h; the definition is in projtape.hpp and DESIGN section 4j).
//
// A sample is what an fp64 tape of the same name holds: model.hip runs the tape's front end into a slab of the recorder's own, and
// the kernel below applies export_unit (sample_source.hpp) exactly as tape_store_kernel does; precnv / precls are read where the
// column kernel stores them, in their stored precision, widened.  One 256-lane workgroup per (member, distinct plane among the
// entries): it loads its plane once, 18 values per lane at p = t + 256 r (every load of a wavefront is 512 contiguous bytes), and
// then serves every entry on that plane -- four at a time: each lane forms the lane sums of four patterns side by side, each in
// the stated order, and leaves them in LDS, and behind one barrier wavefront k folds entry k.  The fold is the stated tree: the
// two halvings that cross wavefronts (128, 64) are read from LDS by lane t < 64 as (tree[t] + tree[t + 128]) + (tree[t + 64] +
// tree[t + 192]), the six inside a wavefront (32 ... 1) are tree[t] + tree[t + half] through a cross-lane move.  A lane >= half
// adds something nobody reads: lane t < half of the next halving reads lane t + half / 2 < half.  The patterns (36 KB each, at
// most 64) are read by every workgroup and stay in cache; a plane is read from memory once, however many patterns project it.
// Every product and sum is rounded on its own (no contraction, the __d*_rn intrinsics), so that the numpy restatement gives the
// same bits whatever the launch plan.  The front end wrote the slab just before: ordinary loads.  The ring is written once and
// read by the host's gather only.
#include <hip/hip_runtime.h>

#include "global_mem.hpp"
#include "model_state.hpp"
#include "projtape.hpp"
#include "tables.hpp"

namespace spd {

namespace {
constexpr int kT = 256;
constexpr int kPer = NG / kT;  // 18 points per lane
constexpr int kBatch = 4;      // entries per barrier: one per wavefront of the workgroup
static_assert(NG % kT == 0, "a plane is a whole number of passes of the workgroup");
static_assert(kBatch * 64 == kT, "one wavefront per entry of a batch");

// blockIdx.x: distinct plane (descriptor), blockIdx.y: member of the group
__global__ __launch_bounds__(kT) void projtape_kernel(const ProjTapePlane *__restrict__ planes, const ProjTapeItem *__restrict__ items,
                                                      const double *__restrict__ weights, const double *__restrict__ slab, int slab_fields,
                                                      double *__restrict__ ring_slot, int n_entries, int first, int store32) {
#pragma clang fp contract(off)
    __shared__ double tree[kBatch][kT];
    const ProjTapePlane d = planes[blockIdx.x];
    const int t = threadIdx.x;
    const long i = first + static_cast<long>(blockIdx.y);
    double x[kPer];
    // with_sample_plane's decision (sample_source.hpp), written out: with the unrolled loop behind a function boundary of any kind
    // the compiler forms the 18 values in another order and commutes the operands of the first products below
    if (d.source.slab_plane >= 0) {
        const double *src = slab + (i * slab_fields + d.source.slab_plane) * NG;
#pragma unroll
        for (int r = 0; r < kPer; ++r) x[r] = export_unit(load_global(src + t + kT * r), d.source.unit);
    } else if (store32) {
        const float *src = static_cast<const float *>(d.source.src) + i * NG;
#pragma unroll
        for (int r = 0; r < kPer; ++r) x[r] = export_unit(static_cast<double>(load_global(src + t + kT * r)), d.source.unit);
    } else {
        const double *src = static_cast<const double *>(d.source.src) + i * NG;
#pragma unroll
        for (int r = 0; r < kPer; ++r) x[r] = export_unit(load_global(src + t + kT * r), d.source.unit);
    }
    const int wave = t >> 6, lane = t & 63;
    for (int e0 = 0; e0 < d.count; e0 += kBatch) {
        const int nb = d.count - e0 < kBatch ? d.count - e0 : kBatch;
        // the four lane sums side by side, so that the loads of four patterns are in flight together (a batch of fewer entries
        // forms its last one again and stores it nowhere); each sum keeps its own stated order
        const double *w[kBatch];
        double s[kBatch];
#pragma unroll
        for (int b = 0; b < kBatch; ++b) {
            w[b] = weights + static_cast<long>(items[d.first + e0 + (b < nb ? b : nb - 1)].pattern) * NG + t;
            s[b] = __dmul_rn(w[b][0], x[0]);
        }
#pragma unroll
        for (int r = 1; r < kPer; ++r) {
#pragma unroll
            for (int b = 0; b < kBatch; ++b) s[b] = __dadd_rn(s[b], __dmul_rn(w[b][kT * r], x[r]));
        }
#pragma unroll
        for (int b = 0; b < kBatch; ++b) tree[b][t] = s[b];
        __syncthreads();
        if (wave < nb) {
            const double v = projtape_fold(tree[wave], lane);
            if (lane == 0) ring_slot[i * n_entries + items[d.first + e0 + wave].column] = v;
        }
        __syncthreads();  // (the next batch overwrites the rows)
    }
}
}  // namespace

// One launch for the members [first, first + count), all planes.  weights: [P][4608]; slab: [M][slab_fields][4608] fp64, as the
// front end left it; store32: the model keeps precnv / precls as float; ring_slot: member 0 of the sample's slot, [M][n_entries].
hipError_t run_projtape_sample(const ProjTapePlane *planes, int nplanes, const ProjTapeItem *items, const double *weights, const double *slab,
                               int slab_fields, double *ring_slot, int n_entries, int first, int count, int store32, hipStream_t s) {
    if (nplanes == 0 || count == 0) return hipSuccess;
    hipLaunchKernelGGL(projtape_kernel, dim3(nplanes, count), dim3(kT), 0, s, planes, items, weights, slab, slab_fields, ring_slot,
                       n_entries, first, store32);
    return hipGetLastError();
}

}  // namespace spd

// ---- host side: the step loop's sample, the configuration and the C ABI (spd_model_projtape_*) ----

namespace {
constexpr int kProjMaxPatterns = 64, kProjMaxEntries = 1024;
const char *const kProjOff = "no projection tape configured (spd_model_projtape_configure)";
}  // namespace

// the sample of members [first, first + count): the front end into the recorder's own slab, then every entry's sum into ring slot
// (n - 1) % capacity
hipError_t spd::projtape_sample(spd_model *m, int first, int count, long long n, hipStream_t s) {
    const spd_model::ProjTape &pt = m->projtape;
    const size_t per_slot = static_cast<size_t>(m->M) * pt.entries.size();
    hipError_t e = sample_front(m, pt, first, count, s);
    if (e == hipSuccess)
        e = run_projtape_sample(pt.planes, pt.nplanes, pt.items, pt.weights, pt.slab, pt.slab_fields,
                                pt.data + static_cast<size_t>(pt.ring.slot(n)) * per_slot, static_cast<int>(pt.entries.size()), first, count,
                                m->stored32 ? 1 : 0, s);
    return e;
}

extern "C" {

int spd_model_projtape_configure(spd_model_handle m, const double *weights, int n_patterns, const char *const *names, const int *levels,
                                 const int *patterns, int n_entries, int every, int capacity) {
    const char *who = "spd_model_projtape_configure";
    // (the arguments first, in the header's order: nothing in this block needs the device or a model; n_entries = 0 is "off")
    std::vector<PatternEntry> entries;
    if (n_entries != 0) {
        if (every < 1) return m_fail(SPD_E_ARG, std::string(who) + ": every must be at least 1");
        if (capacity < 1) return m_fail(SPD_E_ARG, std::string(who) + ": capacity must be at least 1");
        if (n_patterns < 1 || n_patterns > kProjMaxPatterns)
            return m_fail(SPD_E_ARG, std::string(who) + ": n_patterns must be 1 ... " + std::to_string(kProjMaxPatterns) + ", got " +
                                         std::to_string(n_patterns));
        if (n_entries < 0 || n_entries > kProjMaxEntries)
            return m_fail(SPD_E_ARG, std::string(who) + ": n_entries must be 0 ... " + std::to_string(kProjMaxEntries) + ", got " +
                                         std::to_string(n_entries));
        if (!weights) return m_fail(SPD_E_ARG, std::string(who) + ": null weights");
        if (!names || !levels || !patterns) return m_fail(SPD_E_ARG, std::string(who) + ": bad list of entries");
        if (int rc = check_weight_maps(who, weights, n_patterns)) return rc;
        for (int k = 0; k < n_entries; ++k) {
            const int id = entry_id(who, names[k], SPD_CATALOGUE_LIST);
            if (id < 0) return SPD_E_ARG;
            entries.push_back({id, levels[k], patterns[k]});
        }
        for (int k = 0; k < n_entries; ++k) {
            if (int rc = check_entry_level(who, k, names[k], entries[k].name, levels[k])) return rc;
            if (int rc = check_entry_pattern(who, k, names[k], patterns[k], n_patterns)) return rc;
        }
    }
    if (int rc = configure_allowed(m, who)) return rc;
    if (int rc = check_plev_entries(m, who, names, entries)) return rc;
    spd_model::ProjTape &pt = m->projtape;
    if (int rc = retire(m, pt)) return rc;
    if (n_entries == 0) return SPD_OK;  // off
    spd_model::ProjTape next;
    next.every = every;
    next.npatterns = n_patterns;
    const size_t M = static_cast<size_t>(m->M), slots = static_cast<size_t>(capacity), E = static_cast<size_t>(n_entries);
    // the sample plan over the names among the entries (the front end transforms a name's every level), and the entries sorted by
    // distinct plane (stable: the caller's order within a plane)
    const EntryPlanes table = entry_planes(entries);
    SamplePlan plan;
    plan_sample(m, table.ids, next, plan);
    // one allocation: ring | patterns | slab | tables[2] | plane descriptors | entry list
    const size_t per_slot = M * E * sizeof(double);
    if (slots > (static_cast<size_t>(-1) / 2) / per_slot) return m_fail(SPD_E_ARG, std::string(who) + ": the size of the series does not fit size_t");
    const size_t ring = sample_up(slots * per_slot), maps = sample_up(static_cast<size_t>(n_patterns) * NG * sizeof(double));
    const size_t desc = sample_up(table.distinct.size() * sizeof(ProjTapePlane)), list = sample_up(E * sizeof(ProjTapeItem));
    const size_t total = ring + maps + plan.slab_bytes + 2 * plan.table_bytes + desc + list;
    void *p = nullptr;
    if (hipMalloc(&p, total) != hipSuccess) {  // the projection tape is off; the model is as usable as before
        (void)hipGetLastError();
        return m_fail(SPD_E_DEVICE, std::string(who) + ": cannot allocate the projection tape (" + std::to_string(total) +
                                        " bytes asked for: " + std::to_string(capacity) + " samples of " + std::to_string(per_slot) +
                                        " bytes); the projection tape is off");
    }
    Carve carve{static_cast<char *>(p)};
    next.alloc = p;
    next.data = carve.take<double>(ring);
    next.weights = carve.take<double>(maps);
    carve_front(carve, plan, next);
    next.planes = carve.take<ProjTapePlane>(desc);
    next.items = carve.take<ProjTapeItem>(list);
    std::vector<SampleSource> sources;  // (per plane of plan.vars, in their order)
    hipError_t e = build_sample_front(m, plan, next, sources);
    std::vector<ProjTapePlane> host_planes;
    std::vector<ProjTapeItem> host_items;
    for (size_t q = 0; q < table.distinct.size(); ++q) {
        ProjTapePlane d{};
        d.source = plane_source(plan, sources, table.distinct[q].first, table.distinct[q].second);
        d.first = static_cast<int>(host_items.size());
        table.each_entry_of(q, [&](int k) { host_items.push_back({entries[k].pattern, k}); });
        d.count = static_cast<int>(host_items.size()) - d.first;
        host_planes.push_back(d);
    }
    if (e == hipSuccess) e = hipMemcpy(next.weights, weights, static_cast<size_t>(n_patterns) * NG * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(next.planes, host_planes.data(), host_planes.size() * sizeof(ProjTapePlane), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(next.items, host_items.data(), host_items.size() * sizeof(ProjTapeItem), hipMemcpyHostToDevice);
    if (e != hipSuccess) return upload_failed(who, e, p);
    next.nplanes = static_cast<int>(host_planes.size());
    next.entries = std::move(entries);
    next.ring = SampleRing(capacity, 6);
    next.on = true;
    pt = std::move(next);
    return SPD_OK;
}

int spd_model_projtape_reset(spd_model_handle m) { return ring_reset(m, "spd_model_projtape_reset", &spd_model::projtape, kProjOff); }

int spd_model_projtape_info(spd_model_handle m, long long *taken, int *held, int *capacity, int *every, int *n_patterns, int *n_entries) {
    if (!m) return m_fail(SPD_E_ARG, "spd_model_projtape_info: null model");
    const spd_model::ProjTape &pt = m->projtape;
    if (!pt.on) return m_fail(SPD_E_ARG, std::string("spd_model_projtape_info: ") + kProjOff);
    if (taken) *taken = pt.ring.taken;
    if (held) *held = static_cast<int>(pt.ring.held());
    if (capacity) *capacity = pt.ring.capacity;
    if (every) *every = pt.every;
    if (n_patterns) *n_patterns = pt.npatterns;
    if (n_entries) *n_entries = static_cast<int>(pt.entries.size());
    return SPD_OK;
}

int spd_model_projtape_times(spd_model_handle m, int32_t *rows, int max_rows) {
    return ring_rows(m, "spd_model_projtape_times", &spd_model::projtape, kProjOff, rows, max_rows);
}

int spd_model_projtape_read(spd_model_handle m, int first, int count, int t0, int nt, void *dst_device, size_t dst_bytes, void *stream) {
    const char *who = "spd_model_projtape_read";
    if (!m) return m_fail(SPD_E_ARG, std::string(who) + ": null model");
    const spd_model::ProjTape &pt = m->projtape;
    if (int rc = read_allowed(m, who, pt.on, kProjOff, pt.validity, "the projection tape is invalid until spd_model_projtape_reset")) return rc;
    if (first < 0 || count < 0 || first + count > m->M) return m_fail(SPD_E_ARG, std::string(who) + ": member range out of bounds");
    if (int rc = held_range(who, pt.ring, t0, nt, "sample")) return rc;
    const size_t per = pt.entries.size();
    const size_t need = static_cast<size_t>(count) * static_cast<size_t>(nt) * per * sizeof(double);
    if (int rc = destination_fits(who, dst_device, dst_bytes, need, sizeof(double))) return rc;
    // (the ring is [slot][M][E] as a spectra ring is [slot][M][per]: the same gather)
    return gather_slots(m, who, pt.data + static_cast<size_t>(first) * per, per, static_cast<size_t>(m->M) * per, count, t0, nt, pt.ring, dst_device, stream);
}

}  // extern "C"
