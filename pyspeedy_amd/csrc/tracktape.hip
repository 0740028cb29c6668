// Extremes of the state's grid-space fields over regions and their positions, formed on the GPU behind the sampled steps of a
// multi-step call and kept as (value, index, di, dj) series (spd_model_tracktape_*, include/pyspeedy_amd.h; the definition is in
// tracktape.hpp, the rule for one plane in track_point.hpp, and DESIGN section 4p).
//
// A sample is what an fp64 tape of the same name holds: model.hip runs the tape's front end into a slab of the recorder's own, and
// the kernel below applies export_unit (sample_source.hpp) exactly as projtape_kernel does; precnv / precls are read where the
// column kernel stores them, in their stored precision, widened.  One 256-lane workgroup per (member, distinct plane among the
// entries): it loads its plane once, 18 values per lane at p = t + 256 r, keeps them in registers for the scans and in 36 KB of
// LDS for the neighbour reads of the offsets, and then serves every entry on that plane -- four at a time: each lane scans its 18
// points against the region bytes and the windows of four entries side by side, in ascending p, and leaves its four (value, p)
// in LDS; behind one barrier wavefront k folds entry k: the two halvings that cross wavefronts are read from LDS by lane t < 64,
// the six inside a wavefront go through cross-lane moves, every merge by (value, p) (track_merge), so that any tree gives the
// same pair.  Lane 0 forms the offsets from the LDS plane and writes the four doubles and the follow-state with plain vector
// stores.  No atomics; an entry's follow-state is read and written by the one workgroup of its plane and member.  The regions (4.5
// KB each, at most 64) are read by every workgroup and stay in cache.
#include <hip/hip_runtime.h>

#include "global_mem.hpp"
#include "model_state.hpp"
#include "tables.hpp"
#include "track_point.hpp"
#include "tracktape.hpp"

namespace spd {

namespace {
constexpr int kT = kTrackLanes;
constexpr int kPer = kTrackPer;  // 18 points per lane
constexpr int kBatch = 4;        // entries per barrier: one per wavefront of the workgroup
static_assert(NG == kTrackPoints && IX == kTrackIX && IL == kTrackIL, "track_point.hpp speaks of the model's plane");
static_assert(kBatch * 64 == kT, "one wavefront per entry of a batch");

// blockIdx.x: distinct plane (descriptor), blockIdx.y: member of the group
__global__ __launch_bounds__(kT) void tracktape_kernel(const TrackTapePlane *__restrict__ planes, const TrackTapeItem *__restrict__ items,
                                                       const unsigned char *__restrict__ masks, const double *__restrict__ slab, int slab_fields,
                                                       double *__restrict__ ring_slot, int *__restrict__ last, int n_entries, int first,
                                                       int store32) {
#pragma clang fp contract(off)
    __shared__ double plane[NG];
    __shared__ double tree_v[kBatch][kT];
    __shared__ int tree_p[kBatch][kT];
    const TrackTapePlane d = planes[blockIdx.x];
    const int t = threadIdx.x;
    const long i = first + static_cast<long>(blockIdx.y);
    double x[kPer];
    // (the three source forms written out, as in projtape_kernel)
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
#pragma unroll
    for (int r = 0; r < kPer; ++r) plane[t + kT * r] = x[r];  // (read behind the first barrier of the loop below)
    const int wave = t >> 6, lane = t & 63;
    for (int e0 = 0; e0 < d.count; e0 += kBatch) {
        const int nb = d.count - e0 < kBatch ? d.count - e0 : kBatch;
        // the four scans side by side, so that the region bytes of four entries are in flight together (a batch of fewer entries
        // scans its last one again and stores it nowhere)
        const unsigned char *mk[kBatch];
        int prev[kBatch], radius[kBatch], op[kBatch];
        TrackBest best[kBatch];
#pragma unroll
        for (int b = 0; b < kBatch; ++b) {
            const TrackTapeItem it = items[d.first + e0 + (b < nb ? b : nb - 1)];
            mk[b] = masks + static_cast<long>(it.region) * NG + t;
            radius[b] = it.radius;
            op[b] = it.op;
            prev[b] = it.radius > 0 ? load_global(last + i * n_entries + it.column) : -1;
            best[b] = TrackBest{0.0, -1};
        }
#pragma unroll
        for (int r = 0; r < kPer; ++r) {
#pragma unroll
            for (int b = 0; b < kBatch; ++b)
                if (track_candidate(x[r], load_global(mk[b] + kT * r), t + kT * r, prev[b], radius[b])) track_take(best[b], x[r], t + kT * r, op[b]);
        }
#pragma unroll
        for (int b = 0; b < kBatch; ++b) {
            tree_v[b][t] = best[b].v;
            tree_p[b][t] = best[b].p;
        }
        __syncthreads();
        if (wave < nb) {
            const TrackTapeItem mine = items[d.first + e0 + wave];
            const double *tv = tree_v[wave];
            const int *tp = tree_p[wave];
            TrackBest v = track_merge(track_merge(TrackBest{tv[lane], tp[lane]}, TrackBest{tv[lane + 128], tp[lane + 128]}, mine.op),
                                      track_merge(TrackBest{tv[lane + 64], tp[lane + 64]}, TrackBest{tv[lane + 192], tp[lane + 192]}, mine.op), mine.op);
#pragma unroll
            for (int half = 32; half > 0; half >>= 1) {
                const TrackBest other{__shfl_down(v.v, half, 64), __shfl_down(v.p, half, 64)};
                v = track_merge(v, other, mine.op);
            }
            if (lane == 0) {
                const TrackResult got = track_finish(plane, v);
                double *dst = ring_slot + (i * n_entries + mine.column) * 4;
                double2v lo, hi;
                lo.x = got.value;
                lo.y = got.p;
                hi.x = got.di;
                hi.y = got.dj;
                store_pair(dst, lo);
                store_pair(dst + 2, hi);
                store_global(last + i * n_entries + mine.column, v.p);
            }
        }
        __syncthreads();  // (the next batch overwrites the rows)
    }
}
}  // namespace

hipError_t run_tracktape_sample(const TrackTapePlane *planes, int nplanes, const TrackTapeItem *items, const unsigned char *masks,
                                const double *slab, int slab_fields, double *ring_slot, int *last, int n_entries, int first, int count,
                                int store32, hipStream_t s) {
    if (nplanes == 0 || count == 0) return hipSuccess;
    hipLaunchKernelGGL(tracktape_kernel, dim3(nplanes, count), dim3(kT), 0, s, planes, items, masks, slab, slab_fields, ring_slot, last,
                       n_entries, first, store32);
    return hipGetLastError();
}

}  // namespace spd

// ---- host side: the step loop's sample, the configuration and the C ABI (spd_model_tracktape_*) ----

namespace {
const char *const kTrackOff = "no track tape configured (spd_model_tracktape_configure)";

// every entry of every member follows nothing; the device is idle before and after
hipError_t unseed(const spd_model *m, const spd_model::TrackTape &tt) {
    hipError_t e = hipMemset(tt.last, 0xFF, static_cast<size_t>(m->M) * tt.entries.size() * sizeof(int));
    if (e == hipSuccess) e = hipDeviceSynchronize();
    return e;
}

// a call that reads or writes the follow-state of the members [first, first + count) between the model's calls
int follow_call_allowed(spd_model *m, const char *who, int first, int count) {
    if (!m) return m_fail(SPD_E_ARG, std::string(who) + ": null model");
    if (int rc = usable(m, who)) return rc;
    if (!m->tracktape.on) return m_fail(SPD_E_ARG, std::string(who) + ": " + kTrackOff);
    if (m->steps_pending) return m_fail(SPD_E_ARG, std::string(who) + ": a checked multi-step call is in flight; end it first");
    if (first < 0 || count < 0 || first + count > m->M) return m_fail(SPD_E_ARG, std::string(who) + ": member range out of bounds");
    return SPD_OK;
}
}  // namespace

// the sample of members [first, first + count): the front end into the recorder's own slab, then every entry's winner into ring
// slot (n - 1) % capacity and into the follow-state
hipError_t spd::tracktape_sample(spd_model *m, int first, int count, long long n, hipStream_t s) {
    const spd_model::TrackTape &tt = m->tracktape;
    const size_t per_slot = static_cast<size_t>(m->M) * tt.entries.size() * 4;
    hipError_t e = sample_front(m, tt, first, count, s);
    if (e == hipSuccess)
        e = run_tracktape_sample(tt.planes, tt.nplanes, tt.items, tt.masks, tt.slab, tt.slab_fields,
                                 tt.data + static_cast<size_t>(tt.ring.slot(n)) * per_slot, tt.last, static_cast<int>(tt.entries.size()), first,
                                 count, m->stored32 ? 1 : 0, s);
    return e;
}

hipError_t spd::tracktape_unseed(spd_model *m) {
    if (!m->tracktape.on) return hipSuccess;
    return unseed(m, m->tracktape);
}

extern "C" {

int spd_track_point_host(const double *plane, const unsigned char *mask, int prev, int radius, int op, double *out4) {
    const char *who = "spd_track_point_host";
    if (!plane || !mask || !out4) return m_fail(SPD_E_ARG, std::string(who) + ": null argument");
    if (prev < -1 || prev >= kTrackPoints) return m_fail(SPD_E_ARG, std::string(who) + ": prev must be -1 or 0 ... 4607, got " + std::to_string(prev));
    if (radius < 0 || radius > kTrackMaxRadius)
        return m_fail(SPD_E_ARG, std::string(who) + ": radius must be 0 ... " + std::to_string(kTrackMaxRadius) + ", got " + std::to_string(radius));
    if (op != SPD_TRACK_MIN && op != SPD_TRACK_MAX) return m_fail(SPD_E_ARG, std::string(who) + ": op must be SPD_TRACK_MIN or SPD_TRACK_MAX, got " + std::to_string(op));
    track_point_host(plane, mask, prev, radius, op, out4);
    return SPD_OK;
}

int spd_model_tracktape_configure(spd_model_handle m, const double *regions, int n_regions, const char *const *names, const int *levels,
                                  const int *region_of, const int *ops, const int *radii, int n_entries, int every, int capacity) {
    const char *who = "spd_model_tracktape_configure";
    // (the arguments first, in the header's order: nothing in this block needs the device or a model; n_entries = 0 is "off")
    std::vector<spd_model::TrackTape::Entry> entries;
    std::vector<unsigned char> host_masks;
    if (n_entries != 0) {
        if (every < 1) return m_fail(SPD_E_ARG, std::string(who) + ": every must be at least 1");
        if (capacity < 1) return m_fail(SPD_E_ARG, std::string(who) + ": capacity must be at least 1");
        if (n_regions < 1 || n_regions > kTrackMaxRegions)
            return m_fail(SPD_E_ARG, std::string(who) + ": n_regions must be 1 ... " + std::to_string(kTrackMaxRegions) + ", got " +
                                         std::to_string(n_regions));
        if (n_entries < 0 || n_entries > kTrackMaxEntries)
            return m_fail(SPD_E_ARG, std::string(who) + ": n_entries must be 0 ... " + std::to_string(kTrackMaxEntries) + ", got " +
                                         std::to_string(n_entries));
        if (!regions) return m_fail(SPD_E_ARG, std::string(who) + ": null regions");
        if (!names || !levels || !region_of || !ops || !radii) return m_fail(SPD_E_ARG, std::string(who) + ": bad list of entries");
        if (int rc = check_weight_maps(who, regions, n_regions)) return rc;
        host_masks.resize(static_cast<size_t>(n_regions) * NG);
        for (int r = 0; r < n_regions; ++r) {
            int points = 0;
            for (int q = 0; q < NG; ++q) {
                const bool inside = regions[static_cast<size_t>(r) * NG + q] != 0.0;
                host_masks[static_cast<size_t>(r) * NG + q] = inside ? 1 : 0;
                points += inside ? 1 : 0;
            }
            if (points == 0) return m_fail(SPD_E_ARG, std::string(who) + ": region " + std::to_string(r) + " holds no point (every weight is zero)");
        }
        for (int k = 0; k < n_entries; ++k) {
            const int id = entry_id(who, names[k], SPD_CATALOGUE_LIST);
            if (id < 0) return SPD_E_ARG;
            entries.push_back({id, levels[k], region_of[k], ops[k], radii[k]});
        }
        for (int k = 0; k < n_entries; ++k) {
            if (int rc = check_entry_level(who, k, names[k], entries[k].name, levels[k])) return rc;
            if (int rc = check_entry_pattern(who, k, names[k], region_of[k], n_regions)) return rc;
            if (ops[k] != SPD_TRACK_MIN && ops[k] != SPD_TRACK_MAX)
                return m_fail(SPD_E_ARG, std::string(who) + ": op " + std::to_string(ops[k]) + " of " + entry_text(k, names[k]) +
                                             " is not SPD_TRACK_MIN (0) or SPD_TRACK_MAX (1)");
            if (radii[k] < 0 || radii[k] > kTrackMaxRadius)
                return m_fail(SPD_E_ARG, std::string(who) + ": radius " + std::to_string(radii[k]) + " of " + entry_text(k, names[k]) +
                                             " is out of range (0 ... " + std::to_string(kTrackMaxRadius) + ")");
        }
    }
    if (int rc = configure_allowed(m, who)) return rc;
    if (int rc = check_plev_entries(m, who, names, entries)) return rc;
    spd_model::TrackTape &tt = m->tracktape;
    if (int rc = retire(m, tt)) return rc;
    if (n_entries == 0) return SPD_OK;  // off
    spd_model::TrackTape next;
    next.every = every;
    next.nregions = n_regions;
    const size_t M = static_cast<size_t>(m->M), slots = static_cast<size_t>(capacity), E = static_cast<size_t>(n_entries);
    // the sample plan over the names among the entries (the front end transforms a name's every level), and the entries sorted by
    // distinct plane (stable: the caller's order within a plane)
    const EntryPlanes table = entry_planes(entries);
    SamplePlan plan;
    plan_sample(m, table.ids, next, plan);
    // one allocation: ring | regions | last | slab | tables[2] | plane descriptors | entry list
    const size_t per_slot = M * E * 4 * sizeof(double);
    if (slots > (static_cast<size_t>(-1) / 2) / per_slot) return m_fail(SPD_E_ARG, std::string(who) + ": the size of the series does not fit size_t");
    const size_t ring = sample_up(slots * per_slot), maps = sample_up(host_masks.size()), follow = sample_up(M * E * sizeof(int));
    const size_t desc = sample_up(table.distinct.size() * sizeof(TrackTapePlane)), list = sample_up(E * sizeof(TrackTapeItem));
    const size_t total = ring + maps + follow + plan.slab_bytes + 2 * plan.table_bytes + desc + list;
    void *p = nullptr;
    if (hipMalloc(&p, total) != hipSuccess) {  // the track tape is off; the model is as usable as before
        (void)hipGetLastError();
        return m_fail(SPD_E_DEVICE, std::string(who) + ": cannot allocate the track tape (" + std::to_string(total) + " bytes asked for: " +
                                        std::to_string(capacity) + " samples of " + std::to_string(per_slot) + " bytes); the track tape is off");
    }
    Carve carve{static_cast<char *>(p)};
    next.alloc = p;
    next.data = carve.take<double>(ring);
    next.masks = carve.take<unsigned char>(maps);
    next.last = carve.take<int>(follow);
    carve_front(carve, plan, next);
    next.planes = carve.take<TrackTapePlane>(desc);
    next.items = carve.take<TrackTapeItem>(list);
    std::vector<SampleSource> sources;  // (per plane of plan.vars, in their order)
    hipError_t e = build_sample_front(m, plan, next, sources);
    std::vector<TrackTapePlane> host_planes;
    std::vector<TrackTapeItem> host_items;
    for (size_t q = 0; q < table.distinct.size(); ++q) {
        TrackTapePlane d{};
        d.source = plane_source(plan, sources, table.distinct[q].first, table.distinct[q].second);
        d.first = static_cast<int>(host_items.size());
        table.each_entry_of(q, [&](int k) { host_items.push_back({entries[k].region, k, entries[k].op, entries[k].radius}); });
        d.count = static_cast<int>(host_items.size()) - d.first;
        host_planes.push_back(d);
    }
    next.entries = std::move(entries);
    if (e == hipSuccess) e = hipMemcpy(next.masks, host_masks.data(), host_masks.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(next.planes, host_planes.data(), host_planes.size() * sizeof(TrackTapePlane), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(next.items, host_items.data(), host_items.size() * sizeof(TrackTapeItem), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = unseed(m, next);
    if (e != hipSuccess) return upload_failed(who, e, p);
    next.nplanes = static_cast<int>(host_planes.size());
    next.host_masks = std::move(host_masks);
    next.ring = SampleRing(capacity, 6);
    next.on = true;
    tt = std::move(next);
    return SPD_OK;
}

int spd_model_tracktape_reset(spd_model_handle m) {
    const char *who = "spd_model_tracktape_reset";
    if (int rc = ring_reset(m, who, &spd_model::tracktape, kTrackOff)) return rc;
    M_HIP(hipSetDevice(m->ctx->device));
    M_HIP(hipDeviceSynchronize());  // (samples in flight still write the follow-state)
    M_HIP(unseed(m, m->tracktape));
    return SPD_OK;
}

int spd_model_tracktape_info(spd_model_handle m, long long *taken, int *held, int *capacity, int *every, int *n_regions, int *n_entries) {
    if (!m) return m_fail(SPD_E_ARG, "spd_model_tracktape_info: null model");
    const spd_model::TrackTape &tt = m->tracktape;
    if (!tt.on) return m_fail(SPD_E_ARG, std::string("spd_model_tracktape_info: ") + kTrackOff);
    if (taken) *taken = tt.ring.taken;
    if (held) *held = static_cast<int>(tt.ring.held());
    if (capacity) *capacity = tt.ring.capacity;
    if (every) *every = tt.every;
    if (n_regions) *n_regions = tt.nregions;
    if (n_entries) *n_entries = static_cast<int>(tt.entries.size());
    return SPD_OK;
}

int spd_model_tracktape_times(spd_model_handle m, int32_t *rows, int max_rows) {
    return ring_rows(m, "spd_model_tracktape_times", &spd_model::tracktape, kTrackOff, rows, max_rows);
}

int spd_model_tracktape_read(spd_model_handle m, int first, int count, int t0, int nt, void *dst_device, size_t dst_bytes, void *stream) {
    const char *who = "spd_model_tracktape_read";
    if (!m) return m_fail(SPD_E_ARG, std::string(who) + ": null model");
    const spd_model::TrackTape &tt = m->tracktape;
    if (int rc = read_allowed(m, who, tt.on, kTrackOff, tt.validity, "the track tape is invalid until spd_model_tracktape_reset")) return rc;
    if (first < 0 || count < 0 || first + count > m->M) return m_fail(SPD_E_ARG, std::string(who) + ": member range out of bounds");
    if (int rc = held_range(who, tt.ring, t0, nt, "sample")) return rc;
    const size_t per = tt.entries.size() * 4;
    const size_t need = static_cast<size_t>(count) * static_cast<size_t>(nt) * per * sizeof(double);
    if (int rc = destination_fits(who, dst_device, dst_bytes, need, sizeof(double))) return rc;
    // (the ring is [slot][M][E * 4] as a spectra ring is [slot][M][per]: the same gather)
    return gather_slots(m, who, tt.data + static_cast<size_t>(first) * per, per, static_cast<size_t>(m->M) * per, count, t0, nt, tt.ring, dst_device, stream);
}

int spd_model_tracktape_positions(spd_model_handle m, int first, int count, int32_t *dst, int max) {
    const char *who = "spd_model_tracktape_positions";
    if (int rc = follow_call_allowed(m, who, first, count)) return rc;
    const size_t E = m->tracktape.entries.size(), n = static_cast<size_t>(count) * E;
    if (max < 0 || (n > 0 && !dst)) return m_fail(SPD_E_ARG, std::string(who) + ": bad destination");
    if (static_cast<size_t>(max) < n) return m_fail(SPD_E_SIZE, std::string(who) + ": destination too small (" + std::to_string(n) + " values needed)");
    if (n == 0) return 0;
    M_HIP(hipSetDevice(m->ctx->device));
    M_HIP(hipDeviceSynchronize());  // (samples in flight still write the follow-state)
    M_HIP(hipMemcpy(dst, m->tracktape.last + static_cast<size_t>(first) * E, n * sizeof(int32_t), hipMemcpyDeviceToHost));
    return static_cast<int>(n);
}

int spd_model_tracktape_seed(spd_model_handle m, int first, int count, const int32_t *src) {
    const char *who = "spd_model_tracktape_seed";
    if (int rc = follow_call_allowed(m, who, first, count)) return rc;
    const spd_model::TrackTape &tt = m->tracktape;
    const size_t E = tt.entries.size(), n = static_cast<size_t>(count) * E;
    if (n > 0 && !src) return m_fail(SPD_E_ARG, std::string(who) + ": null source");
    for (size_t at = 0; at < n; ++at) {
        const int q = src[at], k = static_cast<int>(at % E), member = first + static_cast<int>(at / E);
        if (q == -1) continue;
        if (q < -1 || q >= NG)
            return m_fail(SPD_E_ARG, std::string(who) + ": the seed of member " + std::to_string(member) + ", entry " + std::to_string(k) + " (" +
                                         std::to_string(q) + ") is not -1 or 0 ... " + std::to_string(NG - 1));
        if (!tt.host_masks[static_cast<size_t>(tt.entries[k].region) * NG + q])
            return m_fail(SPD_E_ARG, std::string(who) + ": the seed of member " + std::to_string(member) + ", entry " + std::to_string(k) + " (point " +
                                         std::to_string(q) + ": row " + std::to_string(q / IX) + ", column " + std::to_string(q % IX) +
                                         ") lies outside region " + std::to_string(tt.entries[k].region));
    }
    if (n == 0) return SPD_OK;
    M_HIP(hipSetDevice(m->ctx->device));
    M_HIP(hipDeviceSynchronize());  // (samples in flight still read and write the follow-state)
    M_HIP(hipMemcpy(tt.last + static_cast<size_t>(first) * E, src, n * sizeof(int32_t), hipMemcpyHostToDevice));
    M_HIP(hipDeviceSynchronize());
    return SPD_OK;
}

}  // extern "C"
