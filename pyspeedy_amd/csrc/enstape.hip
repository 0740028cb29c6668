// Ensemble mean and spread recorded on the GPU inside multi-step calls (spd_model_enstape_*, include/pyspeedy_amd.h).
//
// A sample is what the tape samples (tape.hip): model.hip runs the same front end into a slab of the ensemble tape's own, and the
// fold kernel below reads what tape_store_kernel reads -- the slab's planes, precnv / precls where the column kernel stores them,
// in their stored precision -- applies the same export_unit and, instead of writing every member's value, folds the members of the
// launch in member order into one partial (mean, M2) with Welford's update.  The value of member j that enters is therefore exactly
// what an fp64 tape holds for it; the reduction is the only new arithmetic.  One partial per group stream and slot (enstape.hpp):
// the mean and M2 that come out depend on the launch plan at round-off level and on nothing else.
// Two points (16 bytes of fp64) per lane, coalesced over the 4608 points of a plane.  No LDS, no atomics, no scratch.
#include <hip/hip_runtime.h>

#include <cmath>

#include "enstape.hpp"
#include "global_mem.hpp"
#include "model_state.hpp"
#include "tables.hpp"

namespace spd {

namespace {
constexpr int kT = 256;
constexpr int kPairs = NG / 2;  // 2304 = 9 blocks of 256 lanes: no partial block
static_assert(NG % 2 == 0 && kPairs % kT == 0, "a plane is a whole number of blocks of point pairs");
// Members whose loads are issued before the first of them is folded.  The walk over the members is a chain (each update needs
// the mean before it), and a launch is a few dozen workgroups on 256 compute units: nothing else hides a load's latency, so without
// batches the walk costs one memory round trip per member.  8 members are 8 x 16 bytes in flight per lane and 32 VGPRs; a group of
// the default plan at 64 members (32 members) is four round trips.
constexpr int kBatch = 8;

// The walk: members j = 0 ... count - 1 at base + j * stride, kBatch loads ahead of the first update.  A batch past the last member
// loads that member again instead of branching around the load (a branch per load would wait for each one on its own).
template <typename T>
__device__ __forceinline__ void fold_members(const T *base, long stride, int count, int unit, int n0, double2v &mean, double2v &m2) {
    for (int j0 = 0; j0 < count; j0 += kBatch) {
        double2v x[kBatch];
#pragma unroll
        for (int b = 0; b < kBatch; ++b) {
            const int j = j0 + b < count ? j0 + b : count - 1;
            x[b] = widen(stream_load_pair(base + j * stride));
        }
#pragma unroll
        for (int b = 0; b < kBatch; ++b) {
            if (j0 + b < count) {  // Welford's update with member j0 + b as the n-th value of the partial
                const double n = static_cast<double>(n0 + j0 + b + 1);
                const double vx = export_unit(x[b].x, unit), vy = export_unit(x[b].y, unit);
                const double dx = vx - mean.x, dy = vy - mean.y;
                mean.x += dx / n;
                mean.y += dy / n;
                m2.x += dx * (vx - mean.x);
                m2.y += dy * (vy - mean.y);
            }
        }
    }
}

// blockIdx.x: pairs of points, blockIdx.y: plane
__global__ __launch_bounds__(kT) void enstape_fold_kernel(const EnsTapePlane *__restrict__ planes, int nplanes,
                                                          const double *__restrict__ slab, int slab_fields, int first, int count,
                                                          int partial, int n0, int store32) {
    const int p = 2 * (blockIdx.x * kT + threadIdx.x);
    if (p >= NG) return;
    const EnsTapePlane d = planes[blockIdx.y];
    const long at = static_cast<long>(partial) * nplanes * NG + p;
    double2v mean = {0.0, 0.0}, m2 = {0.0, 0.0};
    if (n0 > 0) {  // (the first members of a sample's partial: nothing of it is read -- a lap over the ring needs no device work)
        mean = load_pair(d.mean + at);
        m2 = load_pair(d.m2 + at);
    }
    with_sample_plane(d.source, slab, slab_fields, store32, first, [=](auto plane, long stride, double2v &mean, double2v &m2) {
        fold_members(plane + p, stride, count, d.source.unit, n0, mean, m2);
    }, mean, m2);
    // (plain stores: a later round of the same sample reads the partial back, and so does the read)
    store_pair(d.mean + at, mean);
    store_pair(d.m2 + at, m2);
}

// blockIdx.x: pairs of points of the variable's planes, blockIdx.y: sample of this launch
__global__ __launch_bounds__(kT) void enstape_read_kernel(const double *__restrict__ mean, const double *__restrict__ m2, long per,
                                                          long partial_stride, int kind, int slot0, int capacity, EnsTapeCounts counts,
                                                          double *__restrict__ dst) {
    const long q = 2 * (static_cast<long>(blockIdx.x) * kT + threadIdx.x);
    if (q >= per) return;
    const int t = blockIdx.y;
    const long slot = (slot0 + static_cast<long>(t)) % capacity;
    double2v mu = {0.0, 0.0}, s = {0.0, 0.0};
    double na = 0.0;
    for (int g = 0; g < kEnsTapeGroups; ++g) {  // Chan's merge of the partials that hold members, in the fixed order g = 0 ... 3
        const int c = counts.n[t][g];
        if (c == 0) continue;
        const long at = (slot * kEnsTapeGroups + g) * partial_stride + q;
        const double2v mb = *reinterpret_cast<const double2v *>(mean + at), sb = *reinterpret_cast<const double2v *>(m2 + at);
        const double nb = static_cast<double>(c);
        if (na == 0.0) {
            mu = mb;
            s = sb;
            na = nb;
            continue;
        }
        const double n = na + nb, w = nb / n, ww = na * nb / n;
        const double dx = mb.x - mu.x, dy = mb.y - mu.y;
        mu.x = mu.x + dx * w;
        mu.y = mu.y + dy * w;
        s.x = (s.x + sb.x) + (dx * dx) * ww;
        s.y = (s.y + sb.y) + (dy * dy) * ww;
        na = n;
    }
    double2v out;
    if (kind == 0) {
        out = mu;
    } else if (kind == 2) {
        out = s;
    } else {  // the unbiased standard deviation (one member: 0 / 0, NaN, as stats_ensemble_kernel)
        out.x = sqrt(s.x / (na - 1.0));
        out.y = sqrt(s.y / (na - 1.0));
    }
    *reinterpret_cast<double2v *>(dst + static_cast<long>(t) * per + q) = out;
}
}  // namespace

// Fold the sample of the members [first, first + count), in member order, into the partial `partial` (= slot * 4 + group) of every
// plane: one launch.  n0: members the partial already holds (0: nothing of it is read).  slab: [M][slab_fields][4608] fp64;
// store32: the physics outputs are stored as fp32.
static hipError_t run_enstape_fold(const EnsTapePlane *planes, int nplanes, const double *slab, int slab_fields, int first, int count,
                                   int partial, int n0, int store32, hipStream_t s) {
    if (nplanes == 0 || count == 0) return hipSuccess;
    hipLaunchKernelGGL(enstape_fold_kernel, dim3(kPairs / kT, nplanes), dim3(kT), 0, s, planes, nplanes, slab, slab_fields, first, count,
                       partial, n0, store32);
    return hipGetLastError();
}

// Merge the partials of the samples [0, nt) of one variable (sample t of the read lies in slot (slot0 + t) % capacity; counts: per
// sample and group, in the read's order) into dst[nt][per] doubles (per = levels * 4608): kind 0 the mean, 1 the unbiased standard
// deviation sqrt(M2 / (n - 1)) (one member: NaN), 2 M2.  mean / m2: the variable's first plane in partial (slot 0, group 0);
// nplanes: planes of all variables (the stride between partials is nplanes * 4608 doubles).
static hipError_t run_enstape_read(const double *mean, const double *m2, long per, int nplanes, int kind, int nt, int slot0, int capacity,
                                   const int *counts, double *dst, hipStream_t s) {
    if (nt == 0 || per == 0) return hipSuccess;
    const long pairs = per / 2;  // (a plane is 4608 points: `per` is even)
    for (int t_base = 0; t_base < nt; t_base += kEnsTapeReadSamples) {  // (the counts of a launch travel by value: a long read goes out in pieces)
        const int ny = nt - t_base < kEnsTapeReadSamples ? nt - t_base : kEnsTapeReadSamples;
        EnsTapeCounts c{};
        for (int t = 0; t < ny; ++t)
            for (int g = 0; g < kEnsTapeGroups; ++g) c.n[t][g] = counts[static_cast<size_t>(t_base + t) * kEnsTapeGroups + g];
        hipLaunchKernelGGL(enstape_read_kernel, dim3(static_cast<unsigned>((pairs + kT - 1) / kT), ny), dim3(kT), 0, s, mean, m2, per,
                           static_cast<long>(nplanes) * NG, kind, (slot0 + t_base) % capacity, capacity, c, dst + static_cast<long>(t_base) * per);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace spd

// ---- host side: the step loop's sample, the configuration and the C ABI (spd_model_enstape_*) ----

// the sample of members [first, first + count): the front end into its own slab, then the fold of these members into partial `group` of ring slot
// (n - 1) % capacity, behind the members the partial already holds (rounds: the same stream, one after the other)
hipError_t spd::enstape_sample(spd_model *m, int first, int count, long long n, int group, hipStream_t s) {
    spd_model::EnsTape &et = m->enstape;
    const int slot = et.ring.slot(n);
    int &held = et.counts[static_cast<size_t>(slot) * kEnsTapeGroups + group];
    hipError_t e = sample_front(m, et, first, count, s);
    if (e == hipSuccess)
        e = run_enstape_fold(et.planes, et.nplanes, et.slab, et.slab_fields, first, count, slot * kEnsTapeGroups + group, held,
                             m->stored32 ? 1 : 0, s);
    if (e == hipSuccess) held += count;
    return e;
}

extern "C" {

int spd_model_enstape_configure(spd_model_handle m, const char *const *names, int n_names, int every, int capacity) {
    const char *who = "spd_model_enstape_configure";
    // (the arguments first: nothing below needs the device)
    std::vector<int> ids;
    if (int rc = sample_ids(who, names, n_names, ids)) return rc;
    if (n_names > 0 && every < 1) return m_fail(SPD_E_ARG, std::string(who) + ": every must be at least 1");
    if (n_names > 0 && capacity < 1) return m_fail(SPD_E_ARG, std::string(who) + ": capacity must be at least 1");
    if (int rc = configure_allowed(m, who)) return rc;
    for (size_t k = 0; k < ids.size(); ++k)
        if (cat_needs_levels(ids[k]) && m->plev.n == 0)
            return levels_first(who, names[k]);
    spd_model::EnsTape &et = m->enstape;
    if (int rc = retire(m, et)) return rc;
    if (n_names == 0) return SPD_OK;  // off
    spd_model::EnsTape next;
    next.every = every;
    SamplePlan plan;
    plan_sample(m, ids, next, plan);
    const size_t slots = static_cast<size_t>(capacity);
    for (const auto &v : plan.vars) next.vars.push_back({v.id, v.levels, v.first_plane});
    next.nplanes = static_cast<int>(plan.planes);
    // one allocation: mean ring | M2 ring | slab | tables[2] | plane descriptors
    const size_t per_slot = kEnsTapeGroups * plan.planes * NG * sizeof(double);  // of ONE of the two rings
    if (per_slot != 0 && slots > (static_cast<size_t>(-1) / 4) / per_slot)
        return m_fail(SPD_E_ARG, std::string(who) + ": the ensemble tape's size does not fit size_t");
    const size_t ring = sample_up(slots * per_slot), desc = sample_up(plan.planes * sizeof(EnsTapePlane));
    const size_t total = 2 * ring + plan.slab_bytes + 2 * plan.table_bytes + desc;
    void *p = nullptr;
    if (hipMalloc(&p, total) != hipSuccess) {  // the ensemble tape is off; the model is as usable as before
        (void)hipGetLastError();
        return m_fail(SPD_E_DEVICE, std::string(who) + ": cannot allocate the ensemble tape (" + std::to_string(total) + " bytes asked for: " +
                                        std::to_string(capacity) + " samples of " + std::to_string(2 * per_slot) +
                                        " bytes); the ensemble tape is off");
    }
    Carve carve{static_cast<char *>(p)};
    next.alloc = p;
    next.mean = carve.take<double>(ring);
    next.m2 = carve.take<double>(ring);
    carve_front(carve, plan, next);
    next.planes = carve.take<EnsTapePlane>(desc);
    std::vector<SampleSource> sources;
    hipError_t e = build_sample_front(m, plan, next, sources);
    std::vector<EnsTapePlane> host_planes;
    for (const auto &v : next.vars)
        for (int k = 0; k < v.levels; ++k) {
            EnsTapePlane d{};
            d.source = sources[host_planes.size()];
            d.mean = next.mean + (v.first_plane + static_cast<size_t>(k)) * NG;
            d.m2 = next.m2 + (v.first_plane + static_cast<size_t>(k)) * NG;
            host_planes.push_back(d);
        }
    if (e == hipSuccess) e = hipMemcpy(next.planes, host_planes.data(), host_planes.size() * sizeof(EnsTapePlane), hipMemcpyHostToDevice);
    if (e != hipSuccess) return upload_failed(who, e, p);
    next.ring = SampleRing(capacity, 6);
    next.counts.assign(slots * kEnsTapeGroups, 0);
    next.on = true;
    et = std::move(next);
    return SPD_OK;
}

int spd_model_enstape_reset(spd_model_handle m) {
    return ring_reset(m, "spd_model_enstape_reset", &spd_model::enstape, "no ensemble tape configured (spd_model_enstape_configure)");
}

int spd_model_enstape_info(spd_model_handle m, long long *taken, int *held, int *capacity, int *every, int *members) {
    if (!m) return m_fail(SPD_E_ARG, "spd_model_enstape_info: null model");
    const spd_model::EnsTape &et = m->enstape;
    if (!et.on) return m_fail(SPD_E_ARG, "spd_model_enstape_info: no ensemble tape configured (spd_model_enstape_configure)");
    if (taken) *taken = et.ring.taken;
    if (held) *held = static_cast<int>(et.ring.held());
    if (capacity) *capacity = et.ring.capacity;
    if (every) *every = et.every;
    if (members) *members = m->M;
    return SPD_OK;
}

int spd_model_enstape_times(spd_model_handle m, int32_t *rows, int max_rows) {
    return ring_rows(m, "spd_model_enstape_times", &spd_model::enstape, "no ensemble tape configured (spd_model_enstape_configure)", rows, max_rows);
}

int spd_model_enstape_read(spd_model_handle m, const char *name, int kind, int t0, int nt, void *dst_device, size_t dst_bytes, void *stream) {
    const char *who = "spd_model_enstape_read";
    if (!m || !name) return m_fail(SPD_E_ARG, std::string(who) + ": null argument");
    const spd_model::EnsTape &et = m->enstape;
    if (int rc = read_allowed(m, who, et.on, "no ensemble tape configured (spd_model_enstape_configure)", et.validity,
                              "the ensemble tape is invalid until spd_model_enstape_reset"))
        return rc;
    const int id = stats_id(name);
    const spd_model::EnsTape::Var *v = nullptr;
    for (const auto &x : et.vars)
        if (x.id == id) v = &x;
    if (!v) return m_fail(SPD_E_ARG, std::string(who) + ": '" + name + "' is not among the configured variables");
    if (kind != SPD_ENS_MEAN && kind != SPD_ENS_STD && kind != SPD_ENS_M2)
        return m_fail(SPD_E_ARG, std::string(who) + ": kind must be SPD_ENS_MEAN, SPD_ENS_STD or SPD_ENS_M2");
    if (int rc = held_range(who, et.ring, t0, nt, "sample")) return rc;
    const size_t per = static_cast<size_t>(v->levels) * NG, need = static_cast<size_t>(nt) * per * sizeof(double);
    if (int rc = destination_fits(who, dst_device, dst_bytes, need, 16)) return rc;
    if (nt == 0) return SPD_OK;
    M_HIP(hipSetDevice(m->ctx->device));
    const int slot0 = et.ring.slot_of_held(t0);
    std::vector<int> counts(static_cast<size_t>(nt) * kEnsTapeGroups);  // of the samples of the read, in its order
    for (int t = 0; t < nt; ++t)
        std::memcpy(counts.data() + static_cast<size_t>(t) * kEnsTapeGroups,
                    et.counts.data() + static_cast<size_t>(et.ring.slot_of_held(t0 + static_cast<long long>(t))) * kEnsTapeGroups,
                    kEnsTapeGroups * sizeof(int));
    const size_t var_at = v->first_plane * NG;
    const hipError_t e = run_enstape_read(et.mean + var_at, et.m2 + var_at, static_cast<long>(per), et.nplanes, kind, nt, slot0, et.ring.capacity,
                                          counts.data(), static_cast<double *>(dst_device), static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return m_fail(SPD_E_DEVICE, std::string(who) + ": " + hipGetErrorString(e));
    return SPD_OK;
}

}  // extern "C"
