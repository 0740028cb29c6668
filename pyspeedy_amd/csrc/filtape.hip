// Window means, covariances and last values of time-filtered grid-space fields, formed on the GPU behind the sampled steps of a
// multi-step call (spd_model_filtape_*, include/pyspeedy_amd.h; the definition is in filtape.hpp, the rule for one point in
// filter_point.hpp, and DESIGN section 4q).
//
// A sample is what an fp64 tape of the same name holds: model.hip runs the tape's front end into a slab of the recorder's own, and
// the filter kernel applies export_unit (sample_source.hpp) exactly as tape_store_kernel does; precnv / precls are read where the
// column kernel stores them, in their stored precision, widened.  Two launches per sampled step and member group:
//   1. filtape_filter_kernel, one lane per two points of one filtered plane -- a (name, level, filter) among the entries -- of one
//      member: it loads x, steps the cascade's sections with their state (two planes per section) and leaves y in a scratch plane.
//      Whether the sample is filter sample 1 comes by value: the sections then start in the steady state of a constant input and
//      read no state, so a reset or a reconfiguration needs no device work.
//   2. filtape_accumulate_kernel, one lane per two points of one entry of one member: it reads y_a (and y_b of a covariance),
//      updates the entry's one accumulator and, at a close, writes the window's result into the ring slot.  The sample's counted
//      number within its window comes by value: 1 overwrites the accumulator and reads none; 0 means that the launch only closes.
// A sample of the spin-up issues the first launch alone, a step that only closes the second alone.  The arithmetic is fixed -- every
// operation of the filter rounded on its own (filter_point.hpp), the product of a covariance one multiplication, the sum in sample
// order from the first counted value itself, the mean one division -- so the result does not depend on the launch plan.
// State, y and accumulators are read again at the next sample or by the next launch: ordinary loads and stores.  Ring stores are
// written once and read by the host's gather only: non-temporal.  Two points (16 bytes of fp64) per lane, coalesced over the 4608
// points of a plane; no atomics.
#include <hip/hip_runtime.h>

#include <cmath>

#include "filtape.hpp"
#include "global_mem.hpp"
#include "model_state.hpp"
#include "tables.hpp"

namespace spd {

namespace {
constexpr int kT = 256;
constexpr int kPairs = NG / 2;  // 2304 = 9 blocks of 256 lanes: no partial block
static_assert(NG % 2 == 0 && kPairs % kT == 0, "a plane is a whole number of blocks of point pairs");

// blockIdx.x: pairs of points, blockIdx.y: filtered plane (descriptor), blockIdx.z: member of the group
__global__ __launch_bounds__(kT) void filtape_filter_kernel(const FilTapePlane *__restrict__ planes, const double *__restrict__ slab,
                                                            int slab_fields, double *__restrict__ state, double *__restrict__ y, int nplanes,
                                                            int smax, int first, int first_sample, int store32) {
#pragma clang fp contract(off)
    const int p = 2 * (blockIdx.x * kT + threadIdx.x);
    if (p >= NG) return;
    const FilTapePlane &d = planes[blockIdx.y];
    const long i = first + static_cast<long>(blockIdx.z);
    const long f = i * nplanes + blockIdx.y;
    double2v x = with_sample_plane(d.source, slab, slab_fields, store32 && d.narrow, i, [&](auto plane, long) { return widen(load_pair(plane + p)); });
    x.x = export_unit(x.x, d.source.unit);
    x.y = export_unit(x.y, d.source.unit);
    double *st = state + f * smax * 2 * NG + p;
    const int n = d.n_sections;
#pragma unroll
    for (int s = 0; s < kFilMaxSections; ++s) {
        if (s >= n) break;
        const FilSection c = d.sec[s];
        double a1 = 0.0, a2 = 0.0, b1 = 0.0, b2 = 0.0;  // the state of the two points: (a1, a2) and (b1, b2)
        if (first_sample) {
            x.x = fil_first(c, x.x, a1, a2);
            x.y = fil_first(c, x.y, b1, b2);
        } else {
            const double2v s1 = load_pair(st + (2 * s) * NG), s2 = load_pair(st + (2 * s + 1) * NG);
            a1 = s1.x, b1 = s1.y, a2 = s2.x, b2 = s2.y;
            x.x = fil_next(c, x.x, a1, a2);
            x.y = fil_next(c, x.y, b1, b2);
        }
        double2v s1, s2;
        s1.x = a1, s1.y = b1, s2.x = a2, s2.y = b2;
        store_pair(st + (2 * s) * NG, s1);
        store_pair(st + (2 * s + 1) * NG, s2);
    }
    store_pair(y + f * NG + p, x);
}

// blockIdx.x: pairs of points, blockIdx.y: entry (descriptor), blockIdx.z: member of the group
template <typename T>
__global__ __launch_bounds__(kT) void filtape_accumulate_kernel(const FilTapeItem *__restrict__ items, const double *__restrict__ y,
                                                                double *__restrict__ acc, int nplanes, int nentries, long slot_stride, int first,
                                                                int c, int close, int n, int slot) {
#pragma clang fp contract(off)
    const int p = 2 * (blockIdx.x * kT + threadIdx.x);
    if (p >= NG) return;
    const FilTapeItem d = items[blockIdx.y];
    const long i = first + static_cast<long>(blockIdx.z);
    double2v v = both(0.0);
    if (c > 0) {
        v = load_pair(y + (i * nplanes + d.plane_a) * NG + p);
        if (d.op == kFilCov) {
            const double2v b = d.plane_b != d.plane_a ? load_pair(y + (i * nplanes + d.plane_b) * NG + p) : v;
            v.x = __dmul_rn(v.x, b.x);
            v.y = __dmul_rn(v.y, b.y);
        }
    }
    // the accumulator holds the window's earlier counted samples when there are any: c - 1 of them before this sample, n without
    // one; SPD_FIL_LAST keeps the last value and never adds
    double *at = acc + (i * nentries + blockIdx.y) * NG + p;
    const bool held = d.op == kFilLast ? (c == 0 && n > 0) : (c > 1 || (c == 0 && n > 0));
    double2v a = v;
    if (held) {
        a = load_pair(at);
        if (c > 0) {
            a.x = __dadd_rn(a.x, v.x);
            a.y = __dadd_rn(a.y, v.y);
        }
    }
    if (c > 0 && !close) store_pair(at, a);
    if (close) {
        double2v out = both(__builtin_nan(""));
        if (n > 0) {
            out = a;
            if (d.op != kFilLast) {
                const double cnt = static_cast<double>(n);
                out.x = a.x / cnt;
                out.y = a.y / cnt;
            }
        }
        ring_store<T>(d.ring, static_cast<long>(slot) * slot_stride + i * NG + p, out);
    }
}
}  // namespace

}  // namespace spd

// ---- host side: the decision of a step, the step loop's launches, the argument checks, the configuration and the C ABI ----

namespace {
const char *const kFilOff = "no filter tape configured (spd_model_filtape_configure)";

struct FilPlaneKey {
    int name, level, filter;
    bool operator==(const FilPlaneKey &o) const { return name == o.name && level == o.level && filter == o.filter; }
};
// what the argument checks leave for the configuration
struct FilChecked {
    std::vector<std::vector<FilSection>> filters;
    std::vector<spd_model::FilTape::Entry> entries;
    std::vector<FilPlaneKey> planes;      // the distinct filtered planes in the order they first appear
    std::vector<int> plane_a, plane_b;    // [E]
};

int plane_index(std::vector<FilPlaneKey> &planes, const FilPlaneKey &key) {
    const int at = static_cast<int>(std::find(planes.begin(), planes.end(), key) - planes.begin());  // (before the vector may move)
    if (at == static_cast<int>(planes.size())) planes.push_back(key);
    return at;
}

bool names_b_at(const char *const *names_b, int k) { return names_b && names_b[k] && names_b[k][0] != '\0'; }

// cascades: sections [n][5] -> the sections with their gains, or SPD_E_ARG behind the error text (what: "filter 2, " or "")
int check_sections(const char *who, const std::string &what, const double *sections, int n, std::vector<FilSection> &out) {
    for (int s = 0; s < n; ++s) {
        const double *c = sections + 5 * static_cast<size_t>(s);
        if (!fil_section_finite(c))
            return m_fail(SPD_E_ARG, std::string(who) + ": " + what + "section " + std::to_string(s) + " holds a coefficient that is not finite");
        if (!fil_section_stable(c))
            return m_fail(SPD_E_ARG, std::string(who) + ": " + what + "section " + std::to_string(s) + " is not stable (|a2| < 1 and |a1| < 1 + a2; a1 = " +
                                         std::to_string(c[3]) + ", a2 = " + std::to_string(c[4]) + ")");
        out.push_back(fil_section(c));
    }
    return SPD_OK;
}

// the arguments of _configure in the header's order; nothing here needs a model or the device
int check_arguments(const char *who, const double *sections, const int *n_sections, int n_filters, const char *const *names_a, const int *levels_a,
                    const int *filters, const int *ops, const char *const *names_b, const int *levels_b, int n_entries, int window, int every,
                    int sample_every, int spinup, int capacity, int dtype, FilChecked &out) {
    if (n_filters < 1 || n_filters > kFilMaxFilters)
        return m_fail(SPD_E_ARG, std::string(who) + ": n_filters must be 1 ... " + std::to_string(kFilMaxFilters) + ", got " + std::to_string(n_filters));
    if (!sections || !n_sections) return m_fail(SPD_E_ARG, std::string(who) + ": null filters");
    for (int f = 0; f < n_filters; ++f)
        if (n_sections[f] < 1 || n_sections[f] > kFilMaxSections)
            return m_fail(SPD_E_ARG, std::string(who) + ": filter " + std::to_string(f) + " must have 1 ... " + std::to_string(kFilMaxSections) +
                                         " sections, got " + std::to_string(n_sections[f]));
    size_t at = 0;
    for (int f = 0; f < n_filters; ++f) {
        out.filters.emplace_back();
        if (int rc = check_sections(who, "filter " + std::to_string(f) + ", ", sections + 5 * at, n_sections[f], out.filters.back())) return rc;
        at += static_cast<size_t>(n_sections[f]);
    }
    if (n_entries < 1 || n_entries > kFilMaxEntries)
        return m_fail(SPD_E_ARG, std::string(who) + ": n_entries must be 1 ... " + std::to_string(kFilMaxEntries) + ", got " + std::to_string(n_entries));
    if (!names_a || !levels_a || !filters || !ops) return m_fail(SPD_E_ARG, std::string(who) + ": bad list of entries");
    for (int k = 0; k < n_entries; ++k) {
        const int id = entry_id(who, names_a[k], SPD_CATALOGUE_LIST);
        if (id < 0) return SPD_E_ARG;
        int id_b = -1;
        if (names_b_at(names_b, k) && (id_b = entry_id(who, names_b[k], SPD_CATALOGUE_LIST)) < 0) return SPD_E_ARG;
        out.entries.push_back({id, levels_a[k], filters[k], ops[k], id_b, id_b >= 0 && levels_b ? levels_b[k] : 0});
    }
    for (int k = 0; k < n_entries; ++k) {
        const spd_model::FilTape::Entry &e = out.entries[k];
        if (int rc = check_entry_level(who, k, names_a[k], e.name, e.level)) return rc;
        if (e.name_b >= 0)
            if (int rc = check_entry_level(who, k, names_b[k], e.name_b, e.level_b)) return rc;
        if (e.filter < 0 || e.filter >= n_filters)
            return m_fail(SPD_E_ARG, std::string(who) + ": filter " + std::to_string(e.filter) + " of " + entry_text(k, names_a[k]) +
                                         " is out of range (0 ... " + std::to_string(n_filters - 1) + ")");
        if (e.op != SPD_FIL_MEAN && e.op != SPD_FIL_COV && e.op != SPD_FIL_LAST)
            return m_fail(SPD_E_ARG, std::string(who) + ": op " + std::to_string(e.op) + " of " + entry_text(k, names_a[k]) +
                                         " is not SPD_FIL_MEAN (0), SPD_FIL_COV (1) or SPD_FIL_LAST (2)");
        if (e.name_b >= 0 && e.op != SPD_FIL_COV)
            return m_fail(SPD_E_ARG, std::string(who) + ": " + entry_text(k, names_a[k]) + " names a second field ('" + names_b[k] +
                                         "'), which only SPD_FIL_COV takes");
    }
    for (const auto &e : out.entries) {
        out.plane_a.push_back(plane_index(out.planes, {e.name, e.level, e.filter}));
        out.plane_b.push_back(e.name_b >= 0 ? plane_index(out.planes, {e.name_b, e.level_b, e.filter}) : out.plane_a.back());
    }
    if (out.planes.size() > static_cast<size_t>(kFilMaxPlanes))
        return m_fail(SPD_E_ARG, std::string(who) + ": the entries name " + std::to_string(out.planes.size()) +
                                     " distinct (name, level, filter) planes; at most " + std::to_string(kFilMaxPlanes) + " can be filtered");
    if (spinup < 0) return m_fail(SPD_E_ARG, std::string(who) + ": spinup must not be negative");
    if (int rc = wintape_schedule_check(who, window, every, sample_every)) return rc;
    if (capacity < 1) return m_fail(SPD_E_ARG, std::string(who) + ": capacity must be at least 1");
    if (dtype != SPD_TAPE_F32 && dtype != SPD_TAPE_F64) return m_fail(SPD_E_ARG, std::string(who) + ": dtype must be SPD_TAPE_F32 or SPD_TAPE_F64");
    return SPD_OK;
}
}  // namespace

FilDecision spd::filtape_advance(const WinSchedule &s, int spinup, WinOpen &w, long long &k, int step_after, const Calendar &next, int32_t *row) {
    const int before = w.samples;
    const WinDecision wd = wintape_advance(s, w, step_after, next, row);
    FilDecision d;
    d.sample = wd.sample;
    d.close = wd.close;
    bool counted = false;
    if (wd.sample) {
        ++k;
        d.first = k == 1 ? 1 : 0;
        counted = k > spinup;
        if (!counted) {  // (the schedule has counted the sample: into the closed window's row, or into the open window)
            if (wd.close) --row[6];
            else --w.samples;
        }
    }
    d.c = counted ? before + 1 : 0;
    d.n = before + (counted ? 1 : 0);
    return d;
}

hipError_t spd::filtape_step(spd_model *m, int first, int count, const FilDecision &d, int slot, hipStream_t s) {
    const spd_model::FilTape &ft = m->filtape;
    if (count == 0) return hipSuccess;
    hipError_t e = hipSuccess;
    if (d.sample) {
        e = sample_front(m, ft, first, count, s);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(filtape_filter_kernel, dim3(kPairs / kT, ft.nplanes, count), dim3(kT), 0, s, ft.planes, ft.slab, ft.slab_fields, ft.state,
                               ft.y, ft.nplanes, ft.smax, first, d.first, m->stored32 ? 1 : 0);
            e = hipGetLastError();
        }
    }
    if (e == hipSuccess && (d.c > 0 || d.close)) {
        const int E = static_cast<int>(ft.entries.size());
        const dim3 grid(kPairs / kT, E, count);
        const long slot_stride = static_cast<long>(m->M) * NG;
        if (ft.dtype == SPD_TAPE_F64)
            hipLaunchKernelGGL(filtape_accumulate_kernel<double>, grid, dim3(kT), 0, s, ft.items, ft.y, ft.acc, ft.nplanes, E, slot_stride, first, d.c,
                               d.close ? 1 : 0, d.n, slot);
        else
            hipLaunchKernelGGL(filtape_accumulate_kernel<float>, grid, dim3(kT), 0, s, ft.items, ft.y, ft.acc, ft.nplanes, E, slot_stride, first, d.c,
                               d.close ? 1 : 0, d.n, slot);
        e = hipGetLastError();
    }
    return e;
}

extern "C" {

int spd_filtape_filter_host(const double *sections, int n_sections, const double *x, int n, double *y) {
    const char *who = "spd_filtape_filter_host";
    if (n_sections < 1 || n_sections > kFilMaxSections)
        return m_fail(SPD_E_ARG, std::string(who) + ": n_sections must be 1 ... " + std::to_string(kFilMaxSections) + ", got " + std::to_string(n_sections));
    if (!sections) return m_fail(SPD_E_ARG, std::string(who) + ": null sections");
    std::vector<FilSection> cascade;
    if (int rc = check_sections(who, "", sections, n_sections, cascade)) return rc;
    if (n < 0 || (n > 0 && (!x || !y))) return m_fail(SPD_E_ARG, std::string(who) + ": bad series");
    fil_series_host(cascade.data(), n_sections, x, n, y);
    return SPD_OK;
}

int spd_filtape_check(const double *sections, const int *n_sections, int n_filters, const char *const *names_a, const int *levels_a,
                      const int *filters, const int *ops, const char *const *names_b, const int *levels_b, int n_entries, int window, int every,
                      int sample_every, int spinup, int capacity, int dtype) {
    FilChecked checked;
    return check_arguments("spd_filtape_check", sections, n_sections, n_filters, names_a, levels_a, filters, ops, names_b, levels_b, n_entries, window,
                           every, sample_every, spinup, capacity, dtype, checked);
}

int spd_model_filtape_off(spd_model_handle m) {
    const char *who = "spd_model_filtape_off";
    if (int rc = configure_allowed(m, who)) return rc;
    return retire(m, m->filtape);
}

int spd_model_filtape_configure(spd_model_handle m, const double *sections, const int *n_sections, int n_filters, const char *const *names_a,
                                const int *levels_a, const int *filters, const int *ops, const char *const *names_b, const int *levels_b,
                                int n_entries, int window, int every, int sample_every, int spinup, int capacity, int dtype) {
    const char *who = "spd_model_filtape_configure";
    FilChecked in;
    if (int rc = check_arguments(who, sections, n_sections, n_filters, names_a, levels_a, filters, ops, names_b, levels_b, n_entries, window, every,
                                 sample_every, spinup, capacity, dtype, in))
        return rc;
    if (int rc = configure_allowed(m, who)) return rc;
    {  // the planes on the target levels of spd_model_plev_configure, a's and b's
        struct Named { int name, level; };
        std::vector<Named> both_sides;
        std::vector<const char *> both_names;
        for (int k = 0; k < n_entries; ++k) {
            both_sides.push_back({in.entries[k].name, in.entries[k].level});
            both_names.push_back(names_a[k]);
        }
        for (int k = 0; k < n_entries; ++k)
            if (in.entries[k].name_b >= 0) {
                both_sides.push_back({in.entries[k].name_b, in.entries[k].level_b});
                both_names.push_back(names_b[k]);
            }
        if (int rc = check_plev_entries(m, who, both_names.data(), both_sides)) return rc;
    }
    spd_model::FilTape &ft = m->filtape;
    if (int rc = retire(m, ft)) return rc;
    spd_model::FilTape next;
    next.window = window;
    next.every = every;
    next.sample_every = sample_every;
    next.spinup = spinup;
    next.dtype = dtype;
    next.nfilters = n_filters;
    for (const FilPlaneKey &q : in.planes) next.smax = std::max(next.smax, static_cast<int>(in.filters[q.filter].size()));
    const size_t M = static_cast<size_t>(m->M), slots = static_cast<size_t>(capacity), E = static_cast<size_t>(n_entries), F = in.planes.size();
    const size_t S = static_cast<size_t>(next.smax), elem = dtype == SPD_TAPE_F64 ? sizeof(double) : sizeof(float);
    // the sample plan over the names among the filtered planes, in the order they first appear
    std::vector<int> ids;
    for (const FilPlaneKey &q : in.planes)
        if (std::find(ids.begin(), ids.end(), q.name) == ids.end()) ids.push_back(q.name);
    SamplePlan plan;
    plan_sample(m, ids, next, plan);
    // one allocation: ring | state | y | accumulators | slab | tables[2] | plane descriptors | entry descriptors
    const size_t per_slot = M * E * NG * elem;
    if (slots > (static_cast<size_t>(-1) / 2) / per_slot) return m_fail(SPD_E_ARG, std::string(who) + ": the filter tape's size does not fit size_t");
    const size_t ring = sample_up(slots * per_slot), state = sample_up(M * F * S * 2 * NG * sizeof(double));
    const size_t ys = sample_up(M * F * NG * sizeof(double)), accs = sample_up(M * E * NG * sizeof(double));
    const size_t desc = sample_up(F * sizeof(FilTapePlane)), list = sample_up(E * sizeof(FilTapeItem));
    const size_t total = ring + state + ys + accs + plan.slab_bytes + 2 * plan.table_bytes + desc + list;
    void *p = nullptr;
    if (hipMalloc(&p, total) != hipSuccess) {  // the filter tape is off; the model is as usable as before
        (void)hipGetLastError();
        return m_fail(SPD_E_DEVICE, std::string(who) + ": cannot allocate the filter tape (" + std::to_string(total) + " bytes asked for: " +
                                        std::to_string(capacity) + " windows of " + std::to_string(per_slot) + " bytes, " + std::to_string(state + ys) +
                                        " bytes of filter state and " + std::to_string(accs) + " bytes of accumulators); the filter tape is off");
    }
    Carve carve{static_cast<char *>(p)};
    next.alloc = p;
    next.data = carve.take<char>(ring);
    next.state = carve.take<double>(state);
    next.y = carve.take<double>(ys);
    next.acc = carve.take<double>(accs);
    carve_front(carve, plan, next);
    next.planes = carve.take<FilTapePlane>(desc);
    next.items = carve.take<FilTapeItem>(list);
    std::vector<SampleSource> sources;  // (per plane of plan.vars, in their order)
    hipError_t e = build_sample_front(m, plan, next, sources);
    std::vector<FilTapePlane> host_planes;
    for (const FilPlaneKey &q : in.planes) {
        FilTapePlane d{};
        d.source = plane_source(plan, sources, q.name, q.level);
        d.narrow = cat_kind(q.name) == CAT_PRECIP && m->reg[kStatsCatalogue[q.name].name].f32 ? 1 : 0;  // (what physics_storage32 keeps as float)
        d.n_sections = static_cast<int>(in.filters[q.filter].size());
        for (int s = 0; s < d.n_sections; ++s) d.sec[s] = in.filters[q.filter][s];
        host_planes.push_back(d);
    }
    std::vector<FilTapeItem> host_items;
    for (size_t k = 0; k < E; ++k)  // (the kernel indexes y with these)
        if (in.plane_a[k] < 0 || in.plane_b[k] < 0 || static_cast<size_t>(in.plane_a[k]) >= F || static_cast<size_t>(in.plane_b[k]) >= F) {
            (void)hipFree(p);
            return m_fail(SPD_E_ARG, std::string(who) + ": entry " + std::to_string(k) + " points outside the filtered planes");
        }
    for (size_t k = 0; k < E; ++k)
        host_items.push_back({in.plane_a[k], in.plane_b[k], in.entries[k].op, 0, static_cast<char *>(next.data) + slots * M * k * NG * elem});
    if (e == hipSuccess) e = hipMemcpy(next.planes, host_planes.data(), host_planes.size() * sizeof(FilTapePlane), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(next.items, host_items.data(), host_items.size() * sizeof(FilTapeItem), hipMemcpyHostToDevice);
    if (e != hipSuccess) return upload_failed(who, e, p);
    next.nplanes = static_cast<int>(F);
    next.entries = std::move(in.entries);
    next.ring = SampleRing(capacity, 8);
    next.window_start = -1;  // (the first window starts at the model's current step, with filter sample 1: plan_segment reads the counter)
    next.on = true;
    ft = std::move(next);
    return SPD_OK;
}

int spd_model_filtape_reset(spd_model_handle m) {
    if (int rc = ring_reset(m, "spd_model_filtape_reset", &spd_model::filtape, kFilOff)) return rc;
    // (the next window starts at the next step; the next sample is filter sample 1, which reads no state, and the first counted
    // sample overwrites the accumulators: no device work)
    m->filtape.window_start = -1;
    m->filtape.samples = 0;
    m->filtape.filter_samples = 0;
    return SPD_OK;
}

int spd_model_filtape_info(spd_model_handle m, long long *taken, int *held, int *capacity, int *window, int *every, int *sample_every, int *spinup,
                           int *dtype, int *n_filters, int *n_planes, int *n_entries, long long *filter_samples) {
    if (!m) return m_fail(SPD_E_ARG, "spd_model_filtape_info: null model");
    const spd_model::FilTape &ft = m->filtape;
    if (!ft.on) return m_fail(SPD_E_ARG, std::string("spd_model_filtape_info: ") + kFilOff);
    if (taken) *taken = ft.ring.taken;
    if (held) *held = static_cast<int>(ft.ring.held());
    if (capacity) *capacity = ft.ring.capacity;
    if (window) *window = ft.window;
    if (every) *every = ft.every;
    if (sample_every) *sample_every = ft.sample_every;
    if (spinup) *spinup = ft.spinup;
    if (dtype) *dtype = ft.dtype;
    if (n_filters) *n_filters = ft.nfilters;
    if (n_planes) *n_planes = ft.nplanes;
    if (n_entries) *n_entries = static_cast<int>(ft.entries.size());
    if (filter_samples) *filter_samples = ft.window_start < 0 ? 0 : ft.filter_samples;
    return SPD_OK;
}

int spd_model_filtape_times(spd_model_handle m, int32_t *rows, int max_rows) {
    return ring_rows(m, "spd_model_filtape_times", &spd_model::filtape, kFilOff, rows, max_rows);
}

int spd_model_filtape_read(spd_model_handle m, int entry, int first, int count, int t0, int nt, void *dst_device, size_t dst_bytes, void *stream) {
    const char *who = "spd_model_filtape_read";
    if (!m) return m_fail(SPD_E_ARG, std::string(who) + ": null model");
    const spd_model::FilTape &ft = m->filtape;
    if (int rc = read_allowed(m, who, ft.on, kFilOff, ft.validity, "the filter tape is invalid until spd_model_filtape_reset")) return rc;
    if (entry < 0 || entry >= static_cast<int>(ft.entries.size()))
        return m_fail(SPD_E_ARG, std::string(who) + ": entry " + std::to_string(entry) + " is out of range (0 ... " + std::to_string(ft.entries.size() - 1) + ")");
    if (first < 0 || count < 0 || first + count > m->M) return m_fail(SPD_E_ARG, std::string(who) + ": member range out of bounds");
    if (int rc = held_range(who, ft.ring, t0, nt, "window")) return rc;
    const size_t elem = ft.dtype == SPD_TAPE_F64 ? sizeof(double) : sizeof(float), per = NG, M = static_cast<size_t>(m->M);
    const size_t need = static_cast<size_t>(count) * static_cast<size_t>(nt) * per * elem;
    if (int rc = destination_fits(who, dst_device, dst_bytes, need, 16)) return rc;
    if (count == 0 || nt == 0) return SPD_OK;
    M_HIP(hipSetDevice(m->ctx->device));
    const size_t offset = static_cast<size_t>(ft.ring.capacity) * M * static_cast<size_t>(entry) * per;
    const char *src = static_cast<const char *>(ft.data) + (offset + static_cast<size_t>(first) * per) * elem;
    const hipError_t e = run_tape_gather(src, dst_device, static_cast<long>(per), static_cast<long>(M * per), static_cast<int>(elem), count, nt,
                                         ft.ring.slot_of_held(t0), ft.ring.capacity, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return m_fail(SPD_E_DEVICE, std::string(who) + ": " + hipGetErrorString(e));
    return SPD_OK;
}

}  // extern "C"
