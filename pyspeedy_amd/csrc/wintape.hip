// Window sums, means, extremes and threshold counts of the state's grid-space fields, accumulated on the GPU behind the sampled
// steps of a multi-step call (spd_model_wintape_*, include/pyspeedy_amd.h).
//
// A sample is what an fp64 tape of the same name holds: model.hip runs the tape's front end into a slab of the recorder's own, and
// the kernel below applies export_unit (sample_source.hpp) exactly as tape_store_kernel does; precnv / precls are read where the
// column kernel stores them, in their stored precision, widened.  A wind-speed name is sqrt(u * u + v * v) of two such values in
// four correctly rounded operations without contraction, so that a host restatement gives the same bits.  One launch per member
// group serves every entry: a lane loads two points of one plane of one member once and updates whichever of sum, minimum, maximum
// and the two counts the entries of that name ask for.  The sample's number within its window comes by value: sample 1 overwrites
// the accumulators and reads none of them, so a new window, a reset or a reconfiguration needs no device work.  The closing step
// writes the window's results into the ring slot in the same launch; a closing step that is not sampled launches the kernel with
// k = 0, which loads no sample and only closes.  The arithmetic is fixed -- sum in sample order from the first value itself, mean =
// sum / n as one division, acc = x < acc ? x : acc, acc = x > acc ? x : acc, counts as fp64 integers -- so the result does not
// depend on the launch plan.
// The front end wrote the slab just before and the accumulators are read again at the next sample: ordinary loads and stores.
// Ring stores are written once and read by the host's gather only: non-temporal.  Two points (16 bytes of fp64) per lane,
// coalesced over the 4608 points of a plane.
#include <hip/hip_runtime.h>

#include <cmath>

#include "global_mem.hpp"
#include "model_state.hpp"
#include "tables.hpp"
#include "wintape.hpp"

namespace spd {

namespace {
constexpr int kT = 256;
constexpr int kPairs = NG / 2;  // 2304 = 9 blocks of 256 lanes: no partial block
static_assert(NG % 2 == 0 && kPairs % kT == 0, "a plane is a whole number of blocks of point pairs");

// blockIdx.x: pairs of points, blockIdx.y: plane (descriptor), blockIdx.z: member of the group
template <typename T>
__global__ __launch_bounds__(kT) void wintape_step_kernel(const WinTapePlane *__restrict__ planes, const double *__restrict__ slab,
                                                          int slab_fields, int first, int k, int close, int n, int slot, int store32) {
    const int p = 2 * (blockIdx.x * kT + threadIdx.x);
    if (p >= NG) return;
    const WinTapePlane d = planes[blockIdx.y];
    const long i = first + static_cast<long>(blockIdx.z);
    const long at = i * d.member_stride + p;
    double2v x = both(0.0);
    if (k > 0) {
        x = with_sample_plane(d.source, slab, slab_fields, store32 && d.narrow, i, [&](auto plane, long) { return widen(load_pair(plane + p)); });
        x.x = export_unit(x.x, d.source.unit);
        x.y = export_unit(x.y, d.source.unit);
        if (d.slab_b >= 0) {  // wind speed: u and v carry no unit conversion
            const double2v v = load_pair(slab + (i * slab_fields + d.slab_b) * NG + p);
            x.x = __dsqrt_rn(__dadd_rn(__dmul_rn(x.x, x.x), __dmul_rn(v.x, v.x)));
            x.y = __dsqrt_rn(__dadd_rn(__dmul_rn(x.y, x.y), __dmul_rn(v.y, v.y)));
        }
    }
    // the accumulators hold the window's earlier samples when there are any: k - 1 of them before this sample, n without one
    const bool held = k > 1 || (k == 0 && n > 0);
    const bool keep = k > 0 && !close;
    const long ring_at = static_cast<long>(slot) * d.slot_stride + at;
    const double nan = __builtin_nan("");
    if (d.sum) {
        double2v acc = x;
        if (held) {
            acc = load_pair(d.sum + at);
            if (k > 0) {
                acc.x = acc.x + x.x;
                acc.y = acc.y + x.y;
            }
        }
        if (keep) store_pair(d.sum + at, acc);
        if (close) {
            if (d.ring[0]) ring_store<T>(d.ring[0], ring_at, n > 0 ? acc : both(0.0));
            if (d.ring[1]) {
                double2v mean = both(nan);
                if (n > 0) {
                    const double cnt = static_cast<double>(n);
                    mean.x = acc.x / cnt;
                    mean.y = acc.y / cnt;
                }
                ring_store<T>(d.ring[1], ring_at, mean);
            }
        }
    }
    if (d.mn) {
        double2v acc = x;
        if (held) {
            acc = load_pair(d.mn + at);
            if (k > 0) {
                acc.x = x.x < acc.x ? x.x : acc.x;
                acc.y = x.y < acc.y ? x.y : acc.y;
            }
        }
        if (keep) store_pair(d.mn + at, acc);
        if (close) ring_store<T>(d.ring[2], ring_at, n > 0 ? acc : both(nan));
    }
    if (d.mx) {
        double2v acc = x;
        if (held) {
            acc = load_pair(d.mx + at);
            if (k > 0) {
                acc.x = x.x > acc.x ? x.x : acc.x;
                acc.y = x.y > acc.y ? x.y : acc.y;
            }
        }
        if (keep) store_pair(d.mx + at, acc);
        if (close) ring_store<T>(d.ring[3], ring_at, n > 0 ? acc : both(nan));
    }
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        if (!d.cnt[c]) continue;
        double2v acc = both(0.0);
        if (held) acc = load_pair(d.cnt[c] + at);
        if (k > 0) {
            const double t = d.thr[c];
            acc.x = acc.x + ((c == 0 ? x.x > t : x.x < t) ? 1.0 : 0.0);
            acc.y = acc.y + ((c == 0 ? x.y > t : x.y < t) ? 1.0 : 0.0);
        }
        if (keep) store_pair(d.cnt[c] + at, acc);
        if (close) ring_store<T>(d.ring[4 + c], ring_at, acc);
    }
}
}  // namespace

// One launch for the members [first, first + count), all planes.  k: number of this launch's sample within its window, from 1
// (1 overwrites the accumulators and reads none of them); 0: the step is not sampled and the launch only closes.  close: the step
// ends the window, whose n samples (this one included) give the results that go into ring slot `slot`; n = 0 closes an empty
// window (sum and counts 0, mean, minimum and maximum quiet NaN) and reads no accumulator.  slab: [M][slab_fields][4608] fp64, as
// the front end left it; store32: the model keeps the narrow sources as float; f64: the ring holds doubles (else floats, rounded to
// nearest).
static hipError_t run_wintape_step(const WinTapePlane *planes, int nplanes, const double *slab, int slab_fields, int first, int count, int k,
                                   int close, int n, int slot, int store32, int f64, hipStream_t s) {
    if (nplanes == 0 || count == 0 || (k == 0 && !close)) return hipSuccess;
    const dim3 grid(kPairs / kT, nplanes, count);
    if (f64)
        hipLaunchKernelGGL(wintape_step_kernel<double>, grid, dim3(kT), 0, s, planes, slab, slab_fields, first, k, close, n, slot, store32);
    else
        hipLaunchKernelGGL(wintape_step_kernel<float>, grid, dim3(kT), 0, s, planes, slab, slab_fields, first, k, close, n, slot, store32);
    return hipGetLastError();
}

}  // namespace spd

// ---- host side: the schedule, the step loop's launches, the configuration and the C ABI (spd_model_wintape_*, spd_wintape_plan) ----

namespace {
// names: the catalogue's, then the two wind speeds of this recorder only (u and v: the catalogue ids they are formed from)
constexpr int kWinWspdGrid = kStatsCatalogueSize, kWinWspdPlev = kStatsCatalogueSize + 1, kWinNNames = kStatsCatalogueSize + 2;
constexpr int kWinNOps = 6;
int win_name_id(const char *name) {
    if (!name) return -1;
    if (std::strcmp(name, "wspd_grid") == 0) return kWinWspdGrid;
    if (std::strcmp(name, "wspd_plev") == 0) return kWinWspdPlev;
    return stats_id(name);
}
bool win_needs_levels(int id) { return id == kWinWspdPlev || (id < kStatsCatalogueSize && cat_needs_levels(id)); }
int win_u_id(int id) { return id == kWinWspdGrid ? 0 : kPlevFirst + PLEV_U; }
const char *const kWinOff = "no window tape configured (spd_model_wintape_configure)";
const char *const kWinOpNames[kWinNOps] = {"SPD_WIN_SUM", "SPD_WIN_MEAN", "SPD_WIN_MIN", "SPD_WIN_MAX", "SPD_WIN_COUNT_ABOVE", "SPD_WIN_COUNT_BELOW"};

}  // namespace

// window kind, `every` and sample_every, as _configure, spd_wintape_plan and the filter tape refuse them
int spd::wintape_schedule_check(const char *who, int window, int every, int sample_every) {
    if (window != SPD_WINDOW_STEPS && window != SPD_WINDOW_DAY && window != SPD_WINDOW_MONTH)
        return m_fail(SPD_E_ARG, std::string(who) + ": unknown window kind " + std::to_string(window) +
                                     " (SPD_WINDOW_STEPS, SPD_WINDOW_DAY or SPD_WINDOW_MONTH)");
    if (window == SPD_WINDOW_STEPS && every < 1) return m_fail(SPD_E_ARG, std::string(who) + ": every must be at least 1 for SPD_WINDOW_STEPS");
    if (window != SPD_WINDOW_STEPS && every != 0)
        return m_fail(SPD_E_ARG, std::string(who) + ": every must be 0 for SPD_WINDOW_DAY and SPD_WINDOW_MONTH");
    if (sample_every < 1) return m_fail(SPD_E_ARG, std::string(who) + ": sample_every must be at least 1");
    return SPD_OK;
}

WinDecision spd::wintape_advance(const WinSchedule &s, WinOpen &w, int step_after, const Calendar &next, int32_t *row) {
    WinDecision d;
    d.sample = step_after % s.sample_every == 0;
    const bool midnight = next.hour == 0 && next.minute == 0;
    d.close = s.window == SPD_WINDOW_STEPS ? step_after % s.every == 0 : s.window == SPD_WINDOW_DAY ? midnight : midnight && next.day == 1;
    if (d.sample) ++w.samples;
    if (d.close) {
        stamp_row(row, step_after, next);
        row[6] = w.samples;
        row[7] = step_after - w.start;
        w.start = step_after;
        w.samples = 0;
    }
    return d;
}

// the launches of the members [first, first + count) for a step that samples (k >= 1: the front end into the recorder's own slab,
// then the kernel) or only closes (k = 0: the kernel alone)
hipError_t spd::wintape_step(spd_model *m, int first, int count, int k, int close, int n, int slot, hipStream_t s) {
    const spd_model::WinTape &wt = m->wintape;
    hipError_t e = hipSuccess;
    if (k > 0) e = sample_front(m, wt, first, count, s);
    if (e == hipSuccess)
        e = run_wintape_step(wt.planes, wt.nplanes, wt.slab, wt.slab_fields, first, count, k, close, n, slot, m->stored32 ? 1 : 0,
                             wt.dtype == SPD_TAPE_F64 ? 1 : 0, s);
    return e;
}

extern "C" {

int spd_wintape_plan(int year, int month, int day, int hour, int minute, int step0, int nsteps, int window, int every, int sample_every,
                     int32_t *rows, int max_rows) {
    const char *who = "spd_wintape_plan";
    if (month < 1 || month > 12 || day < 1 || day > 31 || hour < 0 || hour > 23 || minute < 0 || minute > 59)
        return m_fail(SPD_E_ARG, std::string(who) + ": bad date");
    if (step0 < 0 || nsteps < 0) return m_fail(SPD_E_ARG, std::string(who) + ": step0 and nsteps must not be negative");
    if (static_cast<long long>(step0) + nsteps > 2147483647LL) return m_fail(SPD_E_ARG, std::string(who) + ": step0 + nsteps does not fit an int");
    if (int rc = wintape_schedule_check(who, window, every, sample_every)) return rc;
    if (max_rows < 0 || (max_rows > 0 && !rows)) return m_fail(SPD_E_ARG, std::string(who) + ": bad destination");
    Calendar cal;
    cal.set(year, month, day, hour, minute);
    const WinSchedule schedule{window, every, sample_every};
    WinOpen open{step0, 0};
    int closed = 0;
    for (int it = 0; it < nsteps; ++it) {
        cal.advance();
        int32_t row[8];
        if (wintape_advance(schedule, open, step0 + it + 1, cal, row).close) {
            if (closed < max_rows) std::memcpy(rows + 8 * static_cast<size_t>(closed), row, sizeof(row));
            ++closed;
        }
    }
    return closed;
}

int spd_model_wintape_configure(spd_model_handle m, const char *const *names, const int *ops, const double *thresholds, int n_entries,
                                int window, int every, int sample_every, int capacity, int dtype) {
    const char *who = "spd_model_wintape_configure";
    // (the arguments first, in the header's order: nothing below needs the device)
    if (n_entries < 0 || (n_entries > 0 && (!names || !ops))) return m_fail(SPD_E_ARG, std::string(who) + ": bad list of entries");
    std::vector<spd_model::WinTape::Entry> entries;
    for (int k = 0; k < n_entries; ++k) {
        const int id = win_name_id(names[k]);
        if (id < 0)
            return m_fail(SPD_E_ARG, std::string(who) + ": unknown variable '" + (names[k] ? names[k] : "(null)") +
                                         "' (u_grid, v_grid, t_grid, q_grid, phi_grid, ps_grid, precnv, precls, u_plev, v_plev, t_plev, "
                                         "q_plev, z_plev, mslp, wspd_grid, wspd_plev)" SPD_DERIVED_TAIL);
        entries.push_back({id, ops[k], 0, 0.0, 0});
    }
    for (int k = 0; k < n_entries; ++k)
        if (ops[k] < 0 || ops[k] >= kWinNOps)
            return m_fail(SPD_E_ARG, std::string(who) + ": unknown op " + std::to_string(ops[k]) + " for '" + names[k] +
                                         "' (SPD_WIN_SUM, SPD_WIN_MEAN, SPD_WIN_MIN, SPD_WIN_MAX, SPD_WIN_COUNT_ABOVE or SPD_WIN_COUNT_BELOW)");
    for (int k = 0; k < n_entries; ++k)
        if (ops[k] == SPD_WIN_COUNT_ABOVE || ops[k] == SPD_WIN_COUNT_BELOW) {
            if (!thresholds || !std::isfinite(thresholds[k]))
                return m_fail(SPD_E_ARG, std::string(who) + ": " + kWinOpNames[ops[k]] + " of '" + names[k] + "' needs a finite threshold");
            entries[k].threshold = thresholds[k];
        }
    for (int k = 0; k < n_entries; ++k)
        for (int j = 0; j < k; ++j)
            if (entries[j].name == entries[k].name && entries[j].op == entries[k].op)
                return m_fail(SPD_E_ARG, std::string(who) + ": entry ('" + names[k] + "', " + std::to_string(ops[k]) + ") named twice");
    if (n_entries > 0) {
        if (int rc = wintape_schedule_check(who, window, every, sample_every)) return rc;
        if (capacity < 1) return m_fail(SPD_E_ARG, std::string(who) + ": capacity must be at least 1");
        if (dtype != SPD_TAPE_F32 && dtype != SPD_TAPE_F64) return m_fail(SPD_E_ARG, std::string(who) + ": dtype must be SPD_TAPE_F32 or SPD_TAPE_F64");
    }
    if (int rc = configure_allowed(m, who)) return rc;
    for (int k = 0; k < n_entries; ++k)
        if (win_needs_levels(entries[k].name) && m->plev.n == 0)
            return levels_first(who, names[k]);
    spd_model::WinTape &wt = m->wintape;
    if (int rc = retire(m, wt)) return rc;
    if (n_entries == 0) return SPD_OK;  // off
    spd_model::WinTape next;
    next.window = window;
    next.every = every;
    next.sample_every = sample_every;
    next.dtype = dtype;
    const size_t M = static_cast<size_t>(m->M), slots = static_cast<size_t>(capacity);
    const size_t elem = dtype == SPD_TAPE_F64 ? sizeof(double) : sizeof(float);
    // The sample plan: the catalogue names among the entries in the order they first appear, then the u and v a wind speed is
    // formed from where no entry names them -- planes of the slab without accumulators of their own.
    std::vector<int> ids;
    auto want = [&](int id) {
        if (std::find(ids.begin(), ids.end(), id) == ids.end()) ids.push_back(id);
    };
    for (const auto &e : entries)
        if (e.name < kStatsCatalogueSize) want(e.name);
    for (const auto &e : entries)
        if (e.name >= kStatsCatalogueSize) want(win_u_id(e.name)), want(win_u_id(e.name) + 1);
    SamplePlan plan;
    plan_sample(m, ids, next, plan);
    auto plan_var = [&](int id) -> const SamplePlan::Var & {
        return *std::find_if(plan.vars.begin(), plan.vars.end(), [&](const SamplePlan::Var &v) { return v.id == id; });
    };
    // what each name needs: [0] a running sum (sum or mean), [1] a minimum, [2] a maximum, [3] / [4] a count above / below
    bool need[kWinNNames][5] = {};
    int levels[kWinNNames] = {};
    size_t ring_planes = 0, acc_planes = 0, desc_planes = 0;
    for (auto &e : entries) {
        e.levels = plan_var(e.name < kStatsCatalogueSize ? e.name : win_u_id(e.name)).levels;
        levels[e.name] = e.levels;
        e.offset = slots * M * ring_planes * NG;
        ring_planes += static_cast<size_t>(e.levels);
        need[e.name][e.op <= SPD_WIN_MEAN ? 0 : e.op - 1] = true;
    }
    for (int v = 0; v < kWinNNames; ++v) {
        int kinds = 0;
        for (int a = 0; a < 5; ++a) kinds += need[v][a] ? 1 : 0;
        acc_planes += static_cast<size_t>(kinds) * levels[v];
        if (kinds) desc_planes += static_cast<size_t>(levels[v]);
    }
    // one allocation: ring | accumulators | slab | tables[2] | plane descriptors
    const size_t per_slot = M * ring_planes * NG * elem;
    if (per_slot != 0 && slots > (static_cast<size_t>(-1) / 2) / per_slot)
        return m_fail(SPD_E_ARG, std::string(who) + ": the window tape's size does not fit size_t");
    const size_t ring = sample_up(slots * per_slot), accs = sample_up(M * acc_planes * NG * sizeof(double));
    const size_t desc = sample_up(desc_planes * sizeof(WinTapePlane));
    const size_t total = ring + accs + plan.slab_bytes + 2 * plan.table_bytes + desc;
    void *p = nullptr;
    if (hipMalloc(&p, total) != hipSuccess) {  // the window tape is off; the model is as usable as before
        (void)hipGetLastError();
        return m_fail(SPD_E_DEVICE, std::string(who) + ": cannot allocate the window tape (" + std::to_string(total) +
                                        " bytes asked for: " + std::to_string(capacity) + " windows of " + std::to_string(per_slot) +
                                        " bytes and " + std::to_string(accs) + " bytes of accumulators); the window tape is off");
    }
    Carve carve{static_cast<char *>(p)};
    next.alloc = p;
    next.data = carve.take<char>(ring);
    double *acc_at = carve.take<double>(accs);
    carve_front(carve, plan, next);
    next.planes = carve.take<WinTapePlane>(desc);
    std::vector<SampleSource> sources;  // (per plane of plan.vars, in their order)
    hipError_t e = build_sample_front(m, plan, next, sources);
    std::vector<WinTapePlane> host_planes;
    for (int v = 0; v < kWinNNames; ++v) {
        bool any = false;
        for (int a = 0; a < 5; ++a) any = any || need[v][a];
        if (!any) continue;
        const bool wspd = v >= kStatsCatalogueSize;
        const size_t nlev = static_cast<size_t>(levels[v]), per = nlev * NG;
        double *acc[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
        for (int a = 0; a < 5; ++a)
            if (need[v][a]) acc[a] = acc_at, acc_at += M * per;
        const size_t plane_a = plan_var(wspd ? win_u_id(v) : v).first_plane;
        const size_t plane_b = wspd ? plan_var(win_u_id(v) + 1).first_plane : 0;
        for (size_t k = 0; k < nlev; ++k) {
            WinTapePlane d{};
            d.source = sources[plane_a + k];  // (a wind speed: its u, a slab plane of unit 0)
            d.slab_b = wspd ? sources[plane_b + k].slab_plane : -1;
            d.narrow = !wspd && cat_kind(v) == CAT_PRECIP && m->reg[kStatsCatalogue[v].name].f32 ? 1 : 0;  // (what physics_storage32 keeps as float)
            d.sum = acc[0] ? acc[0] + k * NG : nullptr;
            d.mn = acc[1] ? acc[1] + k * NG : nullptr;
            d.mx = acc[2] ? acc[2] + k * NG : nullptr;
            d.cnt[0] = acc[3] ? acc[3] + k * NG : nullptr;
            d.cnt[1] = acc[4] ? acc[4] + k * NG : nullptr;
            for (const auto &x : entries)
                if (x.name == v) {
                    d.ring[x.op] = static_cast<char *>(next.data) + (x.offset + k * NG) * elem;
                    if (x.op >= SPD_WIN_COUNT_ABOVE) d.thr[x.op - SPD_WIN_COUNT_ABOVE] = x.threshold;
                }
            d.member_stride = static_cast<long>(per);
            d.slot_stride = static_cast<long>(M * per);
            host_planes.push_back(d);
        }
    }
    if (e == hipSuccess) e = hipMemcpy(next.planes, host_planes.data(), host_planes.size() * sizeof(WinTapePlane), hipMemcpyHostToDevice);
    if (e != hipSuccess) return upload_failed(who, e, p);
    next.nplanes = static_cast<int>(host_planes.size());
    next.entries = std::move(entries);
    next.ring = SampleRing(capacity, 8);
    next.window_start = -1;  // (the first window starts at the model's current step: step_impl reads the counter when it next runs)
    next.on = true;
    wt = std::move(next);
    return SPD_OK;
}

int spd_model_wintape_reset(spd_model_handle m) {
    if (int rc = ring_reset(m, "spd_model_wintape_reset", &spd_model::wintape, kWinOff)) return rc;
    m->wintape.window_start = -1;  // (the next window starts at the next step; its first sample overwrites the accumulators: no device work)
    m->wintape.samples = 0;
    return SPD_OK;
}

int spd_model_wintape_info(spd_model_handle m, long long *taken, int *held, int *capacity, int *window, int *every, int *sample_every,
                           int *dtype) {
    if (!m) return m_fail(SPD_E_ARG, "spd_model_wintape_info: null model");
    const spd_model::WinTape &wt = m->wintape;
    if (!wt.on) return m_fail(SPD_E_ARG, std::string("spd_model_wintape_info: ") + kWinOff);
    if (taken) *taken = wt.ring.taken;
    if (held) *held = static_cast<int>(wt.ring.held());
    if (capacity) *capacity = wt.ring.capacity;
    if (window) *window = wt.window;
    if (every) *every = wt.every;
    if (sample_every) *sample_every = wt.sample_every;
    if (dtype) *dtype = wt.dtype;
    return SPD_OK;
}

int spd_model_wintape_times(spd_model_handle m, int32_t *rows, int max_rows) {
    return ring_rows(m, "spd_model_wintape_times", &spd_model::wintape, kWinOff, rows, max_rows);
}

int spd_model_wintape_read(spd_model_handle m, const char *name, int op, int first, int count, int t0, int nt, void *dst_device,
                           size_t dst_bytes, void *stream) {
    const char *who = "spd_model_wintape_read";
    if (!m || !name) return m_fail(SPD_E_ARG, std::string(who) + ": null argument");
    const spd_model::WinTape &wt = m->wintape;
    if (int rc = read_allowed(m, who, wt.on, kWinOff, wt.validity, "the window tape is invalid until spd_model_wintape_reset")) return rc;
    const int id = win_name_id(name);
    const spd_model::WinTape::Entry *v = nullptr;
    for (const auto &x : wt.entries)
        if (x.name == id && x.op == op) v = &x;
    if (!v) return m_fail(SPD_E_ARG, std::string(who) + ": ('" + name + "', " + std::to_string(op) + ") is not among the configured entries");
    if (first < 0 || count < 0 || first + count > m->M) return m_fail(SPD_E_ARG, std::string(who) + ": member range out of bounds");
    if (int rc = held_range(who, wt.ring, t0, nt, "window")) return rc;
    const size_t elem = wt.dtype == SPD_TAPE_F64 ? sizeof(double) : sizeof(float), per = static_cast<size_t>(v->levels) * NG;
    const size_t need = static_cast<size_t>(count) * static_cast<size_t>(nt) * per * elem;
    if (int rc = destination_fits(who, dst_device, dst_bytes, need, 16)) return rc;
    if (count == 0 || nt == 0) return SPD_OK;
    M_HIP(hipSetDevice(m->ctx->device));
    const char *src = static_cast<const char *>(wt.data) + (v->offset + static_cast<size_t>(first) * per) * elem;
    const hipError_t e = run_tape_gather(src, dst_device, static_cast<long>(per), static_cast<long>(static_cast<size_t>(m->M) * per),
                                         static_cast<int>(elem), count, nt, wt.ring.slot_of_held(t0), wt.ring.capacity,
                                         static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return m_fail(SPD_E_DEVICE, std::string(who) + ": " + hipGetErrorString(e));
    return SPD_OK;
}

}  // extern "C"
