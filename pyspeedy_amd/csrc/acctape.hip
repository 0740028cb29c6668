// Window sums, means and extremes of the column physics' 2-D outputs, accumulated on the GPU behind every step of a multi-step call
// (spd_model_acctape_*, include/pyspeedy_amd.h).
//
// The values are read where the column kernel stores them (diag = 1 on every step while the recorder is on), in their stored
// precision, widened to fp64: no front end, no slab, no transform.  One launch per member group and step serves every entry: a lane
// loads two points of one plane of one member once and updates whichever of sum, minimum and maximum the entries of that name ask
// for.  The step's number within its window comes by value: step 1 overwrites the accumulators and reads none of them, so a new
// window, a reset or a reconfiguration needs no device work.  The closing step writes the window's results into the ring slot in
// the same launch.  The arithmetic is fixed -- sum in step order from the first value itself, mean = sum / n as one division,
// acc = x < acc ? x : acc and acc = x > acc ? x : acc -- so the result does not depend on the launch plan.
// Accumulators are read again one step later: ordinary loads and stores.  Source loads and ring stores are read once / written once:
// non-temporal.  Two points (16 bytes of fp64) per lane, coalesced over the 4608 points of a plane.
#include <hip/hip_runtime.h>

#include "acctape.hpp"
#include "global_mem.hpp"
#include "model_state.hpp"
#include "tables.hpp"

namespace spd {

namespace {
constexpr int kT = 256;
constexpr int kPairs = NG / 2;  // 2304 = 9 blocks of 256 lanes: no partial block
static_assert(NG % 2 == 0 && kPairs % kT == 0, "a plane is a whole number of blocks of point pairs");

// blockIdx.x: pairs of points, blockIdx.y: plane (descriptor), blockIdx.z: member of the group
template <typename T>
__global__ __launch_bounds__(kT) void acctape_step_kernel(const AccTapePlane *__restrict__ planes, int first, int step, int close, int slot,
                                                          int store32) {
    const int p = 2 * (blockIdx.x * kT + threadIdx.x);
    if (p >= NG) return;
    const AccTapePlane d = planes[blockIdx.y];
    const long at = (first + static_cast<long>(blockIdx.z)) * d.member_stride + p;
    const long src_at = at + static_cast<long>(d.plane) * NG;
    const double2v x = store32 && d.narrow ? widen(stream_load_pair(static_cast<const float *>(d.src) + src_at))
                                           : widen(stream_load_pair(static_cast<const double *>(d.src) + src_at));
    const long ring_at = static_cast<long>(slot) * d.slot_stride + at;
    if (d.sum) {
        double2v acc = x;
        if (step > 1) {
            acc = load_pair(d.sum + at);
            acc.x = acc.x + x.x;
            acc.y = acc.y + x.y;
        }
        if (!close) {
            store_pair(d.sum + at, acc);
        } else {
            if (d.ring[0]) ring_store<T>(d.ring[0], ring_at, acc);
            if (d.ring[1]) {
                const double n = static_cast<double>(step);
                double2v mean;
                mean.x = acc.x / n;
                mean.y = acc.y / n;
                ring_store<T>(d.ring[1], ring_at, mean);
            }
        }
    }
    if (d.mn) {
        double2v acc = x;
        if (step > 1) {
            acc = load_pair(d.mn + at);
            acc.x = x.x < acc.x ? x.x : acc.x;
            acc.y = x.y < acc.y ? x.y : acc.y;
        }
        if (!close) store_pair(d.mn + at, acc);
        else ring_store<T>(d.ring[2], ring_at, acc);
    }
    if (d.mx) {
        double2v acc = x;
        if (step > 1) {
            acc = load_pair(d.mx + at);
            acc.x = x.x > acc.x ? x.x : acc.x;
            acc.y = x.y > acc.y ? x.y : acc.y;
        }
        if (!close) store_pair(d.mx + at, acc);
        else ring_store<T>(d.ring[3], ring_at, acc);
    }
}
}  // namespace

hipError_t run_acctape_step(const AccTapePlane *planes, int nplanes, int first, int count, int step, int close, int slot, int store32,
                            int f64, hipStream_t s) {
    if (nplanes == 0 || count == 0) return hipSuccess;
    const dim3 grid(kPairs / kT, nplanes, count);
    if (f64)
        hipLaunchKernelGGL(acctape_step_kernel<double>, grid, dim3(kT), 0, s, planes, first, step, close, slot, store32);
    else
        hipLaunchKernelGGL(acctape_step_kernel<float>, grid, dim3(kT), 0, s, planes, first, step, close, slot, store32);
    return hipGetLastError();
}

}  // namespace spd

// ---- host side: the configuration and the C ABI (spd_model_acctape_*); the step loop calls run_acctape_step itself ----

namespace {
// The column physics' 2-D outputs of which every plane is stored on every step that runs with diag = 1 (physics.hip).  hfluxn (its
// third plane is never written) and qcloud_equiv (written on shortwave steps only, and an input of the next steps rather than a
// flux) are not confirmed and are refused by name.
struct AccName {
    const char *name;
    int planes;
};
constexpr AccName kAccNames[] = {{"precnv", 1}, {"precls", 1}, {"cbmf", 1}, {"olr", 1},  {"tsr", 1},  {"ssr", 1},  {"ssrd", 1},
                                 {"slr", 1},    {"slrd", 1},   {"ustr", 3}, {"vstr", 3}, {"shf", 3}, {"evap", 3}, {"slru", 3}};
constexpr int kAccNNames = static_cast<int>(sizeof(kAccNames) / sizeof(kAccNames[0]));
int acc_name_id(const char *name) {
    for (int v = 0; name && v < kAccNNames; ++v)
        if (std::strcmp(name, kAccNames[v].name) == 0) return v;
    return -1;
}
const void *acc_source(const spd_model *m, int id) {
    const spd_physics_args &pa = m->pa;
    const double *const src[kAccNNames] = {pa.precnv, pa.precls, pa.cbmf, pa.olr, pa.tsr, pa.ssr, pa.ssrd,
                                           pa.slr,    pa.slrd,   pa.ustr, pa.vstr, pa.shf, pa.evap, pa.slru};
    return src[id];
}
const char *const kAccOff = "no accumulation tape configured (spd_model_acctape_configure)";
}  // namespace

extern "C" {

int spd_model_acctape_configure(spd_model_handle m, const char *const *names, const int *ops, int n_entries, int every, int capacity,
                                int dtype) {
    const char *who = "spd_model_acctape_configure";
    // (the arguments first: nothing below needs the device)
    if (n_entries < 0 || (n_entries > 0 && (!names || !ops))) return m_fail(SPD_E_ARG, std::string(who) + ": bad list of entries");
    std::vector<spd_model::AccTape::Entry> entries;
    for (int k = 0; k < n_entries; ++k) {
        const int id = acc_name_id(names[k]);
        if (id < 0) {
            const std::string name = names[k] ? names[k] : "(null)";
            if (name == "hfluxn" || name == "qcloud_equiv")
                return m_fail(SPD_E_ARG, std::string(who) + ": '" + name + "' is not stored in every plane on every step and cannot be accumulated");
            return m_fail(SPD_E_ARG, std::string(who) + ": unknown variable '" + name + "'");
        }
        if (ops[k] != SPD_ACC_SUM && ops[k] != SPD_ACC_MEAN && ops[k] != SPD_ACC_MIN && ops[k] != SPD_ACC_MAX)
            return m_fail(SPD_E_ARG, std::string(who) + ": unknown op " + std::to_string(ops[k]) + " for '" + names[k] +
                                         "' (SPD_ACC_SUM, SPD_ACC_MEAN, SPD_ACC_MIN or SPD_ACC_MAX)");
        for (const auto &e : entries)
            if (e.name == id && e.op == ops[k])
                return m_fail(SPD_E_ARG, std::string(who) + ": entry ('" + names[k] + "', " + std::to_string(ops[k]) + ") named twice");
        entries.push_back({id, ops[k], kAccNames[id].planes, 0});
    }
    if (n_entries > 0 && every < 1) return m_fail(SPD_E_ARG, std::string(who) + ": every must be at least 1");
    if (n_entries > 0 && capacity < 1) return m_fail(SPD_E_ARG, std::string(who) + ": capacity must be at least 1");
    if (n_entries > 0 && dtype != SPD_TAPE_F32 && dtype != SPD_TAPE_F64)
        return m_fail(SPD_E_ARG, std::string(who) + ": dtype must be SPD_TAPE_F32 or SPD_TAPE_F64");
    if (int rc = configure_allowed(m, who)) return rc;
    spd_model::AccTape &ac = m->acctape;
    if (int rc = retire(m, ac)) return rc;
    if (n_entries == 0) return SPD_OK;  // off
    spd_model::AccTape next;
    next.every = every;
    next.dtype = dtype;
    const size_t M = static_cast<size_t>(m->M), slots = static_cast<size_t>(capacity);
    const size_t elem = dtype == SPD_TAPE_F64 ? sizeof(double) : sizeof(float);
    // what each name needs: [0] a running sum (sum or mean), [1] a minimum, [2] a maximum
    bool need[kAccNNames][3] = {};
    size_t ring_planes = 0, acc_planes = 0, desc_planes = 0;
    for (auto &e : entries) {
        e.offset = slots * M * ring_planes * NG;
        ring_planes += static_cast<size_t>(e.planes);
        need[e.name][e.op == SPD_ACC_MIN ? 1 : e.op == SPD_ACC_MAX ? 2 : 0] = true;
    }
    for (int v = 0; v < kAccNNames; ++v) {
        const int kinds = (need[v][0] ? 1 : 0) + (need[v][1] ? 1 : 0) + (need[v][2] ? 1 : 0);
        acc_planes += static_cast<size_t>(kinds) * kAccNames[v].planes;
        if (kinds) desc_planes += static_cast<size_t>(kAccNames[v].planes);
    }
    // one allocation: ring | accumulators | plane descriptors
    const size_t per_slot = M * ring_planes * NG * elem;
    if (per_slot != 0 && slots > (static_cast<size_t>(-1) / 2) / per_slot)
        return m_fail(SPD_E_ARG, std::string(who) + ": the accumulation tape's size does not fit size_t");
    const size_t ring = sample_up(slots * per_slot), accs = sample_up(M * acc_planes * NG * sizeof(double));
    const size_t desc = sample_up(desc_planes * sizeof(AccTapePlane));
    const size_t total = ring + accs + desc;
    void *p = nullptr;
    if (hipMalloc(&p, total) != hipSuccess) {  // the accumulation tape is off; the model is as usable as before
        (void)hipGetLastError();
        return m_fail(SPD_E_DEVICE, std::string(who) + ": cannot allocate the accumulation tape (" + std::to_string(total) +
                                        " bytes asked for: " + std::to_string(capacity) + " windows of " + std::to_string(per_slot) +
                                        " bytes and " + std::to_string(accs) + " bytes of accumulators); the accumulation tape is off");
    }
    Carve carve{static_cast<char *>(p)};
    next.alloc = p;
    next.data = carve.take<char>(ring);
    double *acc_at = carve.take<double>(accs);
    next.planes = carve.take<AccTapePlane>(desc);
    std::vector<AccTapePlane> host_planes;
    for (int v = 0; v < kAccNNames; ++v) {
        if (!need[v][0] && !need[v][1] && !need[v][2]) continue;
        const size_t planes = static_cast<size_t>(kAccNames[v].planes), per = planes * NG;
        double *acc[3] = {nullptr, nullptr, nullptr};
        for (int a = 0; a < 3; ++a)
            if (need[v][a]) acc[a] = acc_at, acc_at += M * per;
        for (size_t k = 0; k < planes; ++k) {
            AccTapePlane d{};
            // (plane k in elements: the kernel indexes the source as float or double, as the model stores it at the time of the step)
            d.src = acc_source(m, v);
            d.plane = static_cast<int>(k);
            d.sum = acc[0] ? acc[0] + k * NG : nullptr;
            d.mn = acc[1] ? acc[1] + k * NG : nullptr;
            d.mx = acc[2] ? acc[2] + k * NG : nullptr;
            for (const auto &e : entries)
                if (e.name == v) d.ring[e.op] = static_cast<char *>(next.data) + (e.offset + k * NG) * elem;
            d.member_stride = static_cast<long>(per);
            d.slot_stride = static_cast<long>(M * per);
            d.narrow = m->reg[kAccNames[v].name].f32 ? 1 : 0;  // (what physics_storage32 keeps as float)
            host_planes.push_back(d);
        }
    }
    const hipError_t e = hipMemcpy(next.planes, host_planes.data(), host_planes.size() * sizeof(AccTapePlane), hipMemcpyHostToDevice);
    if (e != hipSuccess) return upload_failed(who, e, p);
    next.nplanes = static_cast<int>(host_planes.size());
    next.entries = std::move(entries);
    next.ring = SampleRing(capacity, 7);
    next.window_start = -1;  // (the first window starts at the model's current step: step_impl reads the counter when it next runs)
    next.on = true;
    ac = std::move(next);
    return SPD_OK;
}

int spd_model_acctape_reset(spd_model_handle m) {
    if (int rc = ring_reset(m, "spd_model_acctape_reset", &spd_model::acctape, kAccOff)) return rc;
    m->acctape.window_start = -1;  // (the next window starts at the next step, which overwrites the accumulators: no device work)
    return SPD_OK;
}

int spd_model_acctape_info(spd_model_handle m, long long *taken, int *held, int *capacity, int *every, int *dtype) {
    if (!m) return m_fail(SPD_E_ARG, "spd_model_acctape_info: null model");
    const spd_model::AccTape &ac = m->acctape;
    if (!ac.on) return m_fail(SPD_E_ARG, std::string("spd_model_acctape_info: ") + kAccOff);
    if (taken) *taken = ac.ring.taken;
    if (held) *held = static_cast<int>(ac.ring.held());
    if (capacity) *capacity = ac.ring.capacity;
    if (every) *every = ac.every;
    if (dtype) *dtype = ac.dtype;
    return SPD_OK;
}

int spd_model_acctape_times(spd_model_handle m, int32_t *rows, int max_rows) {
    return ring_rows(m, "spd_model_acctape_times", &spd_model::acctape, kAccOff, rows, max_rows);
}

int spd_model_acctape_read(spd_model_handle m, const char *name, int op, int first, int count, int t0, int nt, void *dst_device,
                           size_t dst_bytes, void *stream) {
    const char *who = "spd_model_acctape_read";
    if (!m || !name) return m_fail(SPD_E_ARG, std::string(who) + ": null argument");
    const spd_model::AccTape &ac = m->acctape;
    if (int rc = read_allowed(m, who, ac.on, kAccOff, ac.validity, "the accumulation tape is invalid until spd_model_acctape_reset")) return rc;
    const int id = acc_name_id(name);
    const spd_model::AccTape::Entry *v = nullptr;
    for (const auto &x : ac.entries)
        if (x.name == id && x.op == op) v = &x;
    if (!v) return m_fail(SPD_E_ARG, std::string(who) + ": ('" + name + "', " + std::to_string(op) + ") is not among the configured entries");
    if (first < 0 || count < 0 || first + count > m->M) return m_fail(SPD_E_ARG, std::string(who) + ": member range out of bounds");
    if (int rc = held_range(who, ac.ring, t0, nt, "window")) return rc;
    const size_t elem = ac.dtype == SPD_TAPE_F64 ? sizeof(double) : sizeof(float), per = static_cast<size_t>(v->planes) * NG;
    const size_t need = static_cast<size_t>(count) * static_cast<size_t>(nt) * per * elem;
    if (int rc = destination_fits(who, dst_device, dst_bytes, need, 16)) return rc;
    if (count == 0 || nt == 0) return SPD_OK;
    M_HIP(hipSetDevice(m->ctx->device));
    const char *src = static_cast<const char *>(ac.data) + (v->offset + static_cast<size_t>(first) * per) * elem;
    const hipError_t e = run_tape_gather(src, dst_device, static_cast<long>(per), static_cast<long>(static_cast<size_t>(m->M) * per),
                                         static_cast<int>(elem), count, nt, ac.ring.slot_of_held(t0), ac.ring.capacity,
                                         static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return m_fail(SPD_E_DEVICE, std::string(who) + ": " + hipGetErrorString(e));
    return SPD_OK;
}

}  // extern "C"
