// Time series of grid-space fields recorded on the GPU inside multi-step calls (spd_model_tape_*, include/pyspeedy_amd.h).
//
// A sample is what the statistics sample (stats.hip): model.hip runs the same front end -- vort2vel, the export descriptors with a
// slab of the tape's own as destination, the pressure-level kernel with raw = 1 -- and the store kernel below finds the value and
// applies the export units through the same two functions as stats_accumulate_kernel (sample_source.hpp: precnv / precls are read
// where the column kernel stores them, in their stored precision) and writes it into the ring instead of folding it into a mean.
// Streaming kernels: every value is read once and written once and nothing on the device reads the ring until the host asks, so
// loads and stores carry the non-temporal hint.  Two points (16 bytes of fp64) per lane, coalesced over the 4608 points of a plane.
#include <hip/hip_runtime.h>

#include <cmath>

#include "global_mem.hpp"
#include "model_state.hpp"
#include "stream_store.hpp"
#include "tables.hpp"
#include "tape.hpp"

namespace spd {

namespace {
constexpr int kT = 256;
constexpr int kPairs = NG / 2;  // 2304 = 9 blocks of 256 lanes: no partial block
static_assert(NG % 2 == 0 && kPairs % kT == 0, "a plane is a whole number of blocks of point pairs");

// blockIdx.x: pairs of points, blockIdx.y: plane, blockIdx.z: member of the group
template <typename T>
__global__ __launch_bounds__(kT) void tape_store_kernel(const TapePlane *__restrict__ planes, const double *__restrict__ slab, int slab_fields,
                                                        int first, int slot, int store32) {
    using T2 = typename Pair<T>::type;
    const int p = 2 * (blockIdx.x * kT + threadIdx.x);
    if (p >= NG) return;
    const TapePlane d = planes[blockIdx.y];
    const long i = first + static_cast<long>(blockIdx.z);
    const double2v x = with_sample_plane(d.source, slab, slab_fields, store32, i,
                                         [&](auto plane, long) { return widen(stream_load_pair(plane + p)); });
    T2 out;
    out.x = static_cast<T>(export_unit(x.x, d.source.unit));
    out.y = static_cast<T>(export_unit(x.y, d.source.unit));
    T *dst = static_cast<T *>(d.dst) + static_cast<long>(slot) * d.slot_stride + i * d.member_stride + p;
    stream_store_global(reinterpret_cast<T2 *>(dst), out);
}

// blockIdx.x: 16-byte pieces of one (member, sample) entry, blockIdx.y: sample of the read, blockIdx.z: member of the read
__global__ __launch_bounds__(kT) void tape_gather_kernel(const uint4v *__restrict__ src, uint4v *__restrict__ dst, long per16, long slot_stride16,
                                                         int slot0, int capacity, int t_base, int nt) {
    const long q = static_cast<long>(blockIdx.x) * kT + threadIdx.x;
    if (q >= per16) return;
    const long t = t_base + static_cast<long>(blockIdx.y);
    const long slot = (slot0 + t) % capacity;
    const uint4v v = stream_load(src + slot * slot_stride16 + static_cast<long>(blockIdx.z) * per16 + q);
    stream_store(dst + (static_cast<long>(blockIdx.z) * nt + t) * per16 + q, v);
}
}  // namespace

// Store the sample of the members [first, first + count) into ring slot `slot`: all planes in one launch.
// slab: [M][slab_fields][4608] fp64; store32: the physics outputs are stored as fp32; f64: the tape holds doubles (else floats,
// rounded to nearest).
static hipError_t run_tape_store(const TapePlane *planes, int nplanes, const double *slab, int slab_fields, int first, int count, int slot,
                                 int store32, int f64, hipStream_t s) {
    if (nplanes == 0 || count == 0) return hipSuccess;
    const dim3 grid(kPairs / kT, nplanes, count);
    if (f64)
        hipLaunchKernelGGL(tape_store_kernel<double>, grid, dim3(kT), 0, s, planes, slab, slab_fields, first, slot, store32);
    else
        hipLaunchKernelGGL(tape_store_kernel<float>, grid, dim3(kT), 0, s, planes, slab, slab_fields, first, slot, store32);
    return hipGetLastError();
}

hipError_t run_tape_gather(const void *src, void *dst, long per, long slot_stride, int elem_bytes, int count, int nt, int slot0,
                           int capacity, hipStream_t s) {
    if (count == 0 || nt == 0 || per == 0) return hipSuccess;
    // (a plane is 4608 elements of 4 or 8 bytes: every entry and every stride is a whole number of 16-byte pieces)
    const long per16 = per * elem_bytes / 16, stride16 = slot_stride * elem_bytes / 16;
    constexpr int kMaxY = 32768;  // (grid.y is limited to 65535: a long read goes out in pieces)
    for (int t_base = 0; t_base < nt; t_base += kMaxY) {
        const int ny = nt - t_base < kMaxY ? nt - t_base : kMaxY;
        hipLaunchKernelGGL(tape_gather_kernel, dim3(static_cast<unsigned>((per16 + kT - 1) / kT), ny, count), dim3(kT), 0, s,
                           static_cast<const uint4v *>(src), static_cast<uint4v *>(dst), per16, stride16, slot0, capacity, t_base, nt);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace spd

// ---- host side: the step loop's sample, the configuration and the C ABI (spd_model_tape_*) ----

// the sample of members [first, first + count): the front end into the tape's own slab, then the store into ring slot (n - 1) % capacity
hipError_t spd::tape_sample(spd_model *m, int first, int count, long long n, hipStream_t s) {
    const spd_model::Tape &tp = m->tape;
    hipError_t e = sample_front(m, tp, first, count, s);
    if (e == hipSuccess)
        e = run_tape_store(tp.planes, tp.nplanes, tp.slab, tp.slab_fields, first, count, tp.ring.slot(n),
                           m->stored32 ? 1 : 0, tp.dtype == SPD_TAPE_F64 ? 1 : 0, s);
    return e;
}

extern "C" {

int spd_model_tape_configure(spd_model_handle m, const char *const *names, int n_names, int every, int capacity, int dtype) {
    const char *who = "spd_model_tape_configure";
    // (the arguments first: nothing below needs the device)
    std::vector<int> ids;
    if (int rc = sample_ids(who, names, n_names, ids)) return rc;
    if (n_names > 0 && every < 1) return m_fail(SPD_E_ARG, std::string(who) + ": every must be at least 1");
    if (n_names > 0 && capacity < 1) return m_fail(SPD_E_ARG, std::string(who) + ": capacity must be at least 1");
    if (n_names > 0 && dtype != SPD_TAPE_F32 && dtype != SPD_TAPE_F64)
        return m_fail(SPD_E_ARG, std::string(who) + ": dtype must be SPD_TAPE_F32 or SPD_TAPE_F64");
    if (int rc = configure_allowed(m, who)) return rc;
    for (size_t k = 0; k < ids.size(); ++k)
        if (cat_needs_levels(ids[k]) && m->plev.n == 0)
            return levels_first(who, names[k]);
    spd_model::Tape &tp = m->tape;
    if (int rc = retire(m, tp)) return rc;
    if (n_names == 0) return SPD_OK;  // off
    spd_model::Tape next;
    next.every = every;
    next.dtype = dtype;
    const size_t M = static_cast<size_t>(m->M), elem = dtype == SPD_TAPE_F64 ? sizeof(double) : sizeof(float);
    SamplePlan plan;
    plan_sample(m, ids, next, plan);
    const size_t slots = static_cast<size_t>(capacity);
    for (const auto &v : plan.vars) next.vars.push_back({v.id, v.levels, slots * M * v.first_plane * NG});
    next.nplanes = static_cast<int>(plan.planes);
    // one allocation: ring | slab | tables[2] | plane descriptors
    const size_t per_slot = M * plan.planes * NG * elem;
    if (per_slot != 0 && slots > (static_cast<size_t>(-1) / 2) / per_slot)
        return m_fail(SPD_E_ARG, std::string(who) + ": the tape's size does not fit size_t");
    const size_t ring = sample_up(slots * per_slot), desc = sample_up(plan.planes * sizeof(TapePlane));
    const size_t total = ring + plan.slab_bytes + 2 * plan.table_bytes + desc;
    void *p = nullptr;
    if (hipMalloc(&p, total) != hipSuccess) {  // the tape is off; the model is as usable as before
        (void)hipGetLastError();
        return m_fail(SPD_E_DEVICE, std::string(who) + ": cannot allocate the tape (" + std::to_string(total) + " bytes asked for: " +
                                        std::to_string(capacity) + " samples of " + std::to_string(per_slot) + " bytes); the tape is off");
    }
    Carve carve{static_cast<char *>(p)};
    next.alloc = p;
    next.data = carve.take<char>(ring);
    carve_front(carve, plan, next);
    next.planes = carve.take<TapePlane>(desc);
    std::vector<SampleSource> sources;
    hipError_t e = build_sample_front(m, plan, next, sources);
    std::vector<TapePlane> host_planes;
    for (const auto &v : next.vars)
        for (int k = 0; k < v.levels; ++k) {
            TapePlane d{};
            d.source = sources[host_planes.size()];
            d.dst = static_cast<char *>(next.data) + (v.offset + static_cast<size_t>(k) * NG) * elem;
            d.member_stride = static_cast<long>(v.levels) * NG;
            d.slot_stride = static_cast<long>(M) * v.levels * NG;
            host_planes.push_back(d);
        }
    if (e == hipSuccess) e = hipMemcpy(next.planes, host_planes.data(), host_planes.size() * sizeof(TapePlane), hipMemcpyHostToDevice);
    if (e != hipSuccess) return upload_failed(who, e, p);
    next.ring = SampleRing(capacity, 6);
    next.on = true;
    tp = std::move(next);
    return SPD_OK;
}

int spd_model_tape_reset(spd_model_handle m) {
    return ring_reset(m, "spd_model_tape_reset", &spd_model::tape, "no tape configured (spd_model_tape_configure)");
}

int spd_model_tape_info(spd_model_handle m, long long *taken, int *held, int *capacity, int *every, int *dtype) {
    if (!m) return m_fail(SPD_E_ARG, "spd_model_tape_info: null model");
    const spd_model::Tape &tp = m->tape;
    if (!tp.on) return m_fail(SPD_E_ARG, "spd_model_tape_info: no tape configured (spd_model_tape_configure)");
    if (taken) *taken = tp.ring.taken;
    if (held) *held = static_cast<int>(tp.ring.held());
    if (capacity) *capacity = tp.ring.capacity;
    if (every) *every = tp.every;
    if (dtype) *dtype = tp.dtype;
    return SPD_OK;
}

int spd_model_tape_times(spd_model_handle m, int32_t *rows, int max_rows) {
    return ring_rows(m, "spd_model_tape_times", &spd_model::tape, "no tape configured (spd_model_tape_configure)", rows, max_rows);
}

int spd_model_tape_read(spd_model_handle m, const char *name, int first, int count, int t0, int nt, void *dst_device, size_t dst_bytes,
                        void *stream) {
    const char *who = "spd_model_tape_read";
    if (!m || !name) return m_fail(SPD_E_ARG, std::string(who) + ": null argument");
    const spd_model::Tape &tp = m->tape;
    if (int rc = read_allowed(m, who, tp.on, "no tape configured (spd_model_tape_configure)", tp.validity, "the tape is invalid until spd_model_tape_reset"))
        return rc;
    const int id = stats_id(name);
    const spd_model::Tape::Var *v = nullptr;
    for (const auto &x : tp.vars)
        if (x.id == id) v = &x;
    if (!v) return m_fail(SPD_E_ARG, std::string(who) + ": '" + name + "' is not among the configured variables");
    if (first < 0 || count < 0 || first + count > m->M) return m_fail(SPD_E_ARG, std::string(who) + ": member range out of bounds");
    if (int rc = held_range(who, tp.ring, t0, nt, "sample")) return rc;
    const size_t elem = tp.dtype == SPD_TAPE_F64 ? sizeof(double) : sizeof(float), per = static_cast<size_t>(v->levels) * NG;
    const size_t need = static_cast<size_t>(count) * static_cast<size_t>(nt) * per * elem;
    if (int rc = destination_fits(who, dst_device, dst_bytes, need, 16)) return rc;
    if (count == 0 || nt == 0) return SPD_OK;
    M_HIP(hipSetDevice(m->ctx->device));
    const char *src = static_cast<const char *>(tp.data) + (v->offset + static_cast<size_t>(first) * per) * elem;
    const hipError_t e = run_tape_gather(src, dst_device, static_cast<long>(per), static_cast<long>(static_cast<size_t>(m->M) * per),
                                         static_cast<int>(elem), count, nt, tp.ring.slot_of_held(t0), tp.ring.capacity,
                                         static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return m_fail(SPD_E_DEVICE, std::string(who) + ": " + hipGetErrorString(e));
    return SPD_OK;
}

}  // extern "C"
