// Spectra by total wavenumber and global means of the spectral state (spd_model_spectra_*, include/pyspeedy_amd.h; the definition:
// DESIGN section 4d).
//
// Everything here is a plain sum over the coefficients the step's spectral_step_kernel has just written: no transform.  A spectral
// field is complex [32 n][31 m] (k = m + 31 n), the total wavenumber of an element is l = m + n, and a bin holds
//     sum over m = 0 ... min(l, 30) of w_m |f(n = l - m, m)|^2,   w_0 = 1, w_m = 2 otherwise
// (half of it is the global area mean of f^2 at that l; the elements with m + n > 31 take no part).  One workgroup per (member,
// level) stages the planes of that level -- vorticity, divergence, temperature, humidity: 4 x 15 872 B -- into the LDS with
// coalesced 16-byte loads; a ninth workgroup per member does the same for ln ps.  Then 32 lanes per quantity walk one diagonal
// each of the LDS copy, m ascending, with plain fp64 adds in one lane: no atomics, no cross-lane reduction, nothing that depends
// on the launch plan, so a sample is the same bits whatever the member groups, the rounds or the call length.  The products and
// the adds are separate statements: under -ffp-contract=on (Makefile) nothing is fused, and without fast-math nothing reordered.
//
// LDS banks: lane l reads element 31 l - 30 m at step m, a 16-byte read at a lane stride of 31 x 16 B = 124 dwords = -4 modulo the
// 64 banks.  A 16-byte LDS read is served in groups of 16 lanes whose lane numbers are all different modulo 16, so the 16 reads of
// a group fall on the 16 different 4-bank slots of the bank row: the walk is free of conflicts with the row left at 31 elements.
#include <hip/hip_runtime.h>

#include "global_mem.hpp"
#include "model_state.hpp"
#include "spectra.hpp"
#include "tables.hpp"

namespace spd {

namespace {
constexpr int kT = 128;            // 4 quantities x 32 bins
constexpr int kLevelSlots = KX + 1;  // blockIdx.x: the eight levels, then ln ps
constexpr double kRootHalf = 0.70710678118654752440;
static_assert(kSpectraBins == NX && kT == 4 * kSpectraBins, "a lane per bin, 32 lanes per quantity");
static_assert(4 * NSPEC * 16 <= 64 * 1024, "the four planes of a level fit the static LDS limit");

__device__ __forceinline__ void stage(double2v *lds, const double *__restrict__ plane) {
    const double2v *src = reinterpret_cast<const double2v *>(plane);
    for (int e = threadIdx.x; e < NSPEC; e += kT) lds[e] = src[e];
}

// the bin l of a staged plane: m ascending, one lane
__device__ __forceinline__ double bin_sum(const double2v *lds, int l) {
    const int last = l < MX - 1 ? l : MX - 1;
    double sum = 0.0;
    for (int m = 0; m <= last; ++m) {
        const double2v c = lds[(l - m) * MX + m];
        const double re2 = c.x * c.x;
        const double im2 = c.y * c.y;
        const double p = re2 + im2;
        const double wp = m == 0 ? p : 2.0 * p;
        sum = sum + wp;
    }
    return sum;
}

// blockIdx.x: level (KX: ln ps), blockIdx.y: member of the launch
__global__ __launch_bounds__(kT) void spectra_kernel(const SpectraArgs a) {
    __shared__ double2v lds[4][NSPEC];
    const int slot = blockIdx.x;
    const long i = a.first + static_cast<long>(blockIdx.y);
    const long o = i - a.out_first;
    const int q = threadIdx.x / kSpectraBins, l = threadIdx.x % kSpectraBins;
    const bool rot = a.mask & (1u << SPECTRA_KE_ROT), dvg = a.mask & (1u << SPECTRA_KE_DIV), tsp = a.mask & (1u << SPECTRA_T),
               qsp = a.mask & (1u << SPECTRA_Q), psp = a.mask & (1u << SPECTRA_LNPS), tmn = a.mask & (1u << SPECTRA_T_MEAN),
               qmn = a.mask & (1u << SPECTRA_Q_MEAN), pmn = a.mask & (1u << SPECTRA_LNPS_MEAN);
    if (slot == KX) {  // ln ps: one plane per member
        if (!psp && !pmn) return;
        const double *src = a.ps + i * (2L * NSPEC * 2);
        if (psp) {
            stage(lds[0], src);
            __syncthreads();
            if (q == 0) a.out[SPECTRA_LNPS][o * kSpectraBins + l] = 0.5 * bin_sum(lds[0], l);
        }
        if (pmn && threadIdx.x == 0) a.out[SPECTRA_LNPS_MEAN][o] = src[0] * kRootHalf;
        return;
    }
    if (!(a.mask & ~((1u << SPECTRA_LNPS) | (1u << SPECTRA_LNPS_MEAN)))) return;
    const long plane = (i * 2L * KX + slot) * (NSPEC * 2L);  // time level 1, this level
    if (rot) stage(lds[0], a.vor + plane);
    if (dvg) stage(lds[1], a.div + plane);
    if (tsp) stage(lds[2], a.t + plane);
    if (qsp) stage(lds[3], a.tr + plane);
    __syncthreads();
    const long at = (o * KX + slot) * kSpectraBins + l;
    if (q == 0 && rot) a.out[SPECTRA_KE_ROT][at] = 0.25 * (a.elm2[MX * l] * bin_sum(lds[0], l));
    if (q == 1 && dvg) a.out[SPECTRA_KE_DIV][at] = 0.25 * (a.elm2[MX * l] * bin_sum(lds[1], l));
    if (q == 2 && tsp) a.out[SPECTRA_T][at] = 0.5 * bin_sum(lds[2], l);
    if (q == 3 && qsp) a.out[SPECTRA_Q][at] = 0.5 * bin_sum(lds[3], l);
    if (tmn && threadIdx.x == 2 * kSpectraBins) a.out[SPECTRA_T_MEAN][o * KX + slot] = a.t[plane] * kRootHalf;
    if (qmn && threadIdx.x == 3 * kSpectraBins) a.out[SPECTRA_Q_MEAN][o * KX + slot] = a.tr[plane] * kRootHalf;
}

// blockIdx.x: sample of the read, blockIdx.y: member of the read; a lane per double of the entry
__global__ __launch_bounds__(256) void spectra_gather_kernel(const double *__restrict__ src, double *__restrict__ dst, int per, long slot_stride,
                                                             int slot0, int capacity, int nt) {
    const long t = blockIdx.x, z = blockIdx.y;
    const long slot = (slot0 + t) % capacity;
    for (int e = threadIdx.x; e < per; e += 256) dst[(z * nt + t) * per + e] = src[slot * slot_stride + z * per + e];
}
}  // namespace

// One launch for the members [first, first + count): every name of the mask.
static hipError_t run_spectra(const SpectraArgs &args, int count, hipStream_t s) {
    if (count == 0 || args.mask == 0) return hipSuccess;
    hipLaunchKernelGGL(spectra_kernel, dim3(kLevelSlots, count), dim3(kT), 0, s, args);
    return hipGetLastError();
}

hipError_t run_spectra_gather(const double *src, double *dst, int per, long slot_stride, int count, int nt, int slot0, int capacity,
                              hipStream_t s) {
    if (count == 0 || nt == 0 || per == 0) return hipSuccess;
    constexpr int kMaxY = 32768;  // (grid.y is limited to 65535: a read of many members goes out in pieces)
    for (int z0 = 0; z0 < count; z0 += kMaxY) {
        const int ny = count - z0 < kMaxY ? count - z0 : kMaxY;
        hipLaunchKernelGGL(spectra_gather_kernel, dim3(nt, ny), dim3(256), 0, s, src + static_cast<long>(z0) * per,
                           dst + static_cast<long>(z0) * nt * per, per, slot_stride, slot0, capacity, nt);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace spd

// ---- host side: the step loop's sample, the configuration and the C ABI (spd_model_spectra_*) ----

namespace {
constexpr const char *kSpectraNames[SPECTRA_NNAMES] = {"ke_rot_spectrum", "ke_div_spectrum", "t_spectrum", "q_spectrum",
                                                       "lnps_spectrum",   "t_mean",          "q_mean",     "lnps_mean"};
int spectra_id(const char *name) {
    for (int v = 0; name && v < SPECTRA_NNAMES; ++v)
        if (std::strcmp(name, kSpectraNames[v]) == 0) return v;
    return -1;
}

// the list of names of a call -> ids, in the order given (the arguments first: nothing here needs the device or a model)
int spectra_ids(const char *who, const char *const *names, int n_names, std::vector<int> &ids) {
    if (n_names < 0 || (n_names > 0 && !names)) return m_fail(SPD_E_ARG, std::string(who) + ": bad list of names");
    for (int k = 0; k < n_names; ++k) {
        const int id = spectra_id(names[k]);
        if (id < 0)
            return m_fail(SPD_E_ARG, std::string(who) + ": unknown name '" + (names[k] ? names[k] : "(null)") +
                                         "' (ke_rot_spectrum, ke_div_spectrum, t_spectrum, q_spectrum, lnps_spectrum, t_mean, q_mean, "
                                         "lnps_mean)");
        if (std::find(ids.begin(), ids.end(), id) != ids.end())
            return m_fail(SPD_E_ARG, std::string(who) + ": name '" + names[k] + "' given twice");
        ids.push_back(id);
    }
    return SPD_OK;
}

// the kernel's arguments but for the destinations: the members [first, first + count) of the state as it stands
SpectraArgs spectra_args(const spd_model *m, unsigned mask, int first, int out_first) {
    SpectraArgs a{};
    a.vor = m->P.vor, a.div = m->P.div, a.t = m->P.t, a.tr = m->P.tr, a.ps = m->P.ps;
    a.elm2 = m->ctx->dev.elm2;
    a.mask = mask, a.first = first, a.out_first = out_first;
    return a;
}
}  // namespace

// a sample: one launch for the group's members, straight into ring slot (n - 1) % capacity
hipError_t spd::spectra_sample(spd_model *m, int first, int count, long long n, hipStream_t s) {
    const spd_model::Spectra &sp = m->spectra;
    const size_t M = static_cast<size_t>(m->M), slot = static_cast<size_t>(sp.ring.slot(n));
    SpectraArgs a = spectra_args(m, sp.mask, first, 0);
    for (int v = 0; v < SPECTRA_NNAMES; ++v)
        if (sp.mask & (1u << v)) a.out[v] = static_cast<double *>(sp.alloc) + sp.offset[v] + slot * M * spectra_per_member(v);
    return run_spectra(a, count, s);
}

extern "C" {

int spd_model_spectra_configure(spd_model_handle m, const char *const *names, int n_names, int every, int capacity) {
    const char *who = "spd_model_spectra_configure";
    // (the arguments first: nothing below needs the device)
    std::vector<int> ids;
    if (int rc = spectra_ids(who, names, n_names, ids)) return rc;
    if (n_names > 0 && every < 1) return m_fail(SPD_E_ARG, std::string(who) + ": every must be at least 1");
    if (n_names > 0 && capacity < 1) return m_fail(SPD_E_ARG, std::string(who) + ": capacity must be at least 1");
    if (int rc = configure_allowed(m, who)) return rc;
    spd_model::Spectra &sp = m->spectra;
    if (int rc = retire(m, sp)) return rc;
    if (n_names == 0) return SPD_OK;  // off
    spd_model::Spectra next;
    next.every = every;
    const size_t M = static_cast<size_t>(m->M), slots = static_cast<size_t>(capacity);
    size_t per_slot = 0;  // doubles of a sample
    for (int id : ids) {
        next.mask |= 1u << id;
        per_slot += M * spectra_per_member(id);
    }
    if (slots > (static_cast<size_t>(-1) / 2) / (per_slot * sizeof(double)))
        return m_fail(SPD_E_ARG, std::string(who) + ": the size of the series does not fit size_t");
    size_t at = 0;
    for (int v = 0; v < SPECTRA_NNAMES; ++v)
        if (next.mask & (1u << v)) {
            next.offset[v] = at;
            at += slots * M * spectra_per_member(v);
        }
    const size_t total = sample_up(at * sizeof(double));
    void *p = nullptr;
    if (hipMalloc(&p, total) != hipSuccess) {  // the spectra are off; the model is as usable as before
        (void)hipGetLastError();
        return m_fail(SPD_E_DEVICE, std::string(who) + ": cannot allocate the series (" + std::to_string(total) + " bytes asked for: " +
                                        std::to_string(capacity) + " samples of " + std::to_string(per_slot * sizeof(double)) +
                                        " bytes); the spectra are off");
    }
    next.alloc = p;
    next.ring = SampleRing(capacity, 6);
    next.on = true;
    sp = std::move(next);
    return SPD_OK;
}

int spd_model_spectra_reset(spd_model_handle m) {
    return ring_reset(m, "spd_model_spectra_reset", &spd_model::spectra, "no spectra configured (spd_model_spectra_configure)");
}

int spd_model_spectra_info(spd_model_handle m, long long *taken, int *held, int *capacity, int *every) {
    if (!m) return m_fail(SPD_E_ARG, "spd_model_spectra_info: null model");
    const spd_model::Spectra &sp = m->spectra;
    if (!sp.on) return m_fail(SPD_E_ARG, "spd_model_spectra_info: no spectra configured (spd_model_spectra_configure)");
    if (taken) *taken = sp.ring.taken;
    if (held) *held = static_cast<int>(sp.ring.held());
    if (capacity) *capacity = sp.ring.capacity;
    if (every) *every = sp.every;
    return SPD_OK;
}

int spd_model_spectra_times(spd_model_handle m, int32_t *rows, int max_rows) {
    return ring_rows(m, "spd_model_spectra_times", &spd_model::spectra, "no spectra configured (spd_model_spectra_configure)", rows, max_rows);
}

int spd_model_spectra_read(spd_model_handle m, const char *name, int first, int count, int t0, int nt, void *dst_device, size_t dst_bytes,
                           void *stream) {
    const char *who = "spd_model_spectra_read";
    if (!m || !name) return m_fail(SPD_E_ARG, std::string(who) + ": null argument");
    const spd_model::Spectra &sp = m->spectra;
    if (int rc = read_allowed(m, who, sp.on, "no spectra configured (spd_model_spectra_configure)", sp.validity,
                              "the spectra are invalid until spd_model_spectra_reset"))
        return rc;
    const int id = spectra_id(name);
    if (id < 0 || !(sp.mask & (1u << id))) return m_fail(SPD_E_ARG, std::string(who) + ": '" + name + "' is not among the configured names");
    if (first < 0 || count < 0 || first + count > m->M) return m_fail(SPD_E_ARG, std::string(who) + ": member range out of bounds");
    if (int rc = held_range(who, sp.ring, t0, nt, "sample")) return rc;
    const size_t per = static_cast<size_t>(spectra_per_member(id));
    const size_t need = static_cast<size_t>(count) * static_cast<size_t>(nt) * per * sizeof(double);
    if (int rc = destination_fits(who, dst_device, dst_bytes, need, sizeof(double))) return rc;
    if (count == 0 || nt == 0) return SPD_OK;
    M_HIP(hipSetDevice(m->ctx->device));
    const double *src = static_cast<const double *>(sp.alloc) + sp.offset[id] + static_cast<size_t>(first) * per;
    const hipError_t e = run_spectra_gather(src, static_cast<double *>(dst_device), static_cast<int>(per),
                                            static_cast<long>(static_cast<size_t>(m->M) * per), count, nt,
                                            sp.ring.slot_of_held(t0), sp.ring.capacity, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return m_fail(SPD_E_DEVICE, std::string(who) + ": " + hipGetErrorString(e));
    return SPD_OK;
}

int spd_model_spectra_compute(spd_model_handle m, const char *const *names, int n_names, int first, int count, void *dst_device,
                              size_t dst_bytes, void *stream) {
    const char *who = "spd_model_spectra_compute";
    std::vector<int> ids;
    if (int rc = spectra_ids(who, names, n_names, ids)) return rc;
    if (int rc = member_range(m, first, count, who)) return rc;
    if (!m->initialized) return m_fail(SPD_E_ARG, std::string(who) + ": model state not initialized");
    if (m->steps_pending) return m_fail(SPD_E_ARG, std::string(who) + ": a checked multi-step call is in flight; end it first");
    size_t per = 0;
    for (int id : ids) per += static_cast<size_t>(spectra_per_member(id));
    const size_t need = static_cast<size_t>(count) * per * sizeof(double);
    if (int rc = destination_fits(who, dst_device, dst_bytes, need, sizeof(double))) return rc;
    if (need == 0) return SPD_OK;
    M_HIP(hipSetDevice(m->ctx->device));
    SpectraArgs a = spectra_args(m, 0, first, first);
    double *at = static_cast<double *>(dst_device);
    for (int id : ids) {  // [count][...] per name, one after the other in the order given
        a.mask |= 1u << id;
        a.out[id] = at;
        at += static_cast<size_t>(count) * spectra_per_member(id);
    }
    const hipError_t e = run_spectra(a, count, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return m_fail(SPD_E_DEVICE, std::string(who) + ": " + hipGetErrorString(e));
    return SPD_OK;
}

}  // extern "C"
