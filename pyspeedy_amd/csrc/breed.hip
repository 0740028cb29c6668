// Breeding: rescale the perturbation of a bred member against its control run (spd_model_breed_*, include/pyspeedy_amd.h;
// DESIGN section 4i).
//
// For a bred member p with control c, D = X_p - X_c on time level 1, w_m = 1 for m = 0 and 2 otherwise, over the 527 coefficients
// with m + n <= 31 of a plane (a level of vor, div, t, tr, or ps):
//   E(vor | div, k) = 1/4 sum elm2(m + n) w_m |D|^2        E(t | tr | ps, k) = 1/2 sum w_m |D|^2
//   A = sqrt(sum over the 33 planes of weight * E),  s = target / A,  X_p' = X_c + s * (X_p - X_c) on both time levels.
// Two launches.  breed_norm_kernel: a workgroup per (plane, bred member) reads the plane of both members with 16-byte loads -- a lane
// holds the coefficients k = lane, lane + 256, lane + 512, lane + 768 and adds their terms in that order -- and the 256 lane sums
// go through a tree in the LDS whose shape is fixed; one partial per plane and member is left in device scratch.  Nothing is
// atomic and nothing depends on which members are bred, on the member groups, the rounds or the call length: A is the same bits in
// every plan.  breed_rescale_kernel: shaped like nudge_kernel; every workgroup first adds its member's 33 weighted partials in
// ascending plane order (the reduce at the launch boundary: the partials are complete when this launch starts), forms A and s
// uniformly, and then moves its coefficients.  Every operation is rounded on its own (no contraction, the __d*_rn intrinsics), so
// that numpy's xc + s * (xp - xc) gives the same bits.  A coefficient with m + n >= 32 is neither loaded nor stored: a quiet member
// stays quiet.  Only bred members are written, and a control is never bred: no workgroup reads what another one writes.
#include <hip/hip_runtime.h>

#include "breed.hpp"
#include "model_state.hpp"
#include "tables.hpp"

namespace spd {

namespace {
constexpr int kT = 256;
constexpr int kBlocks = (NSPEC + kT - 1) / kT;  // 4 blocks (or 4 coefficients a lane) over the 992 coefficients
constexpr int kLmax = TRUNC + 1;                // the largest total wavenumber that takes part

typedef double double2v __attribute__((ext_vector_type(2)));

// Pointers that come out of the descriptor table are generic to the compiler; they are device-memory addresses.
__device__ __forceinline__ double2v load_global(const double *p) {
    return *(const __attribute__((address_space(1))) double2v *)p;
}
__device__ __forceinline__ void store_global(double *p, double2v v) {
    *(__attribute__((address_space(1))) double2v *)p = v;
}

// blockIdx.x: plane, blockIdx.y: bred member
__global__ __launch_bounds__(kT) void breed_norm_kernel(const BreedPlane *__restrict__ planes, const BreedPair *__restrict__ pairs,
                                                        const double *__restrict__ elm2, double *__restrict__ partial) {
#pragma clang fp contract(off)
    __shared__ double tree[kT];
    const BreedPlane d = planes[blockIdx.x];
    const BreedPair pr = pairs[blockIdx.y];
    const double *xp = d.state + pr.member * d.member_stride, *xc = d.state + pr.control * d.member_stride;
    double sum = 0.0;
    for (int j = 0; j < kBlocks; ++j) {
        const int k = j * kT + threadIdx.x;
        if (k >= NSPEC) break;
        const int n = k / MX, m = k - n * MX, l = m + n;
        if (l > kLmax) continue;
        const double2v p = load_global(xp + 2 * k), c = load_global(xc + 2 * k);
        const double dx = __dsub_rn(p.x, c.x), dy = __dsub_rn(p.y, c.y);
        double q = __dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy));
        if (m != 0) q = __dmul_rn(2.0, q);
        if (d.kinetic) q = __dmul_rn(elm2[MX * l], q);
        sum = __dadd_rn(sum, q);
    }
    tree[threadIdx.x] = sum;
    __syncthreads();
    for (int half = kT / 2; half > 0; half >>= 1) {
        if (threadIdx.x < half) tree[threadIdx.x] = __dadd_rn(tree[threadIdx.x], tree[threadIdx.x + half]);
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.y * kBreedPlanes + blockIdx.x] = __dmul_rn(d.kinetic ? 0.25 : 0.5, tree[0]);
}

// the amplitude of bred member b from its partials: ascending plane order; a plane of weight zero takes no part
__device__ __forceinline__ double amplitude_of(const BreedPlane *__restrict__ planes, const double *__restrict__ partial, int b) {
#pragma clang fp contract(off)
    double sum = 0.0;
    for (int p = 0; p < kBreedPlanes; ++p) {
        const double w = planes[p].weight;
        if (w != 0.0) sum = __dadd_rn(sum, __dmul_rn(w, partial[b * kBreedPlanes + p]));
    }
    return __dsqrt_rn(sum);
}

// blockIdx.x: coefficients, blockIdx.y: plane, blockIdx.z: bred member
__global__ __launch_bounds__(kT) void breed_rescale_kernel(const BreedPlane *__restrict__ planes, const BreedPair *__restrict__ pairs,
                                                           const double *__restrict__ partial, double target,
                                                           double *__restrict__ amplitude, double *__restrict__ factor) {
#pragma clang fp contract(off)
    const int b = blockIdx.z;
    const BreedPair pr = pairs[b];
    const double a = amplitude_of(planes, partial, b);
    const bool alone = !(a > 0.0) || !(a < __builtin_inf());  // zero or not finite: s = 1 and not one bit of the member moves
    const double s = alone ? 1.0 : __ddiv_rn(target, a);
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
        if (amplitude) amplitude[pr.member] = a;
        if (factor) factor[pr.member] = s;
    }
    if (alone) return;
    const int k = blockIdx.x * kT + threadIdx.x;
    if (k >= NSPEC) return;
    const int n = k / MX, l = k - n * MX + n;
    if (l > kLmax) return;
    const BreedPlane d = planes[blockIdx.y];
    double *p0 = d.state + pr.member * d.member_stride + 2 * k, *p1 = p0 + d.level_stride;
    const double *c0 = d.state + pr.control * d.member_stride + 2 * k, *c1 = c0 + d.level_stride;
    const double2v xc = load_global(c0), yc = load_global(c1);
    double2v x = load_global(p0), y = load_global(p1);
    x.x = __dadd_rn(xc.x, __dmul_rn(s, __dsub_rn(x.x, xc.x)));
    x.y = __dadd_rn(xc.y, __dmul_rn(s, __dsub_rn(x.y, xc.y)));
    y.x = __dadd_rn(yc.x, __dmul_rn(s, __dsub_rn(y.x, yc.x)));
    y.y = __dadd_rn(yc.y, __dmul_rn(s, __dsub_rn(y.y, yc.y)));
    store_global(p0, x);
    store_global(p1, y);
}

// a lane per member
__global__ __launch_bounds__(kT) void breed_amplitude_kernel(const BreedPlane *__restrict__ planes, const int *__restrict__ slot_of, int members,
                                                             const double *__restrict__ partial, double *__restrict__ out) {
    const int i = blockIdx.x * kT + threadIdx.x;
    if (i >= members) return;
    const int b = slot_of[i];
    out[i] = b < 0 ? 0.0 : amplitude_of(planes, partial, b);
}

}  // namespace

constexpr int kMaxZ = 32768;  // (grid.y and grid.z are limited to 65535: many bred members go out in pieces)

// The norm launch for the bred members pairs[0 ... nbred): partial[b][plane] = E(plane) of the difference X_p - X_c on time level 1,
// summed over the 527 coefficients with m + n <= 31 in an order that depends on nothing but the plane.
static hipError_t run_breed_norm(const BreedPlane *planes, const BreedPair *pairs, int nbred, const double *elm2, double *partial, hipStream_t s) {
    for (int z0 = 0; z0 < nbred; z0 += kMaxZ) {
        const int nz = nbred - z0 < kMaxZ ? nbred - z0 : kMaxZ;
        hipLaunchKernelGGL(breed_norm_kernel, dim3(kBreedPlanes, nz), dim3(kT), 0, s, planes, pairs + z0, elm2,
                           partial + static_cast<long>(z0) * kBreedPlanes);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// The rescale launch behind it.  Every workgroup sums its member's 33 weighted partials in ascending plane order:
//   A = sqrt(sum weight[plane] * partial[b][plane]),  s = target / A  (s = 1 and the member left alone if A is zero or not finite)
// and then X_p' = X_c + s * (X_p - X_c) on both time levels for the coefficients with m + n <= 31, each operation rounded on its
// own.  amplitude / factor: [M] of the ring slot, written at the member's index; either may be null.
static hipError_t run_breed_rescale(const BreedPlane *planes, const BreedPair *pairs, int nbred, const double *partial, double target,
                                    double *amplitude, double *factor, hipStream_t s) {
    for (int z0 = 0; z0 < nbred; z0 += kMaxZ) {
        const int nz = nbred - z0 < kMaxZ ? nbred - z0 : kMaxZ;
        hipLaunchKernelGGL(breed_rescale_kernel, dim3(kBlocks, kBreedPlanes, nz), dim3(kT), 0, s, planes, pairs + z0,
                           partial + static_cast<long>(z0) * kBreedPlanes, target, amplitude, factor);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// Amplitudes only, behind run_breed_norm: out[i] = A of member i, 0.0 for a member that is not bred (slot_of[i] < 0: its index in
// pairs otherwise).  Writes nothing else.
static hipError_t run_breed_amplitude(const BreedPlane *planes, const int *slot_of, int members, const double *partial, double *out, hipStream_t s) {
    if (members == 0) return hipSuccess;
    hipLaunchKernelGGL(breed_amplitude_kernel, dim3((members + kT - 1) / kT), dim3(kT), 0, s, planes, slot_of, members, partial, out);
    return hipGetLastError();
}

}  // namespace spd

// ---- host side: the step loop's rescale, the configuration and the C ABI (spd_model_breed_*, spd_breed_check) ----

namespace {
constexpr int kBreedNames = 5, kBreedRows = 8;  // weights: [5][8] for vor, div, t, tr, ps; ps reads entry 0 of its row
const char *const kBreedName[kBreedNames] = {"vor", "div", "t", "tr", "ps"};
const char *const kBreedOff = "no breeding configured (spd_model_breed_configure)";
int breed_levels(int id) { return id == 4 ? 1 : 8; }
}  // namespace

// The rescale of all bred members on the state as it stands, on stream s: the norm launch, the rescale launch behind it, one slot
// of the ring.  What the model derived from the state is dropped as spd_model_set drops it (the look-ahead geopotential, the day's
// interpolated climatologies); a range check that was put off looks at the state as it is now and goes out first.
int spd::breed_rescale(spd_model *m, hipStream_t s, const char *who) {
    spd_model::Breed &br = m->breed;
    if (br.nbred == 0) return SPD_OK;
    if (int rc = settle_deferred_check(m)) return rc;
    m->surf_cache_valid = m->phi_ahead = false;
    const size_t M = static_cast<size_t>(m->M), slot = static_cast<size_t>(br.ring.slot(br.ring.taken + 1));
    double *amplitude = br.data + slot * 2 * M;
    hipError_t e = run_breed_norm(br.planes, br.pairs, br.nbred, m->ctx->dev.elm2, br.partial, s);
    if (e == hipSuccess) e = run_breed_rescale(br.planes, br.pairs, br.nbred, br.partial, br.target, amplitude, amplitude + M, s);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return m_fail(SPD_E_DEVICE, std::string(who) + ": breeding: " + hipGetErrorString(e));
    }
    ++br.ring.taken;
    br.ring.stamp(br.ring.taken, m->current_step, m->cal);
    ++br.applied;
    return SPD_OK;
}

extern "C" {

int spd_breed_check(const int32_t *control, int members, const double *weights, double target, int every, int capacity, int in_loop) {
    const char *who = "spd_model_breed_configure";
    for (int i = 0; control && i < members; ++i) {
        const int c = control[i];
        if (c == -1) continue;
        if (c < -1 || c >= members)
            return m_fail(SPD_E_ARG, std::string(who) + ": the control of member " + std::to_string(i) + " (" + std::to_string(c) + ") is out of range (-1 ... " +
                                         std::to_string(members - 1) + ")");
        if (c == i) return m_fail(SPD_E_ARG, std::string(who) + ": member " + std::to_string(i) + " is its own control");
        if (control[c] != -1)
            return m_fail(SPD_E_ARG, std::string(who) + ": the control of member " + std::to_string(i) + " (" + std::to_string(c) +
                                         ") is itself bred: a control must have -1 (no chains)");
    }
    if (!weights) return m_fail(SPD_E_ARG, std::string(who) + ": null weights");
    bool some = false;
    for (int v = 0; v < kBreedNames; ++v)
        for (int k = 0; k < breed_levels(v); ++k) {
            const double w = weights[v * kBreedRows + k];
            if (!std::isfinite(w) || w < 0.0)
                return m_fail(SPD_E_ARG, std::string(who) + ": the weight of '" + kBreedName[v] + "' at level " + std::to_string(k) +
                                             " is not a finite number >= 0");
            some = some || w > 0.0;
        }
    if (!some) return m_fail(SPD_E_ARG, std::string(who) + ": all weights are zero");
    if (!std::isfinite(target) || !(target > 0.0)) return m_fail(SPD_E_ARG, std::string(who) + ": target must be a finite number > 0");
    if (every < 1) return m_fail(SPD_E_ARG, std::string(who) + ": every must be at least 1");
    if (capacity < 1) return m_fail(SPD_E_ARG, std::string(who) + ": capacity must be at least 1");
    if (in_loop != 0 && in_loop != 1) return m_fail(SPD_E_ARG, std::string(who) + ": in_loop must be 0 or 1");
    return SPD_OK;
}

int spd_model_breed_configure(spd_model_handle m, const int32_t *control, const double *weights, double target, int every, int capacity,
                              int in_loop) {
    const char *who = "spd_model_breed_configure";
    // (the arguments first: what does not need the member count, then the model, then the controls)
    if (control)
        if (int rc = spd_breed_check(nullptr, 0, weights, target, every, capacity, in_loop)) return rc;
    if (int rc = configure_allowed(m, who)) return rc;
    if (control)
        if (int rc = spd_breed_check(control, m->M, weights, target, every, capacity, in_loop)) return rc;
    spd_model::Breed &br = m->breed;
    if (int rc = retire(m, br)) return rc;
    if (!control) return SPD_OK;  // off
    spd_model::Breed next;
    next.in_loop = in_loop != 0;
    next.every = every;
    next.target = target;
    const size_t M = static_cast<size_t>(m->M);
    std::vector<BreedPair> pairs;
    std::vector<int> slot_of(M, -1);
    for (int i = 0; i < m->M; ++i)
        if (control[i] >= 0) {
            slot_of[i] = static_cast<int>(pairs.size());
            pairs.push_back({i, control[i]});
        }
    next.nbred = static_cast<int>(pairs.size());
    if (static_cast<size_t>(capacity) > (static_cast<size_t>(-1) / 64) / M)
        return m_fail(SPD_E_ARG, std::string(who) + ": the ring's size does not fit size_t");
    std::vector<BreedPlane> planes;
    double *const base[kBreedNames] = {m->P.vor, m->P.div, m->P.t, m->P.tr, m->P.ps};
    for (int v = 0; v < kBreedNames; ++v)
        for (int k = 0; k < breed_levels(v); ++k) {
            const size_t levels = static_cast<size_t>(breed_levels(v));
            BreedPlane d{};
            d.state = base[v] + static_cast<size_t>(k) * NSPEC * C;
            d.member_stride = static_cast<long>(2 * levels * NSPEC * C);
            d.level_stride = static_cast<long>(levels * NSPEC * C);
            d.weight = weights[v * kBreedRows + k];
            d.kinetic = v < 2 ? 1 : 0;
            planes.push_back(d);
        }
    // one allocation: plane descriptors | pairs | each member's index among the pairs | partial norms | ring
    const size_t plane_bytes = sample_up(planes.size() * sizeof(BreedPlane)), pair_bytes = sample_up(std::max<size_t>(pairs.size(), 1) * sizeof(BreedPair));
    const size_t slot_bytes = sample_up(M * sizeof(int)), partial_bytes = sample_up(std::max<size_t>(pairs.size(), 1) * kBreedPlanes * sizeof(double));
    const size_t ring_doubles = static_cast<size_t>(capacity) * 2 * M, ring_bytes = sample_up(ring_doubles * sizeof(double));
    const size_t total = plane_bytes + pair_bytes + slot_bytes + partial_bytes + ring_bytes;
    void *p = nullptr;
    if (hipMalloc(&p, total) != hipSuccess) {  // breeding is off; the model is as usable as before
        (void)hipGetLastError();
        return m_fail(SPD_E_DEVICE, std::string(who) + ": cannot allocate the ring (" + std::to_string(total) + " bytes asked for: " +
                                        std::to_string(capacity) + " events); breeding is off");
    }
    Carve carve{static_cast<char *>(p)};
    next.alloc = p;
    next.planes = carve.take<BreedPlane>(plane_bytes);
    next.pairs = carve.take<BreedPair>(pair_bytes);
    next.slot_of = carve.take<int>(slot_bytes);
    next.partial = carve.take<double>(partial_bytes);
    next.data = carve.take<double>(ring_bytes);
    std::vector<double> ring(ring_doubles);  // what a member that is not bred shows: amplitude 0.0, factor 1.0
    for (size_t slot = 0; slot < static_cast<size_t>(capacity); ++slot) {
        std::fill(ring.begin() + slot * 2 * M, ring.begin() + slot * 2 * M + M, 0.0);
        std::fill(ring.begin() + slot * 2 * M + M, ring.begin() + (slot + 1) * 2 * M, 1.0);
    }
    hipError_t e = hipMemcpy(next.planes, planes.data(), planes.size() * sizeof(BreedPlane), hipMemcpyHostToDevice);
    if (e == hipSuccess && !pairs.empty()) e = hipMemcpy(next.pairs, pairs.data(), pairs.size() * sizeof(BreedPair), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(next.slot_of, slot_of.data(), M * sizeof(int), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(next.partial, 0, partial_bytes);
    if (e == hipSuccess) e = hipMemcpy(next.data, ring.data(), ring_doubles * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return upload_failed(who, e, p);
    next.ring = SampleRing(capacity, 6);
    next.on = true;
    br = std::move(next);
    return SPD_OK;
}

int spd_model_breed_apply(spd_model_handle m, void *stream) {
    const char *who = "spd_model_breed_apply";
    if (!m) return m_fail(SPD_E_ARG, std::string(who) + ": null model");
    if (int rc = usable(m, who)) return rc;
    if (!m->breed.on) return m_fail(SPD_E_ARG, std::string(who) + ": " + kBreedOff);
    if (!m->initialized) return m_fail(SPD_E_ARG, std::string(who) + ": model state not initialized");
    if (m->steps_pending) return m_fail(SPD_E_ARG, std::string(who) + ": a checked multi-step call is in flight; end it first");
    M_HIP(hipSetDevice(m->ctx->device));
    return breed_rescale(m, static_cast<hipStream_t>(stream), who);
}

int spd_model_breed_compute(spd_model_handle m, void *dst_device, size_t dst_bytes, void *stream) {
    const char *who = "spd_model_breed_compute";
    if (!m) return m_fail(SPD_E_ARG, std::string(who) + ": null model");
    if (int rc = usable(m, who)) return rc;
    const spd_model::Breed &br = m->breed;
    if (!br.on) return m_fail(SPD_E_ARG, std::string(who) + ": " + kBreedOff);
    if (!m->initialized) return m_fail(SPD_E_ARG, std::string(who) + ": model state not initialized");
    if (m->steps_pending) return m_fail(SPD_E_ARG, std::string(who) + ": a checked multi-step call is in flight; end it first");
    const size_t need = static_cast<size_t>(m->M) * sizeof(double);
    if (int rc = destination_fits(who, dst_device, dst_bytes, need, sizeof(double))) return rc;
    M_HIP(hipSetDevice(m->ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = run_breed_norm(br.planes, br.pairs, br.nbred, m->ctx->dev.elm2, br.partial, s);
    if (e == hipSuccess) e = run_breed_amplitude(br.planes, br.slot_of, m->M, br.partial, static_cast<double *>(dst_device), s);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return m_fail(SPD_E_DEVICE, std::string(who) + ": " + hipGetErrorString(e));
    }
    return SPD_OK;
}

int spd_model_breed_read(spd_model_handle m, int what, int t0, int nt, void *dst_device, size_t dst_bytes, void *stream) {
    const char *who = "spd_model_breed_read";
    if (what != 0 && what != 1) return m_fail(SPD_E_ARG, std::string(who) + ": what is 0 (amplitude) or 1 (factor)");
    if (!m) return m_fail(SPD_E_ARG, std::string(who) + ": null model");
    if (int rc = usable(m, who)) return rc;
    const spd_model::Breed &br = m->breed;
    if (!br.on) return m_fail(SPD_E_ARG, std::string(who) + ": " + kBreedOff);
    if (m->steps_pending) return m_fail(SPD_E_ARG, std::string(who) + ": a checked multi-step call is in flight; end it first");
    if (int rc = held_range(who, br.ring, t0, nt, "event")) return rc;
    const size_t M = static_cast<size_t>(m->M), need = static_cast<size_t>(nt) * M * sizeof(double);
    if (int rc = destination_fits(who, dst_device, dst_bytes, need, sizeof(double))) return rc;
    if (nt == 0) return SPD_OK;
    M_HIP(hipSetDevice(m->ctx->device));
    // (the spectra's gather with one "member" whose entry is the M values of a slot: dst[t][i] = ring[slot(t)][what][i])
    const hipError_t e = run_spectra_gather(br.data + static_cast<size_t>(what) * M, static_cast<double *>(dst_device), m->M, static_cast<long>(2 * M), 1, nt,
                                            br.ring.slot_of_held(t0), br.ring.capacity, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return m_fail(SPD_E_DEVICE, std::string(who) + ": " + hipGetErrorString(e));
    return SPD_OK;
}

int spd_model_breed_rows(spd_model_handle m, int32_t *rows, int max_rows) {
    if (!m) return m_fail(SPD_E_ARG, "spd_model_breed_rows: null model");
    const spd_model::Breed &br = m->breed;
    if (!br.on) return m_fail(SPD_E_ARG, std::string("spd_model_breed_rows: ") + kBreedOff);
    if (max_rows < 0 || (max_rows > 0 && !rows)) return m_fail(SPD_E_ARG, "spd_model_breed_rows: bad destination");
    return br.ring.copy_rows(rows, max_rows);
}

int spd_model_breed_reset(spd_model_handle m) {
    if (!m) return m_fail(SPD_E_ARG, "spd_model_breed_reset: null model");
    if (!m->breed.on) return m_fail(SPD_E_ARG, std::string("spd_model_breed_reset: ") + kBreedOff);
    if (m->steps_pending) return m_fail(SPD_E_ARG, "spd_model_breed_reset: a checked multi-step call is in flight; end it first");
    m->breed.ring.clear();
    return SPD_OK;
}

int spd_model_breed_info(spd_model_handle m, int *bred, int *every, int *capacity, long long *taken, int *in_loop, long long *applied) {
    if (!m) return m_fail(SPD_E_ARG, "spd_model_breed_info: null model");
    const spd_model::Breed &br = m->breed;  // (a model without breeding: all zero)
    if (bred) *bred = br.nbred;
    if (every) *every = br.every;
    if (capacity) *capacity = br.ring.capacity;
    if (taken) *taken = br.ring.taken;
    if (in_loop) *in_loop = br.in_loop ? 1 : 0;
    if (applied) *applied = br.applied;
    return SPD_OK;
}

}  // extern "C"
