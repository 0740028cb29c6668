// Time-mean statistics accumulated on the GPU inside multi-step calls (spd_model_stats_*, include/pyspeedy_amd.h).
//
// A sample of the prognostic variables is what spd_model_spectral2grid would leave in u_grid ... ps_grid if the call ended at
// that step: model.hip runs the same vort2vel and the same 41-entry export descriptors per member (a second table, built like
// exp_inv_table, whose destinations are a scratch slab instead of the registry's grid arrays), then the accumulate kernel below
// applies the export units with export_units_kernel's fp32 literals and updates the moments.  precnv / precls are read where
// the column kernel stores them, in their stored precision.  Everything is fp64; Welford's update keeps the variance stable
// over long periods.  Streaming kernels: one lane per grid point, coalesced over the 4608 points of a plane.
#include <hip/hip_runtime.h>

#include <cmath>

#include "model_state.hpp"
#include "stats.hpp"
#include "tables.hpp"

namespace spd {

namespace {
constexpr int kT = 256;

// blockIdx.x: points, blockIdx.y: plane, blockIdx.z: member of the group
__global__ __launch_bounds__(kT) void stats_accumulate_kernel(const StatsPlane *__restrict__ planes, const double *__restrict__ slab,
                                                              int slab_fields, int first, long long n, int store32) {
    const int p = blockIdx.x * kT + threadIdx.x;
    if (p >= NG) return;
    const StatsPlane d = planes[blockIdx.y];
    const long i = first + static_cast<long>(blockIdx.z);
    double x = with_sample_plane(d.source, slab, slab_fields, store32, i, [&](auto plane, long) { return static_cast<double>(plane[p]); });
    x = export_unit(x, d.source.unit);
    double *mean = d.mean + i * d.member_stride + p;
    double *m2 = d.m2 ? d.m2 + i * d.member_stride + p : nullptr;
    if (n == 1) {  // the first sample of a period: nothing is read (reset needs no device work)
        *mean = x;
        if (m2) *m2 = 0.0;
        return;
    }
    const double old = *mean, delta = x - old, now = old + delta / static_cast<double>(n);
    *mean = now;
    if (m2) *m2 = *m2 + delta * (x - now);
}

__global__ __launch_bounds__(kT) void stats_variance_kernel(const double *__restrict__ m2, double *__restrict__ out, long total,
                                                            double denom) {
    const long i = static_cast<long>(blockIdx.x) * kT + threadIdx.x;
    if (i < total) out[i] = m2[i] / denom;
}

// two passes over the members (mean first, then the squared deviations from it): coalesced over points
__global__ __launch_bounds__(kT) void stats_ensemble_kernel(const double *__restrict__ mean, int M, long points, int want_std,
                                                            double *__restrict__ out) {
    const long i = static_cast<long>(blockIdx.x) * kT + threadIdx.x;
    if (i >= points) return;
    double sum = 0.0;
    for (int j = 0; j < M; ++j) sum += mean[j * points + i];
    const double mu = sum / M;
    if (!want_std) {
        out[i] = mu;
        return;
    }
    double ss = 0.0;
    for (int j = 0; j < M; ++j) {
        const double d = mean[j * points + i] - mu;
        ss += d * d;
    }
    out[i] = sqrt(ss / (M - 1));  // (one member: 0 / 0, NaN, as torch.std of one value)
}
}  // namespace

// Welford update of mean / M2 for the members [first, first + count), sample number n (1-based; n == 1 starts a period).
// slab: [M][slab_fields][4608]; store32: the physics outputs are stored as fp32 (first half of their allocations).
static hipError_t run_stats_accumulate(const StatsPlane *planes, int nplanes, const double *slab, int slab_fields, int first, int count,
                                       long long n, int store32, hipStream_t s) {
    if (nplanes == 0 || count == 0) return hipSuccess;
    hipLaunchKernelGGL(stats_accumulate_kernel, dim3((NG + kT - 1) / kT, nplanes, count), dim3(kT), 0, s, planes, slab, slab_fields,
                       first, n, store32);
    return hipGetLastError();
}

// out[i] = m2[i] / (n - 1) over `total` doubles
static hipError_t run_stats_variance(const double *m2, double *out, long total, long long n, hipStream_t s) {
    if (total == 0) return hipSuccess;
    hipLaunchKernelGGL(stats_variance_kernel, dim3(static_cast<unsigned>((total + kT - 1) / kT)), dim3(kT), 0, s, m2, out, total,
                       static_cast<double>(n - 1));
    return hipGetLastError();
}

// over the M members of one variable's time means ([M][points]): the mean (std = 0) or the unbiased standard deviation (std = 1)
static hipError_t run_stats_ensemble(const double *mean, int M, long points, int std, double *out, hipStream_t s) {
    if (points == 0) return hipSuccess;
    hipLaunchKernelGGL(stats_ensemble_kernel, dim3(static_cast<unsigned>((points + kT - 1) / kT)), dim3(kT), 0, s, mean, M, points,
                       std, out);
    return hipGetLastError();
}

}  // namespace spd

// ---- host side: the step loop's sample, the configuration and the C ABI (spd_model_stats_*) ----

// the sample of members [first, first + count): the front end, then the moments
hipError_t spd::stats_sample(spd_model *m, int first, int count, long long n, hipStream_t s) {
    const spd_model::Stats &st = m->stats;
    hipError_t e = sample_front(m, st, first, count, s);
    if (e == hipSuccess) e = run_stats_accumulate(st.planes, st.nplanes, st.slab, st.slab_fields, first, count, n, m->stored32 ? 1 : 0, s);
    return e;
}

extern "C" {

int spd_model_stats_configure(spd_model_handle m, const char *const *names, int n_names, int every, int with_variance) {
    const char *who = "spd_model_stats_configure";
    // (the arguments first: nothing below needs the device)
    std::vector<int> ids;
    if (int rc = sample_ids(who, names, n_names, ids)) return rc;
    if (n_names > 0 && every < 1) return m_fail(SPD_E_ARG, std::string(who) + ": every must be at least 1");
    if (int rc = configure_allowed(m, who)) return rc;
    for (size_t k = 0; k < ids.size(); ++k)
        if (cat_needs_levels(ids[k]) && m->plev.n == 0)
            return levels_first(who, names[k]);
    spd_model::Stats &st = m->stats;
    if (int rc = retire(m, st)) return rc;
    if (n_names == 0) return SPD_OK;  // off
    spd_model::Stats next;
    next.every = every;
    next.variance = with_variance != 0;
    const size_t M = static_cast<size_t>(m->M);
    SamplePlan plan;
    plan_sample(m, ids, next, plan);
    const size_t planes = plan.planes;
    for (const auto &v : plan.vars) next.vars.push_back({v.id, v.levels, M * v.first_plane * NG});
    next.nplanes = static_cast<int>(planes);
    // one allocation: mean | m2 | slab | tables[2] | plane descriptors
    const size_t acc = sample_up(M * planes * NG * sizeof(double)), desc = sample_up(planes * sizeof(StatsPlane));
    const size_t total = acc * (next.variance ? 2 : 1) + plan.slab_bytes + 2 * plan.table_bytes + desc;
    void *p = nullptr;
    M_HIP(hipMalloc(&p, total));
    Carve carve{static_cast<char *>(p)};
    next.alloc = p;
    next.mean = carve.take<double>(acc);
    if (next.variance) next.m2 = carve.take<double>(acc);
    carve_front(carve, plan, next);
    next.planes = carve.take<StatsPlane>(desc);
    std::vector<SampleSource> sources;
    hipError_t e = build_sample_front(m, plan, next, sources);
    std::vector<StatsPlane> host_planes;
    for (const auto &v : next.vars)
        for (int k = 0; k < v.levels; ++k) {
            StatsPlane d{};
            d.source = sources[host_planes.size()];
            d.mean = next.mean + v.offset + static_cast<size_t>(k) * NG;
            d.m2 = next.variance ? next.m2 + v.offset + static_cast<size_t>(k) * NG : nullptr;
            d.member_stride = static_cast<long>(v.levels) * NG;
            host_planes.push_back(d);
        }
    if (e == hipSuccess) e = hipMemcpy(next.planes, host_planes.data(), host_planes.size() * sizeof(StatsPlane), hipMemcpyHostToDevice);
    if (e != hipSuccess) return upload_failed(who, e, p);
    next.on = true;
    st = std::move(next);
    return SPD_OK;
}

int spd_model_stats_reset(spd_model_handle m) {
    if (!m) return m_fail(SPD_E_ARG, "spd_model_stats_reset: null model");
    if (!m->stats.on) return m_fail(SPD_E_ARG, "spd_model_stats_reset: no statistics configured (spd_model_stats_configure)");
    if (m->steps_pending) return m_fail(SPD_E_ARG, "spd_model_stats_reset: a checked multi-step call is in flight; end it first");
    m->stats.samples = 0;  // (the next sample overwrites the accumulators instead of reading them: no device work)
    m->stats.validity.clear();
    return SPD_OK;
}

int spd_model_stats_samples(spd_model_handle m) {
    if (!m) return m_fail(SPD_E_ARG, "spd_model_stats_samples: null model");
    if (!m->stats.on) return m_fail(SPD_E_ARG, "spd_model_stats_samples: no statistics configured (spd_model_stats_configure)");
    return static_cast<int>(m->stats.samples);
}

// what every read checks; -> the variable's entry
static int stats_readable(spd_model *m, const char *name, const char *who, const spd_model::Stats::Var **out) {
    if (!m || !name) return m_fail(SPD_E_ARG, std::string(who) + ": null argument");
    const spd_model::Stats &st = m->stats;
    if (int rc = read_allowed(m, who, st.on, "no statistics configured (spd_model_stats_configure)", st.validity,
                              "the statistics are invalid until spd_model_stats_reset"))
        return rc;
    const int id = stats_id(name);
    for (const auto &v : st.vars)
        if (v.id == id) {
            if (st.samples == 0) return m_fail(SPD_E_ARG, std::string(who) + ": no sample taken since the statistics were (re)started");
            *out = &v;
            return SPD_OK;
        }
    return m_fail(SPD_E_ARG, std::string(who) + ": '" + name + "' is not among the configured variables");
}

int spd_model_stats_read(spd_model_handle m, const char *name, int kind, int first, int count, void *dst_device, size_t dst_bytes,
                         void *stream) {
    const char *who = "spd_model_stats_read";
    const spd_model::Stats::Var *v = nullptr;
    if (int rc = stats_readable(m, name, who, &v)) return rc;
    if (!dst_device) return m_fail(SPD_E_ARG, std::string(who) + ": null destination");
    if (first < 0 || count < 0 || first + count > m->M) return m_fail(SPD_E_ARG, std::string(who) + ": member range out of bounds");
    if (kind != SPD_STATS_MEAN && kind != SPD_STATS_VARIANCE)
        return m_fail(SPD_E_ARG, std::string(who) + ": kind must be SPD_STATS_MEAN or SPD_STATS_VARIANCE");
    const spd_model::Stats &st = m->stats;
    if (kind == SPD_STATS_VARIANCE && !st.variance) return m_fail(SPD_E_ARG, std::string(who) + ": configured without variance");
    if (kind == SPD_STATS_VARIANCE && st.samples < 2) return m_fail(SPD_E_ARG, std::string(who) + ": the variance needs two samples");
    const size_t per = static_cast<size_t>(v->levels) * NG, need = static_cast<size_t>(count) * per * sizeof(double);
    if (dst_bytes < need) return m_fail(SPD_E_SIZE, std::string(who) + ": destination too small (" + std::to_string(need) + " bytes needed)");
    if (count == 0) return SPD_OK;
    M_HIP(hipSetDevice(m->ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t at = v->offset + static_cast<size_t>(first) * per;
    if (kind == SPD_STATS_MEAN) {
        M_HIP(hipMemcpyAsync(dst_device, st.mean + at, need, hipMemcpyDeviceToDevice, s));
    } else {
        const hipError_t e = run_stats_variance(st.m2 + at, static_cast<double *>(dst_device), static_cast<long>(count * per), st.samples, s);
        if (e != hipSuccess) return m_fail(SPD_E_DEVICE, std::string(who) + ": " + hipGetErrorString(e));
    }
    return SPD_OK;
}

int spd_model_stats_ensemble(spd_model_handle m, const char *name, int kind, void *dst_device, size_t dst_bytes, void *stream) {
    const char *who = "spd_model_stats_ensemble";
    const spd_model::Stats::Var *v = nullptr;
    if (int rc = stats_readable(m, name, who, &v)) return rc;
    if (!dst_device) return m_fail(SPD_E_ARG, std::string(who) + ": null destination");
    if (kind != SPD_STATS_MEAN && kind != SPD_STATS_STD) return m_fail(SPD_E_ARG, std::string(who) + ": kind must be SPD_STATS_MEAN or SPD_STATS_STD");
    const size_t per = static_cast<size_t>(v->levels) * NG, need = per * sizeof(double);
    if (dst_bytes < need) return m_fail(SPD_E_SIZE, std::string(who) + ": destination too small (" + std::to_string(need) + " bytes needed)");
    M_HIP(hipSetDevice(m->ctx->device));
    const hipError_t e = run_stats_ensemble(m->stats.mean + v->offset, m->M, static_cast<long>(per), kind == SPD_STATS_STD ? 1 : 0,
                                            static_cast<double *>(dst_device), static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return m_fail(SPD_E_DEVICE, std::string(who) + ": " + hipGetErrorString(e));
    return SPD_OK;
}

}  // extern "C"
