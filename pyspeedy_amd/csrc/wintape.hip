// Window sums, means, extremes and threshold counts of the state's grid-space fields, accumulated on the GPU behind the sampled
// steps of a multi-step call (spd_model_wintape_*, include/pyspeedy_amd.h).
//
// A sample is what an fp64 tape of the same name holds: model.hip runs the tape's front end into a slab of the recorder's own, and
// the kernel below applies export_unit (export_unit.hpp) exactly as tape_store_kernel does; precnv / precls are read where the
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

#include "export_unit.hpp"
#include "tables.hpp"
#include "wintape.hpp"

namespace spd {

namespace {
constexpr int NG = IX * IL;
constexpr int kT = 256;
constexpr int kPairs = NG / 2;  // 2304 = 9 blocks of 256 lanes: no partial block
static_assert(NG % 2 == 0 && kPairs % kT == 0, "a plane is a whole number of blocks of point pairs");

typedef double double2v __attribute__((ext_vector_type(2)));
typedef float float2v __attribute__((ext_vector_type(2)));
template <typename T> struct Pair;
template <> struct Pair<double> { using type = double2v; };
template <> struct Pair<float> { using type = float2v; };

// Pointers that come out of the descriptor table are generic to the compiler (flat loads and stores); they are device-memory
// addresses, and saying so gives the global forms.
template <typename T>
__device__ __forceinline__ void stream_store_global(T *p, T v) {
    __builtin_nontemporal_store(v, (__attribute__((address_space(1))) T *)p);
}
__device__ __forceinline__ double2v load_global(const double *p) {
    return *(const __attribute__((address_space(1))) double2v *)p;
}
__device__ __forceinline__ float2v load_global(const float *p) {
    return *(const __attribute__((address_space(1))) float2v *)p;
}
__device__ __forceinline__ void store_global(double *p, double2v v) {
    *(__attribute__((address_space(1))) double2v *)p = v;
}

template <typename T>
__device__ __forceinline__ void ring_store(void *ring, long at, double2v v) {
    using T2 = typename Pair<T>::type;
    T2 out;
    out.x = static_cast<T>(v.x);
    out.y = static_cast<T>(v.y);
    stream_store_global(reinterpret_cast<T2 *>(static_cast<T *>(ring) + at), out);
}

__device__ __forceinline__ double2v both(double v) {
    double2v r;
    r.x = v;
    r.y = v;
    return r;
}

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
        if (d.slab_a >= 0) {
            x = load_global(slab + (i * slab_fields + d.slab_a) * NG + p);
        } else if (store32 && d.narrow) {
            const float2v f = load_global(static_cast<const float *>(d.src) + i * NG + p);
            x.x = static_cast<double>(f.x);
            x.y = static_cast<double>(f.y);
        } else {
            x = load_global(static_cast<const double *>(d.src) + i * NG + p);
        }
        x.x = export_unit(x.x, d.unit);
        x.y = export_unit(x.y, d.unit);
        if (d.slab_b >= 0) {  // wind speed: u and v carry no unit conversion
            const double2v v = load_global(slab + (i * slab_fields + d.slab_b) * NG + p);
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
            acc = load_global(d.sum + at);
            if (k > 0) {
                acc.x = acc.x + x.x;
                acc.y = acc.y + x.y;
            }
        }
        if (keep) store_global(d.sum + at, acc);
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
            acc = load_global(d.mn + at);
            if (k > 0) {
                acc.x = x.x < acc.x ? x.x : acc.x;
                acc.y = x.y < acc.y ? x.y : acc.y;
            }
        }
        if (keep) store_global(d.mn + at, acc);
        if (close) ring_store<T>(d.ring[2], ring_at, n > 0 ? acc : both(nan));
    }
    if (d.mx) {
        double2v acc = x;
        if (held) {
            acc = load_global(d.mx + at);
            if (k > 0) {
                acc.x = x.x > acc.x ? x.x : acc.x;
                acc.y = x.y > acc.y ? x.y : acc.y;
            }
        }
        if (keep) store_global(d.mx + at, acc);
        if (close) ring_store<T>(d.ring[3], ring_at, n > 0 ? acc : both(nan));
    }
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        if (!d.cnt[c]) continue;
        double2v acc = both(0.0);
        if (held) acc = load_global(d.cnt[c] + at);
        if (k > 0) {
            const double t = d.thr[c];
            acc.x = acc.x + ((c == 0 ? x.x > t : x.x < t) ? 1.0 : 0.0);
            acc.y = acc.y + ((c == 0 ? x.y > t : x.y < t) ? 1.0 : 0.0);
        }
        if (keep) store_global(d.cnt[c] + at, acc);
        if (close) ring_store<T>(d.ring[4 + c], ring_at, acc);
    }
}
}  // namespace

hipError_t run_wintape_step(const WinTapePlane *planes, int nplanes, const double *slab, int slab_fields, int first, int count, int k,
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
