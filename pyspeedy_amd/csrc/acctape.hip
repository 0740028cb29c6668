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
#include "stream_store.hpp"
#include "tables.hpp"

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
__device__ __forceinline__ T stream_load_global(const T *p) {
    return __builtin_nontemporal_load((const __attribute__((address_space(1))) T *)p);
}
template <typename T>
__device__ __forceinline__ void stream_store_global(T *p, T v) {
    __builtin_nontemporal_store(v, (__attribute__((address_space(1))) T *)p);
}
__device__ __forceinline__ double2v load_global(const double *p) {
    return *(const __attribute__((address_space(1))) double2v *)p;
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

// blockIdx.x: pairs of points, blockIdx.y: plane (descriptor), blockIdx.z: member of the group
template <typename T>
__global__ __launch_bounds__(kT) void acctape_step_kernel(const AccTapePlane *__restrict__ planes, int first, int step, int close, int slot,
                                                          int store32) {
    const int p = 2 * (blockIdx.x * kT + threadIdx.x);
    if (p >= NG) return;
    const AccTapePlane d = planes[blockIdx.y];
    const long at = (first + static_cast<long>(blockIdx.z)) * d.member_stride + p;
    const long src_at = at + static_cast<long>(d.plane) * NG;
    double2v x;
    if (store32 && d.narrow) {
        const float2v f = stream_load_global(reinterpret_cast<const float2v *>(static_cast<const float *>(d.src) + src_at));
        x.x = static_cast<double>(f.x);
        x.y = static_cast<double>(f.y);
    } else {
        x = stream_load_global(reinterpret_cast<const double2v *>(static_cast<const double *>(d.src) + src_at));
    }
    const long ring_at = static_cast<long>(slot) * d.slot_stride + at;
    if (d.sum) {
        double2v acc = x;
        if (step > 1) {
            acc = load_global(d.sum + at);
            acc.x = acc.x + x.x;
            acc.y = acc.y + x.y;
        }
        if (!close) {
            store_global(d.sum + at, acc);
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
            acc = load_global(d.mn + at);
            acc.x = x.x < acc.x ? x.x : acc.x;
            acc.y = x.y < acc.y ? x.y : acc.y;
        }
        if (!close) store_global(d.mn + at, acc);
        else ring_store<T>(d.ring[2], ring_at, acc);
    }
    if (d.mx) {
        double2v acc = x;
        if (step > 1) {
            acc = load_global(d.mx + at);
            acc.x = x.x > acc.x ? x.x : acc.x;
            acc.y = x.y > acc.y ? x.y : acc.y;
        }
        if (!close) store_global(d.mx + at, acc);
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
