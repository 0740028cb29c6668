// Time series of grid-space fields recorded on the GPU inside multi-step calls (spd_model_tape_*, include/pyspeedy_amd.h).
//
// A sample is what the statistics sample (stats.hip): model.hip runs the same front end -- vort2vel, the export descriptors with a
// slab of the tape's own as destination, the pressure-level kernel with raw = 1 -- and the store kernel below applies the export
// units with export_units_kernel's fp32 literals, exactly as stats_accumulate_kernel does, and writes the value into the ring
// instead of folding it into a mean.  precnv / precls are read where the column kernel stores them, in their stored precision.
// Streaming kernels: every value is read once and written once and nothing on the device reads the ring until the host asks, so
// loads and stores carry the non-temporal hint.  Two points (16 bytes of fp64) per lane, coalesced over the 4608 points of a plane.
#include <hip/hip_runtime.h>

#include <cmath>

#include "export_unit.hpp"
#include "stream_store.hpp"
#include "tables.hpp"
#include "tape.hpp"

namespace spd {

namespace {
constexpr int NG = IX * IL;
constexpr int kT = 256;
constexpr int kPairs = NG / 2;  // 2304 = 9 blocks of 256 lanes: no partial block
static_assert(NG % 2 == 0 && kPairs % kT == 0, "a plane is a whole number of blocks of point pairs");

typedef double double2v __attribute__((ext_vector_type(2)));
typedef float float2v __attribute__((ext_vector_type(2)));
typedef unsigned int uint4v __attribute__((ext_vector_type(4)));
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

// blockIdx.x: pairs of points, blockIdx.y: plane, blockIdx.z: member of the group
template <typename T>
__global__ __launch_bounds__(kT) void tape_store_kernel(const TapePlane *__restrict__ planes, const double *__restrict__ slab, int slab_fields,
                                                        int first, int slot, int store32) {
    using T2 = typename Pair<T>::type;
    const int p = 2 * (blockIdx.x * kT + threadIdx.x);
    if (p >= NG) return;
    const TapePlane d = planes[blockIdx.y];
    const long i = first + static_cast<long>(blockIdx.z);
    double2v x;
    if (d.slab_plane >= 0) {
        x = stream_load(reinterpret_cast<const double2v *>(slab + (i * slab_fields + d.slab_plane) * NG + p));
    } else if (store32) {
        const float2v f = stream_load_global(reinterpret_cast<const float2v *>(static_cast<const float *>(d.src) + i * NG + p));
        x.x = static_cast<double>(f.x);
        x.y = static_cast<double>(f.y);
    } else {
        x = stream_load_global(reinterpret_cast<const double2v *>(static_cast<const double *>(d.src) + i * NG + p));
    }
    T2 out;
    out.x = static_cast<T>(export_unit(x.x, d.unit));
    out.y = static_cast<T>(export_unit(x.y, d.unit));
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

hipError_t run_tape_store(const TapePlane *planes, int nplanes, const double *slab, int slab_fields, int first, int count, int slot,
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
