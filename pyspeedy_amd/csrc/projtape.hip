// Weighted sums of the state's grid-space fields, formed on the GPU behind the sampled steps of a multi-step call and kept as
// scalar series (spd_model_projtape_*, include/pyspeedy_amd.h; the definition is in projtape.hpp and DESIGN section 4j).
//
// A sample is what an fp64 tape of the same name holds: model.hip runs the tape's front end into a slab of the recorder's own, and
// the kernel below applies export_unit (export_unit.hpp) exactly as tape_store_kernel does; precnv / precls are read where the
// column kernel stores them, in their stored precision, widened.  One 256-lane workgroup per (member, distinct plane among the
// entries): it loads its plane once, 18 values per lane at p = t + 256 r (every load of a wavefront is 512 contiguous bytes), and
// then serves every entry on that plane -- four at a time: each lane forms the lane sums of four patterns side by side, each in
// the stated order, and leaves them in LDS, and behind one barrier wavefront k folds entry k.  The fold is the stated tree: the
// two halvings that cross wavefronts (128, 64) are read from LDS by lane t < 64 as (tree[t] + tree[t + 128]) + (tree[t + 64] +
// tree[t + 192]), the six inside a wavefront (32 ... 1) are tree[t] + tree[t + half] through a cross-lane move.  A lane >= half
// adds something nobody reads: lane t < half of the next halving reads lane t + half / 2 < half.  The patterns (36 KB each, at
// most 64) are read by every workgroup and stay in cache; a plane is read from memory once, however many patterns project it.
// Every product and sum is rounded on its own (no contraction, the __d*_rn intrinsics), so that the numpy restatement gives the
// same bits whatever the launch plan.  The front end wrote the slab just before: ordinary loads.  The ring is written once and
// read by the host's gather only.
#include <hip/hip_runtime.h>

#include "export_unit.hpp"
#include "projtape.hpp"
#include "tables.hpp"

namespace spd {

namespace {
constexpr int NG = IX * IL;
constexpr int kT = 256;
constexpr int kPer = NG / kT;  // 18 points per lane
constexpr int kBatch = 4;      // entries per barrier: one per wavefront of the workgroup
static_assert(NG % kT == 0, "a plane is a whole number of passes of the workgroup");
static_assert(kBatch * 64 == kT, "one wavefront per entry of a batch");

// Pointers that come out of the descriptor table are generic to the compiler (flat loads); they are device-memory addresses.
__device__ __forceinline__ double load_global(const double *p) { return *(const __attribute__((address_space(1))) double *)p; }
__device__ __forceinline__ float load_global(const float *p) { return *(const __attribute__((address_space(1))) float *)p; }

// blockIdx.x: distinct plane (descriptor), blockIdx.y: member of the group
__global__ __launch_bounds__(kT) void projtape_kernel(const ProjTapePlane *__restrict__ planes, const ProjTapeItem *__restrict__ items,
                                                      const double *__restrict__ weights, const double *__restrict__ slab, int slab_fields,
                                                      double *__restrict__ ring_slot, int n_entries, int first, int store32) {
#pragma clang fp contract(off)
    __shared__ double tree[kBatch][kT];
    const ProjTapePlane d = planes[blockIdx.x];
    const int t = threadIdx.x;
    const long i = first + static_cast<long>(blockIdx.y);
    double x[kPer];
    if (d.slab_plane >= 0) {
        const double *src = slab + (i * slab_fields + d.slab_plane) * NG;
#pragma unroll
        for (int r = 0; r < kPer; ++r) x[r] = export_unit(src[t + kT * r], d.unit);
    } else if (store32) {
        const float *src = static_cast<const float *>(d.src) + i * NG;
#pragma unroll
        for (int r = 0; r < kPer; ++r) x[r] = export_unit(static_cast<double>(load_global(src + t + kT * r)), d.unit);
    } else {
        const double *src = static_cast<const double *>(d.src) + i * NG;
#pragma unroll
        for (int r = 0; r < kPer; ++r) x[r] = export_unit(load_global(src + t + kT * r), d.unit);
    }
    const int wave = t >> 6, lane = t & 63;
    for (int e0 = 0; e0 < d.count; e0 += kBatch) {
        const int nb = d.count - e0 < kBatch ? d.count - e0 : kBatch;
        // the four lane sums side by side, so that the loads of four patterns are in flight together (a batch of fewer entries
        // forms its last one again and stores it nowhere); each sum keeps its own stated order
        const double *w[kBatch];
        double s[kBatch];
#pragma unroll
        for (int b = 0; b < kBatch; ++b) {
            w[b] = weights + static_cast<long>(items[d.first + e0 + (b < nb ? b : nb - 1)].pattern) * NG + t;
            s[b] = __dmul_rn(w[b][0], x[0]);
        }
#pragma unroll
        for (int r = 1; r < kPer; ++r) {
#pragma unroll
            for (int b = 0; b < kBatch; ++b) s[b] = __dadd_rn(s[b], __dmul_rn(w[b][kT * r], x[r]));
        }
#pragma unroll
        for (int b = 0; b < kBatch; ++b) tree[b][t] = s[b];
        __syncthreads();
        if (wave < nb) {
            const double *row = tree[wave];
            double v = __dadd_rn(__dadd_rn(row[lane], row[lane + 128]), __dadd_rn(row[lane + 64], row[lane + 192]));
#pragma unroll
            for (int half = 32; half > 0; half >>= 1) v = __dadd_rn(v, __shfl_down(v, half, 64));
            if (lane == 0) ring_slot[i * n_entries + items[d.first + e0 + wave].column] = v;
        }
        __syncthreads();  // (the next batch overwrites the rows)
    }
}
}  // namespace

hipError_t run_projtape_sample(const ProjTapePlane *planes, int nplanes, const ProjTapeItem *items, const double *weights,
                               const double *slab, int slab_fields, double *ring_slot, int n_entries, int first, int count,
                               int store32, hipStream_t s) {
    if (nplanes == 0 || count == 0) return hipSuccess;
    hipLaunchKernelGGL(projtape_kernel, dim3(nplanes, count), dim3(kT), 0, s, planes, items, weights, slab, slab_fields, ring_slot,
                       n_entries, first, store32);
    return hipGetLastError();
}

}  // namespace spd
