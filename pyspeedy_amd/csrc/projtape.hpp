// The projection tape: weighted sums of the state's grid-space fields -- box and band means, global means, station values, any
// fixed linear functional of one plane -- formed behind the sampled steps of the device loop and kept as scalar time series in a
// ring in device memory (projtape.hip holds the kernel, the configuration and the C ABI:
// spd_model_projtape_* of include/pyspeedy_amd.h; the definition is DESIGN section 4j).
//
// Definition.  P weight maps w (fp64 [48][96], the layout of one level of a tape sample, shared by all members) and E entries
// (name, level, pattern).  x[p], p = 96 j + i, is what an fp64 tape of that name holds at that level after the sampled step, in
// export units.  The result of an entry is one double per member and sample, summed in this order, every product and every sum
// rounded on its own (no contraction):
//   lane t of 256:   s_t = w[t] * x[t];  for r = 1 ... 17 in that order  s_t = s_t + w[t + 256 r] * x[t + 256 r]
//   tree[t] = s_t;   for half = 128, 64, ..., 1:  tree[t] = tree[t] + tree[t + half]  for t < half;   result = tree[0]
// All 4608 = 18 * 256 terms take part; a zero weight is not skipped.  tests/projtape_reference.py restates it in numpy.
#pragma once
#include <hip/hip_runtime.h>

#include "sample_source.hpp"

struct spd_model;

namespace spd {

// One distinct plane (a level of a name) among the entries, as the kernel sees it.
struct ProjTapePlane {
    SampleSource source;  // where the sample's value lies, and its unit
    int first, count;     // its entries: items [first, first + count) of the list below
};

// One entry, in the list sorted by plane: the pattern it projects onto and its column in a member's row of the ring.
struct ProjTapeItem {
    int pattern, column;
};

#if defined(__HIPCC__)
// The tree of the definition over the 256 lane sums of `row` (LDS, complete behind a barrier), formed by one wavefront: the two
// halvings that cross wavefronts are read from the LDS by lane t < 64, the six inside the wavefront go through cross-lane moves.
// Lane 0 returns the result; a lane >= half adds something nobody reads.  (projtape_kernel, and verif_reduce_kernel of verif.hip.)
__device__ __forceinline__ double projtape_fold(const double *row, int lane) {
    double v = __dadd_rn(__dadd_rn(row[lane], row[lane + 128]), __dadd_rn(row[lane + 64], row[lane + 192]));
#pragma unroll
    for (int half = 32; half > 0; half >>= 1) v = __dadd_rn(v, __shfl_down(v, half, 64));
    return v;
}
#endif

// One launch of the projection kernel for the members [first, first + count), all planes (projtape.hip).  weights: [P][4608];
// slab: [M][slab_fields][4608] fp64, as the front end left it; store32: the model keeps precnv / precls as float; ring_slot:
// member 0 of the sample's slot, [M][n_entries].  The assimilation's observation operator is this launch into a one-slot ring.
hipError_t run_projtape_sample(const ProjTapePlane *planes, int nplanes, const ProjTapeItem *items, const double *weights, const double *slab,
                               int slab_fields, double *ring_slot, int n_entries, int first, int count, int store32, hipStream_t s);

// The step loop's sample of the members [first, first + count), number n since the last reset, behind the step just issued on `s`.
hipError_t projtape_sample(spd_model *m, int first, int count, long long n, hipStream_t s);

}  // namespace spd
