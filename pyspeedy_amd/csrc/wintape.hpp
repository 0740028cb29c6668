// The window tape: window sums, means, extremes and threshold counts of the state's grid-space fields, accumulated behind the
// sampled steps of the device loop and closed into a ring in device memory every n steps, at midnight or at month ends
// (wintape.hip holds the kernel, model.hip the schedule, the configuration and the C ABI: spd_model_wintape_* and spd_wintape_plan
// of include/pyspeedy_amd.h; the definition is DESIGN section 4g).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace spd {

// One plane (a level of a name) of every member, as the accumulate kernel sees it.  Accumulator and ring pointers are those of
// member 0 at this plane; a member lies member_stride elements further in the accumulators and in a ring slot alike.
struct WinTapePlane {
    const void *src;     // physics output of member 0 (slab_a < 0: precnv / precls; float when `narrow` and the model stores fp32)
    int slab_a;          // plane inside a member's slab entries (-1: read `src` directly)
    int slab_b;          // second slab plane of a wind-speed name (value = sqrt(a * a + b * b)), else -1
    int unit;            // 0 as it is, 1 q (kg/kg), 2 phi (m), 3 ps (Pa) -- export_unit.hpp, as TapePlane::unit
    int narrow;          // 1: `src` is among the arrays physics_storage32 keeps as float
    double *sum;         // running sum (an entry asks for sum or mean), else null
    double *mn, *mx;     // running minimum / maximum, else null
    double *cnt[2];      // running counts of x > thr[0] / of x < thr[1], as fp64 integers, else null
    double thr[2];       // thresholds of the two counts, in the entry's own unit
    void *ring[6];       // slot 0 of the entry (name, SPD_WIN_SUM ... _COUNT_BELOW) in the ring's dtype, else null
    long member_stride;  // elements between two members (levels * 4608)
    long slot_stride;    // elements between two ring slots of an entry (M * levels * 4608)
};

// One launch for the members [first, first + count), all planes.  k: number of this launch's sample within its window, from 1
// (1 overwrites the accumulators and reads none of them); 0: the step is not sampled and the launch only closes.  close: the step
// ends the window, whose n samples (this one included) give the results that go into ring slot `slot`; n = 0 closes an empty
// window (sum and counts 0, mean, minimum and maximum quiet NaN) and reads no accumulator.  slab: [M][slab_fields][4608] fp64, as
// the front end left it; store32: the model keeps the narrow sources as float; f64: the ring holds doubles (else floats, rounded to
// nearest).
hipError_t run_wintape_step(const WinTapePlane *planes, int nplanes, const double *slab, int slab_fields, int first, int count, int k,
                            int close, int n, int slot, int store32, int f64, hipStream_t s);

}  // namespace spd
