// The accumulation tape: window sums, means and extremes of the column physics' 2-D outputs, accumulated behind every step of the
// device loop and closed into a ring in device memory (acctape.hip holds the kernel, the configuration and the C ABI:
// spd_model_acctape_* of include/pyspeedy_amd.h; the definition is DESIGN section 4f).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace spd {

// One plane of a name, of every member, as the accumulate kernel sees it.  Accumulator and ring pointers are those of member 0 at
// this plane, `src` that of member 0 at plane 0 (its element size is known at the step only); a member lies member_stride elements
// further in the source, the accumulators and a ring slot alike (planes * 4608).
struct AccTapePlane {
    const void *src;     // where the column kernel stores the name (double, or float when `narrow` and the model stores fp32)
    double *sum;         // running sum (an entry asks for sum or mean), else null
    double *mn, *mx;     // running minimum / maximum, else null
    void *ring[4];       // slot 0 of the entry (name, SPD_ACC_SUM / _MEAN / _MIN / _MAX) in the ring's dtype, else null
    long member_stride;  // elements between two members
    long slot_stride;    // elements between two ring slots of an entry (M * planes * 4608)
    int narrow;          // 1: the source is among the arrays physics_storage32 keeps as float
    int plane;           // this plane within the name (land / sea / weighted for the three-plane names)
};

// One step of the members [first, first + count), all planes in one launch.  step: number of this step within its window, from 1
// (1 overwrites the accumulators and reads none of them); close: the step ends the window, whose results (sum, sum / step, min,
// max) go into ring slot `slot`; store32: the model keeps the narrow sources as float; f64: the ring holds doubles (else floats,
// rounded to nearest).
hipError_t run_acctape_step(const AccTapePlane *planes, int nplanes, int first, int count, int step, int close, int slot, int store32,
                            int f64, hipStream_t s);

}  // namespace spd
