// The window tape: window sums, means, extremes and threshold counts of the state's grid-space fields, accumulated behind the
// sampled steps of the device loop and closed into a ring in device memory every n steps, at midnight or at month ends
// (wintape.hip holds the kernel, the schedule, the configuration and the C ABI: spd_model_wintape_* and spd_wintape_plan
// of include/pyspeedy_amd.h; the definition is DESIGN section 4g).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "sample_source.hpp"

struct spd_model;

namespace spd {

struct Calendar;

// One plane (a level of a name) of every member, as the accumulate kernel sees it.  Accumulator and ring pointers are those of
// member 0 at this plane; a member lies member_stride elements further in the accumulators and in a ring slot alike.
struct WinTapePlane {
    SampleSource source; // where the sample's value a lies, and its unit (`src` is float only when `narrow` as well)
    int slab_b;          // second slab plane of a wind-speed name (value = sqrt(a * a + b * b)), else -1
    int narrow;          // 1: `src` is among the arrays physics_storage32 keeps as float
    double *sum;         // running sum (an entry asks for sum or mean), else null
    double *mn, *mx;     // running minimum / maximum, else null
    double *cnt[2];      // running counts of x > thr[0] / of x < thr[1], as fp64 integers, else null
    double thr[2];       // thresholds of the two counts, in the entry's own unit
    void *ring[6];       // slot 0 of the entry (name, SPD_WIN_SUM ... _COUNT_BELOW) in the ring's dtype, else null
    long member_stride;  // elements between two members (levels * 4608)
    long slot_stride;    // elements between two ring slots of an entry (M * levels * 4608)
};

// The window tape's schedule: the ONE place that decides whether a step samples and whether it closes the open window, for the step
// loop (step_impl) and for spd_wintape_plan alike.
struct WinSchedule {
    int window, every, sample_every;
};
struct WinOpen {
    int start, samples;  // the step counter the open window began at; the samples it holds
};
struct WinDecision {
    bool sample, close;
};
// The step that leaves the counter at `step_after` and the date at `next`: a sample goes into the open window first; a closing
// step then fills row[8] (spd_model_wintape_times) and opens the next window at step_after.
WinDecision wintape_advance(const WinSchedule &s, WinOpen &w, int step_after, const Calendar &next, int32_t *row);
// window kind, `every` and sample_every as every caller of the schedule refuses them: SPD_OK, or SPD_E_ARG behind the error text
int wintape_schedule_check(const char *who, int window, int every, int sample_every);

// The step loop's launches for the members [first, first + count) on a step that samples (k >= 1: the front end, then the kernel) or
// only closes (k = 0: the kernel alone); k, close, n and slot as run_wintape_step (wintape.hip) takes them.
hipError_t wintape_step(spd_model *m, int first, int count, int k, int close, int n, int slot, hipStream_t s);

}  // namespace spd
