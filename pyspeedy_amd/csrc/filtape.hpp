// The filter tape: window means, covariances and last values of time-filtered grid-space fields.  A cascade of second-order
// recursive sections (filter_point.hpp) runs per member and point in front of the window tape's schedule, behind the sampled steps
// of the device loop (filtape.hip holds the two kernels, the decision of a step, the configuration and the C ABI:
// spd_model_filtape_*, spd_filtape_check and spd_filtape_filter_host of include/pyspeedy_amd.h; the definition is DESIGN section 4q).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "filter_point.hpp"
#include "sample_source.hpp"
#include "wintape.hpp"

struct spd_model;

namespace spd {

struct Calendar;

// One filtered plane -- a (name, level, filter) among the entries -- of every member, as the filter kernel sees it.  Plane f of
// member i keeps its state at state[((i * F + f) * S + s) * 2 + j][4608] (S: the most sections any configured filter has; j = 0:
// s1, 1: s2) and leaves its output at y[i * F + f][4608].
struct FilTapePlane {
    SampleSource source;  // where the sample's value x lies, and its unit (`src` is float only when `narrow` as well)
    int narrow;           // 1: `src` is among the arrays physics_storage32 keeps as float
    int n_sections;       // 1 ... 4
    FilSection sec[kFilMaxSections];
};

// One entry as the accumulate kernel sees it: its accumulator is acc[i * E + e][4608], its ring [slot][M][4608] in the ring's dtype.
struct FilTapeItem {
    int plane_a, plane_b, op;  // filtered planes (b = a where the entry names none); SPD_FIL_*
    int pad;
    void *ring;                // slot 0, member 0 of the entry
};

// What a step does to the filters and to the open window, decided once on the host (filtape_advance): the decisions themselves are
// wintape_advance's, over a WinSchedule and a WinOpen of this recorder's own in which `samples` counts the COUNTED samples.
struct FilDecision {
    bool sample = false, close = false;
    int first = 0;  // the sample is filter sample 1: the sections start in their steady state and read no state
    int c = 0;      // the sample's counted number within its window (0: the step takes no counted sample)
    int n = 0;      // counted samples of the window with this step's
};
// The step that leaves the counter at `step_after` and the date at `next`: `k` (filter samples so far) and `w` move on; a closing
// step fills row[8] (spd_model_filtape_times) with the counted samples in column 6.
FilDecision filtape_advance(const WinSchedule &s, int spinup, WinOpen &w, long long &k, int step_after, const Calendar &next, int32_t *row);

// The step loop's launches for the members [first, first + count): the front end and the filter kernel when the step samples, the
// accumulate kernel when it takes a counted sample or closes (into ring slot `slot`).
hipError_t filtape_step(spd_model *m, int first, int count, const FilDecision &d, int slot, hipStream_t s);

}  // namespace spd
