// The verification tape: bias, mean squared error, ensemble variance, CRPS and the rank histogram of a masked ensemble against a
// truth member of the same model, per entry (name, level, weight map), formed at a join of the member groups inside the device
// loop and kept in a ring in device memory (verif.hip holds the kernels, the event, the configuration and the C ABI:
// spd_model_verif_*, spd_verif_* of include/pyspeedy_amd.h; the arithmetic is verif_point.hpp; the definition is DESIGN section 4n).
#pragma once
#include <hip/hip_runtime.h>

#include "sample_source.hpp"
#include "verif_point.hpp"

struct spd_model;

namespace spd {

// One entry as the reduce kernel sees it: its plane among the distinct ones and the pattern it is weighted with.
struct VerifItem {
    int plane, pattern;
};

// One event at the model's current step counter, on stream s: the front end for the masked members and the truth, the point
// kernel over the distinct planes, the reduce kernel over the entries.  phase 0 takes the next ring slot, stamps it and leaves
// its second half blank (NaN / -1); phase 1 fills the second half of the slot phase 0 took and marks its row.  Writes nothing
// into the model.  For the step loop at the end of a segment (model.hip: step_impl) and for spd_model_verif_apply; `who` opens the
// error text.
int verif_event(spd_model *m, hipStream_t s, const char *who, int phase);

}  // namespace spd
