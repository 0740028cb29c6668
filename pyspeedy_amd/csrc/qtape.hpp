// The quantile tape: minimum, maximum, quantiles and exceedance probabilities over a masked ensemble, per grid point and entry
// (name, level, op, param), formed at a join of the member groups inside the device loop and kept in a ring in device memory
// (qtape.hip holds the kernel, the event, the configuration and the C ABI: spd_model_qtape_*, spd_qtape_* of
// include/pyspeedy_amd.h; the arithmetic is qtape_point.hpp; the definition is DESIGN section 4o).
#pragma once
#include <hip/hip_runtime.h>

#include "qtape_point.hpp"
#include "sample_source.hpp"

struct spd_model;

namespace spd {

// One distinct plane (name, level) as the kernel finds it: where its values lie, and its entries items[first ... first + count).
struct QtapePlane {
    SampleSource src;
    int first, count;
};

// One event at the model's current step counter, on stream s: the front end for the member ranges that cover the mask, then the
// point kernel over the distinct planes, which writes every entry's plane of the next ring slot.  The slot is stamped with step and
// date.  Writes nothing into the model.  For the step loop at the end of a segment (model.hip: step_impl) and for
// spd_model_qtape_apply; `who` opens the error text.
int qtape_event(spd_model *m, hipStream_t s, const char *who);

}  // namespace spd
