// The track tape: the minimum or maximum of a plane of the state's grid-space fields over a region, and where it lies -- how deep
// the low is and where, the jet or rain maximum --, followed from sample to sample, formed behind the sampled steps of the device
// loop and kept as (value, index, two sub-grid offsets) per member and entry in a ring in device memory (tracktape.hip holds the
// kernel, the configuration and the C ABI: spd_model_tracktape_* of include/pyspeedy_amd.h; the definition is DESIGN section 4p).
//
// Definition.  R regions (fp64 [48][96], the projection tape's weight maps, shared by all members; a point belongs to a region
// where its weight is not zero; kept on the device as one byte per point) and E entries (name, level, region, op, radius).  x[p],
// p = 96 j + i, is what an fp64 tape of that name holds at that level after the sampled step, in export units.  Per member m and
// entry e the follow-state last[m][e] is -1 or the index of the winner of the sample before.  A sample is steps 1 ... 3 of
// track_point.hpp with prev = last[m][e]; the ring slot gets the four doubles (value, p, di, dj) and last[m][e] = p (-1 when
// nothing was found).  The order (value, p) is total, so the result does not depend on the reduction tree or the launch plan;
// tests/tracktape_reference.py restates it in numpy.
#pragma once
#include <hip/hip_runtime.h>

#include "sample_source.hpp"
#include "track_point.hpp"

struct spd_model;

namespace spd {

// One distinct plane (a level of a name) among the entries, as the kernel sees it.
struct TrackTapePlane {
    SampleSource source;  // where the sample's value lies, and its unit
    int first, count;     // its entries: items [first, first + count) of the list below
};

// One entry, in the list sorted by plane: its region, its column in a member's row of the ring and of `last`, op and radius.
struct TrackTapeItem {
    int region, column, op, radius;
};

// One launch of the track kernel for the members [first, first + count), all planes (tracktape.hip).  masks: [R][4608] bytes;
// slab: [M][slab_fields][4608] fp64, as the front end left it; store32: the model keeps precnv / precls as float; ring_slot: member
// 0 of the sample's slot, [M][n_entries][4]; last: [M][n_entries], read and written.
hipError_t run_tracktape_sample(const TrackTapePlane *planes, int nplanes, const TrackTapeItem *items, const unsigned char *masks,
                                const double *slab, int slab_fields, double *ring_slot, int *last, int n_entries, int first, int count,
                                int store32, hipStream_t s);

// The step loop's sample of the members [first, first + count), number n since the last reset, behind the step just issued on `s`.
hipError_t tracktape_sample(spd_model *m, int first, int count, long long n, hipStream_t s);
// spd_model_init: every entry of every member follows nothing (no-op while the recorder is off).  The device is idle.
hipError_t tracktape_unseed(spd_model *m);

}  // namespace spd
