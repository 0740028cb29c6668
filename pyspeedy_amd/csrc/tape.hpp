// The tape: a ring in device memory of the last samples of grid-space fields, recorded by the device loop of a multi-step call
// (tape.hip holds the kernels, the configuration and the C ABI: spd_model_tape_* of include/pyspeedy_amd.h; the
// definition is DESIGN section 4c).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "sample_source.hpp"

struct spd_model;

namespace spd {

// One plane (a level of a variable) of every member, as the store kernel sees it.
struct TapePlane {
    SampleSource source; // where the sample's value lies, and its unit
    void *dst;           // slot 0, member 0 of the variable at this plane (float or double: the tape's dtype)
    long member_stride;  // elements between two members of the variable (levels * 4608)
    long slot_stride;    // elements between two slots of the variable (M * levels * 4608)
};

// Unroll the ring of one variable into dst[count][nt][per] (per = levels * 4608 elements of elem_bytes): sample t of the read lies
// in slot (slot0 + t) % capacity; src: slot 0, member `first` of the variable; slot_stride in elements (M * per).
hipError_t run_tape_gather(const void *src, void *dst, long per, long slot_stride, int elem_bytes, int count, int nt, int slot0,
                           int capacity, hipStream_t s);

// The step loop's sample of the members [first, first + count), number n since the last reset, behind the step just issued on `s`.
hipError_t tape_sample(spd_model *m, int first, int count, long long n, hipStream_t s);

}  // namespace spd
