// What every in-loop recorder keeps on the host beside its device ring, in one place: which slot a sample lies in and which samples
// the ring still holds, the row of step and date kept beside each slot, and whether what was recorded may still be read.
//
// Samples (or closed windows, or events) are numbered from 1 since the last reset.  Sample n lies in slot (n - 1) % capacity, so a
// ring that took `taken` samples holds the last min(taken, capacity) of them, and a read addresses those from 0, the oldest first.
// Host only: nothing here touches the device, and nothing of it is done per member -- with rounds, every round issues the same
// samples into the same slots for its own members, and the host side is written once, by the first.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "surface_host.hpp"

namespace spd {

// columns 0 ... 5 of every row: the absolute step counter of a state and its date (year, month, day, hour, minute)
inline void stamp_row(int32_t *row, int step, const Calendar &at) {
    row[0] = step; row[1] = at.year; row[2] = at.month; row[3] = at.day; row[4] = at.hour; row[5] = at.minute;
}

struct SampleRing {
    int capacity = 0, width = 6;
    long long taken = 0;        // samples since the last reset
    std::vector<int32_t> rows;  // [capacity][width], written at issue time: stamp_row's six columns, then the recorder's own

    SampleRing() = default;
    SampleRing(int capacity_, int width_) : capacity(capacity_), width(width_), rows(static_cast<size_t>(capacity_) * width_, 0) {}

    long long held() const { return std::min<long long>(taken, capacity); }
    long long oldest() const { return taken - held(); }  // (sample numbers from 0)
    int slot(long long n) const { return static_cast<int>((n - 1) % capacity); }
    int slot_of_held(long long t0) const { return static_cast<int>((oldest() + t0) % capacity); }

    int32_t *row(long long n) { return rows.data() + static_cast<size_t>(width) * slot(n); }
    void stamp(long long n, int step, const Calendar &at) { stamp_row(row(n), step, at); }
    // the rows of the samples held, the oldest first, as far as `dst` has room; -> rows written
    int copy_rows(int32_t *dst, int max_rows) const {
        int n = 0;
        for (; n < held() && n < max_rows; ++n)
            std::memcpy(dst + static_cast<size_t>(width) * n, rows.data() + static_cast<size_t>(width) * slot_of_held(n), width * sizeof(int32_t));
        return n;
    }
    void clear() { taken = 0; }  // (the next sample goes into slot 0: no device work)
};

// A recorder's sample number through the rounds of a segment of the step loop: every round issues the same samples, counted on from
// what the recorder had taken when the segment began, and only the first round writes the host side.
struct SampleCursor {
    long long base = 0, count = 0;  // samples taken at the segment's start; samples of the current round
    SampleCursor() = default;
    explicit SampleCursor(long long taken) : base(taken) {}
    void rewind() { count = 0; }                   // (a new round)
    long long next() { return base + ++count; }    // the number of the sample to issue
    long long last() const { return base + count; }
    long long open() const { return base + count + 1; }  // (recorders of windows: the number the open window will close under)
    // the sample last issued has been taken at step counter `step` and date `at`: the ring counts it and keeps its row
    void commit(SampleRing &ring, bool first_round, int step, const Calendar &at) const {
        if (!first_round) return;
        ring.taken = last();
        ring.stamp(ring.taken, step, at);
    }
};

// A member that fails the range check inside a checked call leaves samples behind it that were taken from a state the model does
// not accept: the recorder refuses to be read until it is reset.
struct Validity {
    bool valid = true;
    std::string why;
    void fail(int member, int step) {
        valid = false;
        why = "member " + std::to_string(member) + " failed the range check at step " + std::to_string(step) + " of a checked call";
    }
    void clear() {
        valid = true;
        why.clear();
    }
};

}  // namespace spd
