// What the recorders that are configured by a list of entries -- (name, level, ...) -- and a member mask build from those lists on
// the host: the masked members with their runs of consecutive indices, and the table of the distinct planes among the entries
// (the projection tape, the assimilation, the verification tape and the quantile tape).  Nothing here needs
// HIP, a model or the catalogue: tests/sanitize/entry_front_sanitize.cpp includes this file into a plain C++ program.  The checks
// of the same lists, which need the model and its error text, lie in model_state.hpp ("the entry recorders").
#pragma once
#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

namespace spd {

struct MemberSet {
    std::vector<int> members;                 // a_0 < ... < a_(r-1): the indices with mask 1
    std::vector<std::pair<int, int>> ranges;  // (first, count): the maximal runs of consecutive indices among them and `also`
};
// mask: [M] of 0 / 1; also: one more member whose planes the front end has to prepare (the verification tape's truth), or -1
inline MemberSet member_set(const int32_t *mask, int M, int also = -1) {
    MemberSet set;
    for (int i = 0; i < M; ++i) {
        if (mask[i]) set.members.push_back(i);
        if (!mask[i] && i != also) continue;
        if (set.ranges.empty() || set.ranges.back().first + set.ranges.back().second != i) set.ranges.push_back({i, 0});
        ++set.ranges.back().second;
    }
    return set;
}

struct EntryPlanes {
    std::vector<int> ids;                       // the names among the entries in the order they first appear (the sample plan's)
    std::vector<std::pair<int, int>> distinct;  // the (name, level) planes among them in the order they first appear
    std::vector<int> plane_of;                  // [E]: entry k reads distinct[plane_of[k]]
    // the entries of plane q in the caller's order: f(k) for every k with plane_of[k] == q, ascending
    template <class F>
    void each_entry_of(size_t q, F f) const {
        for (size_t k = 0; k < plane_of.size(); ++k)
            if (plane_of[k] == static_cast<int>(q)) f(static_cast<int>(k));
    }
};
// entries: anything with .name (a catalogue id) and .level
template <class Entry>
EntryPlanes entry_planes(const std::vector<Entry> &entries) {
    EntryPlanes t;
    for (const Entry &e : entries) {
        if (std::find(t.ids.begin(), t.ids.end(), e.name) == t.ids.end()) t.ids.push_back(e.name);
        const std::pair<int, int> key{e.name, e.level};
        const auto at = std::find(t.distinct.begin(), t.distinct.end(), key);
        t.plane_of.push_back(static_cast<int>(at - t.distinct.begin()));
        if (at == t.distinct.end()) t.distinct.push_back(key);
    }
    return t;
}

}  // namespace spd
