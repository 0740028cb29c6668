// AddressSanitizer / UndefinedBehaviorSanitizer driver for the host tables of the entry recorders (pyspeedy_amd/csrc/entry_front.hpp:
// member_set, entry_planes and EntryPlanes::each_entry_of).  The results are compared with restatements written here -- set
// membership plus a linear scan for the runs, nested loops for first appearance -- not with the routines under test.  Compiled by
// tests/test_entry_front_sanitize.py with g++ -fsanitize=address,undefined; the header needs neither HIP nor a model.
#include <cstdint>
#include <cstdio>
#include <utility>
#include <vector>

#include "entry_front.hpp"

using namespace spd;

static long checks = 0;
#define REQUIRE(cond, ...)                                             \
    do {                                                               \
        ++checks;                                                      \
        if (!(cond)) {                                                 \
            std::printf("FAILED %s:%d  %s\n  ", __FILE__, __LINE__, #cond); \
            std::printf(__VA_ARGS__);                                  \
            std::printf("\n");                                         \
            return false;                                              \
        }                                                              \
    } while (0)

// ---- member_set ----
static bool mask_case(const char *what, const std::vector<int32_t> &mask_in, int also) {
    const int M = static_cast<int>(mask_in.size());
    // a heap block of exactly M values, so that a read beyond the mask is caught
    int32_t *mask = new int32_t[M];
    for (int i = 0; i < M; ++i) mask[i] = mask_in[i];
    const MemberSet set = member_set(mask, M, also);
    delete[] mask;
    // the definition again: the set, member by member
    std::vector<char> in_set(M, 0);
    int r = 0;
    for (int i = 0; i < M; ++i) {
        in_set[i] = mask_in[i] == 1 || i == also;
        r += mask_in[i] == 1;
    }
    REQUIRE(static_cast<int>(set.members.size()) == r, "%s M %d also %d: %zu members, %d ones", what, M, also, set.members.size(), r);
    for (size_t j = 0; j < set.members.size(); ++j) {
        REQUIRE(set.members[j] >= 0 && set.members[j] < M && mask_in[set.members[j]] == 1, "%s M %d also %d: member %d", what, M, also, set.members[j]);
        REQUIRE(j == 0 || set.members[j - 1] < set.members[j], "%s M %d also %d: members not ascending at %zu", what, M, also, j);
    }
    // the runs by a linear scan: a run starts where i is in the set and i - 1 is not, and ends in front of the next index outside it
    std::vector<std::pair<int, int>> want;
    for (int i = 0; i < M; ++i) {
        if (!in_set[i] || (i > 0 && in_set[i - 1])) continue;
        int n = 0;
        while (i + n < M && in_set[i + n]) ++n;
        want.push_back({i, n});
    }
    REQUIRE(set.ranges == want, "%s M %d also %d: %zu runs, restated %zu", what, M, also, set.ranges.size(), want.size());
    // ... and the properties themselves: disjoint, ascending, maximal, covering exactly the set
    std::vector<int> covered(M, 0);
    for (size_t j = 0; j < set.ranges.size(); ++j) {
        const int first = set.ranges[j].first, count = set.ranges[j].second;
        REQUIRE(count >= 1 && first >= 0 && first + count <= M, "%s M %d also %d: run (%d, %d)", what, M, also, first, count);
        REQUIRE(j == 0 || set.ranges[j - 1].first + set.ranges[j - 1].second < first, "%s M %d also %d: run %zu touches the one before", what, M, also, j);
        REQUIRE(first == 0 || !in_set[first - 1], "%s M %d also %d: run %zu is not maximal below", what, M, also, j);
        REQUIRE(first + count == M || !in_set[first + count], "%s M %d also %d: run %zu is not maximal above", what, M, also, j);
        for (int i = first; i < first + count; ++i) ++covered[i];
    }
    for (int i = 0; i < M; ++i) REQUIRE(covered[i] == (in_set[i] ? 1 : 0), "%s M %d also %d: index %d covered %d times", what, M, also, i, covered[i]);
    return true;
}

static bool mask_cases() {
    for (int M = 1; M <= 70; ++M) {
        std::vector<int32_t> ones(M, 1), alt(M, 0), alt1(M, 0), mid(M, 0), ends(M, 0), two(M, 0);
        for (int i = 0; i < M; ++i) alt[i] = i % 2 == 0, alt1[i] = i % 2 == 1;
        for (int i = M / 3; i < M - M / 3; ++i) mid[i] = 1;                           // one run in the middle
        for (int i = 0; i < M; ++i) ends[i] = i < (M + 3) / 4 || i >= M - (M + 3) / 4;  // runs touching 0 and M - 1
        for (int i = 0; i < M; ++i) two[i] = i % 5 != 2;                              // runs of two and more, one index between them
        for (int also : {-1, 0, M - 1}) {
            if (!mask_case("all ones", ones, also) || !mask_case("alternating from 0", alt, also) || !mask_case("alternating from 1", alt1, also) ||
                !mask_case("one run in the middle", mid, also) || !mask_case("runs at both ends", ends, also) ||
                !mask_case("runs with single gaps", two, also))
                return false;
        }
        for (int one = 0; one < M; ++one) {  // a single one, and every place of `also` against it: adjacent below, above, isolated, on it
            std::vector<int32_t> single(M, 0);
            single[one] = 1;
            for (int also = -1; also < M; ++also)
                if (!mask_case("a single one", single, also)) return false;
        }
        // `also` everywhere against the middle run (adjacent below and above it, isolated, inside), against the runs with single gaps
        // (bridging two runs), and against none at all
        for (int also = 0; also < M; ++also)
            if (!mask_case("one run in the middle", mid, also) || !mask_case("runs with single gaps", two, also) ||
                !mask_case("no member", std::vector<int32_t>(M, 0), also))
                return false;
    }
    return true;
}

// ---- entry_planes ----
struct Entry {
    int name, level;
    double other;  // (an entry type of the caller's: only .name and .level are read)
};

static bool entry_case(const char *what, const std::vector<Entry> &entries) {
    const int E = static_cast<int>(entries.size());
    const EntryPlanes t = entry_planes(entries);
    // first appearance by nested loops: entry k opens a plane (a name) if no earlier entry has it
    std::vector<std::pair<int, int>> distinct;
    std::vector<int> ids;
    for (int k = 0; k < E; ++k) {
        bool plane_seen = false, name_seen = false;
        for (int j = 0; j < k; ++j) {
            plane_seen = plane_seen || (entries[j].name == entries[k].name && entries[j].level == entries[k].level);
            name_seen = name_seen || entries[j].name == entries[k].name;
        }
        if (!plane_seen) distinct.push_back({entries[k].name, entries[k].level});
        if (!name_seen) ids.push_back(entries[k].name);
    }
    REQUIRE(t.ids == ids, "%s E %d: %zu names, restated %zu", what, E, t.ids.size(), ids.size());
    REQUIRE(t.distinct == distinct, "%s E %d: %zu planes, restated %zu", what, E, t.distinct.size(), distinct.size());
    REQUIRE(static_cast<int>(t.plane_of.size()) == E, "%s E %d: plane_of has %zu", what, E, t.plane_of.size());
    for (int k = 0; k < E; ++k) {
        const int q = t.plane_of[k];
        REQUIRE(q >= 0 && q < static_cast<int>(t.distinct.size()), "%s E %d: plane_of[%d] = %d", what, E, k, q);
        REQUIRE(t.distinct[q].first == entries[k].name && t.distinct[q].second == entries[k].level, "%s E %d: entry %d is not on its plane", what, E, k);
    }
    // the per-plane iteration: every k exactly once, ascending within a plane, on the plane it is listed under
    std::vector<int> visits(E, 0);
    for (size_t q = 0; q < t.distinct.size(); ++q) {
        int last = -1, n = 0;
        bool ok = true;
        t.each_entry_of(q, [&](int k) {
            ok = ok && k > last && k >= 0 && k < E && t.plane_of[k] == static_cast<int>(q);
            if (k >= 0 && k < E) ++visits[k];
            last = k;
            ++n;
        });
        REQUIRE(ok && n >= 1, "%s E %d: plane %zu visited out of order or empty (%d entries)", what, E, q, n);
    }
    for (int k = 0; k < E; ++k) REQUIRE(visits[k] == 1, "%s E %d: entry %d visited %d times", what, E, k, visits[k]);
    return true;
}

static bool entry_cases() {
    const int A = 2, B = 12, Cc = 13, D = 0;  // (catalogue ids as the library has them: any ints do)
    if (!entry_case("one entry", {{A, 7, 0.0}})) return false;
    if (!entry_case("one plane", {{A, 7, 0.0}, {A, 7, 1.0}, {A, 7, 2.0}, {A, 7, 3.0}})) return false;
    if (!entry_case("all distinct", {{A, 0, 0.0}, {B, 1, 0.0}, {Cc, 0, 0.0}, {D, 3, 0.0}, {A, 1, 0.0}})) return false;
    if (!entry_case("A B A C B", {{A, 7, 0.0}, {B, 1, 1.0}, {A, 7, 2.0}, {Cc, 0, 3.0}, {B, 1, 4.0}})) return false;
    if (!entry_case("the issue's list", {{A, 7, 0.0}, {B, 1, 0.0}, {A, 7, 0.0}, {Cc, 0, 0.0}, {B, 1, 0.0}, {D, 0, 0.0}})) return false;
    if (!entry_case("one name, several levels", {{A, 3, 0.0}, {A, 0, 0.0}, {A, 3, 0.0}, {A, 7, 0.0}, {A, 0, 0.0}})) return false;
    if (!entry_case("several names, one level", {{A, 1, 0.0}, {B, 1, 0.0}, {D, 1, 0.0}, {B, 1, 0.0}, {A, 1, 0.0}})) return false;
    std::vector<Entry> many;
    for (int k = 0; k < 1024; ++k) many.push_back({(k * 7) % 28, (k / 3) % 8, static_cast<double>(k)});  // planes revisited far apart
    if (!entry_case("1024 entries", many)) return false;
    std::vector<Entry> apart;
    for (int k = 0; k < 1024; ++k) apart.push_back({k % 32, k / 32, 0.0});  // 1024 distinct planes
    return entry_case("1024 distinct planes", apart);
}

int main() {
    if (!mask_cases() || !entry_cases()) return 1;
    std::printf("entry_front sanitize ok %ld checks\n", checks);
    return 0;
}
