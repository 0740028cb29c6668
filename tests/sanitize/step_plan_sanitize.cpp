// AddressSanitizer / UndefinedBehaviorSanitizer driver for the step loop's host-side schedule (pyspeedy_amd/csrc/step_plan.hpp: member
// partition, transmissivity plan, recorder dueness; ring.hpp: SampleCursor).  Every check compares against a brute-force
// restatement written here -- members dealt out one by one, multiples counted in a loop, the record and the array simulated step
// by step -- not against the functions under test.  Compiled by tests/test_sanitizers.py with g++ -fsanitize=address,undefined.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "ring.hpp"
#include "step_plan.hpp"
#include "surface_host.hpp"

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

// n things dealt out one by one to k holders: counts that differ by at most one, the larger ones first
static std::vector<int> dealt(int n, int k) {
    std::vector<int> c(k, 0);
    for (int i = 0; i < n; ++i) ++c[i % k];
    return c;
}

static bool partition_case(int M, int nchunks, int bm, int nsteps, int one) {
    const Partition p = partition_members(M, nchunks, bm, nsteps, one != 0);
#define WHERE "M %d nchunks %d block_members %d nsteps %d one_group %d: G %d rounds %d", M, nchunks, bm, nsteps, one, p.G, p.rounds
    // the step loop's formula before it moved here
    const int G = (one || nsteps == 1) ? 1 : nchunks;
    int rounds = 1;
    const bool may_round = G > 1 || (nchunks == 1 && !one);
    if (may_round && nsteps > 1 && bm > 0 && M >= 4 * bm) rounds = (M + G * bm - 1) / (G * bm);
    REQUIRE(p.M == M && p.G == G && p.rounds == rounds, WHERE);
    if (nsteps == 1) REQUIRE(p.G == 1 && p.rounds == 1, WHERE);
    REQUIRE(p.G >= 1 && p.G <= kGroupStreams && p.rounds >= 1, WHERE);
    const std::vector<int> per_round = dealt(M, p.rounds);
    int next = 0;  // the first member nobody has yet
    for (int r = 0; r < p.rounds; ++r) {
        const int n = p.round_count(r);
        REQUIRE(n == per_round[r] && n >= 1, WHERE);
        const std::vector<int> per_group = dealt(n, p.G);
        bool empty_seen = false;
        const int round_first = next;
        for (int g = 0; g < p.G; ++g) {  // the step loop gives group g the members [next, next + count): ascending, no gap
            const int count = p.group_count(n, g);
            REQUIRE(count == per_group[g], WHERE);
            REQUIRE(!(empty_seen && count > 0), WHERE);  // an empty group is a trailing one
            empty_seen = empty_seen || count == 0;
            next += count;
        }
        REQUIRE(next == round_first + n, WHERE);
    }
    REQUIRE(next == M, WHERE);
#undef WHERE
    return true;
}

static bool partition_checks() {
    const int blocks[] = {0, 1, 4, 32}, steps[] = {1, 2, 36};
    for (int M = 1; M <= 130; ++M)
        for (int nchunks = 1; nchunks <= std::min(4, M); ++nchunks)
            for (int bm : blocks)
                for (int nsteps : steps)
                    for (int one = 0; one < 2; ++one)
                        if (!partition_case(M, nchunks, bm, nsteps, one)) return false;
    // the plan the GPU tests rely on for rounds with an empty trailing group
    const Partition p = partition_members(9, 2, 1, 36, false);
    REQUIRE(p.G == 2 && p.rounds == 5, "9 members, 2 groups, block_members 1: G %d rounds %d", p.G, p.rounds);
    REQUIRE(p.round_count(4) == 1 && p.group_count(1, 0) == 1 && p.group_count(1, 1) == 0, "the last round is one member in group 0");
    return true;
}

static bool tau_case(int c0, int nsteps, int diag_every_step, int takes_part) {
#define WHERE "start counter %d nsteps %d diag_every_step %d takes part %d step %d", c0, nsteps, diag_every_step, takes_part, it
    int it = 0;
    int first_sw = 0;
    while ((c0 + first_sw) % 3 != 0) ++first_sw;
    REQUIRE(tau_first_sw(c0) == first_sw, WHERE);
    // which shortwave step's values the array and the record hold: -1 what was there before the segment, -2 nothing anybody may read
    int array = -1, record = -2, latest = -1;
    for (it = 0; it < nsteps; ++it) {
        const bool sw = (c0 + it) % 3 == 0;
        const TauPlan t = tau_plan(takes_part != 0, sw, it, nsteps, first_sw, diag_every_step != 0);
        if (!takes_part || nsteps == 1) REQUIRE(!t.compact && !t.store_record && !t.store_array, WHERE);
        if (!t.compact) REQUIRE(!t.store_record && !t.store_array, WHERE);
        if (it == nsteps - 1) REQUIRE(!t.store_record, WHERE);
        if (sw) {
            latest = it;
            if (!t.compact) {
                array = it;  // the array form of a shortwave step stores the array
            } else {
                REQUIRE(t.store_record, WHERE);  // (a compact shortwave step that left nothing would lose its values)
                if (diag_every_step) REQUIRE(t.store_array, WHERE);
                if (t.store_record) record = it;
                if (t.store_array) array = it;
            }
        } else {
            REQUIRE(!t.store_record && !t.store_array, WHERE);
            const int read = t.compact ? record : array;
            REQUIRE(read == latest, WHERE);
            if (t.compact) REQUIRE(read >= 0, WHERE);  // the record is never one of another segment
        }
    }
    REQUIRE(array == latest, WHERE);  // (no shortwave step in the segment: latest is -1, the array untouched)
#undef WHERE
    return true;
}

static bool tau_checks() {
    for (int c0 : {0, 1, 2, 36, 37, 38, 1000, 1001, 1002})
        for (int nsteps = 1; nsteps <= 12; ++nsteps)
            for (int des = 0; des < 2; ++des)
                for (int part = 0; part < 2; ++part)
                    if (!tau_case(c0, nsteps, des, part)) return false;
    return true;
}

struct Issued {
    long long n;
    int slot;
    bool folds;
    bool operator==(const Issued &o) const { return n == o.n && slot == o.slot && folds == o.folds; }
};

// the step loop's use of a cursor for one recorder with period `every`, `rounds` times over the same nsteps steps from counter c0
static bool cursor_case(int capacity, int every, int c0, int nsteps, int rounds, long long taken0) {
#define WHERE "capacity %d every %d start counter %d nsteps %d rounds %d taken %lld", capacity, every, c0, nsteps, rounds, taken0
    int multiples = 0;  // of `every` in (c0, c0 + nsteps]
    for (int v = c0 + 1; v <= c0 + nsteps; ++v)
        for (int k = 1; k * every <= v; ++k) multiples += k * every == v ? 1 : 0;
    SampleRing ring(capacity, 6);
    ring.taken = taken0;
    std::fill(ring.rows.begin(), ring.rows.end(), -7);
    std::vector<int32_t> expected = ring.rows, after_first;
    SampleCursor cur(ring.taken);
    std::vector<Issued> first_round;
    for (int round = 0; round < rounds; ++round) {
        cur.rewind();
        Calendar cal;
        cal.set(1982 + 10 * round, 2, 27, 0, 0);  // (a later round stamping a row would leave another year there)
        std::vector<Issued> issued;
        for (int it = 0; it < nsteps; ++it) {
            const int c = c0 + it;
            cal.advance();
            bool due = false;
            for (int k = 1; k * every <= c + 1; ++k) due = due || k * every == c + 1;
            REQUIRE(due_after(c, every) == due, WHERE);
            if (!due) continue;
            const long long opens = cur.open(), n = cur.next();
            REQUIRE(n == opens && n == cur.last(), WHERE);
            REQUIRE(n == taken0 + static_cast<long long>(issued.size()) + 1, WHERE);
            int slot = 0;  // sample 1 lies in slot 0, every further one in the next, round the ring
            for (long long j = 1; j < n; ++j) slot = slot + 1 == capacity ? 0 : slot + 1;
            REQUIRE(ring.slot(n) == slot, WHERE);
            // folded unless a later sample of this segment takes the slot again
            bool folds = true;
            for (long long later = n + 1; later <= taken0 + multiples; ++later) folds = folds && (later - n) % capacity != 0;
            REQUIRE(enstape_folds(n, taken0, c0, nsteps, every, capacity) == folds, WHERE);
            issued.push_back({n, slot, folds});
            cur.commit(ring, round == 0, c + 1, cal);
            if (round == 0) {
                const int32_t row[6] = {c + 1, cal.year, cal.month, cal.day, cal.hour, cal.minute};
                std::copy(row, row + 6, expected.begin() + 6 * slot);
                REQUIRE(ring.taken == n, WHERE);
            }
        }
        if (round == 0) {
            first_round = issued;
            after_first = ring.rows;
        }
        REQUIRE(issued == first_round, WHERE);
        REQUIRE(static_cast<int>(issued.size()) == multiples, WHERE);
    }
    REQUIRE(ring.taken == taken0 + multiples, WHERE);
    REQUIRE(ring.rows == expected && ring.rows == after_first, WHERE);
#undef WHERE
    return true;
}

static bool cursor_checks() {
    for (int capacity = 1; capacity <= 4; ++capacity)
        for (int every = 1; every <= 5; ++every)
            for (int c0 = 0; c0 <= 7; ++c0)
                for (int nsteps = 1; nsteps <= 13; ++nsteps)
                    for (int rounds = 1; rounds <= 5; ++rounds)
                        for (long long taken0 : {0LL, 6LL})
                            if (!cursor_case(capacity, every, c0, nsteps, rounds, taken0)) return false;
    // the ensemble tape with room for one sample and two samples in one call: only the second is folded
    REQUIRE(!enstape_folds(1, 0, 0, 18, 9, 1) && enstape_folds(2, 0, 0, 18, 9, 1), "capacity 1, two samples in one call");
    return true;
}

int main() {
    if (!partition_checks() || !tau_checks() || !cursor_checks()) return 1;
    std::printf("step plan sanitize ok %ld checks\n", checks);
    return 0;
}
