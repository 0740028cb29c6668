// What the step loop (model.hip: step_segment) decides from the step counter and the configuration alone: how a call's members are
// cut into rounds and member groups, how the column kernel keeps the longwave transmissivities on each step of a segment, and when
// a recorder is due.  Host only, no HIP: small pure functions, exercised on the CPU by tests/sanitize/step_plan_sanitize.cpp.
#pragma once

namespace spd {

constexpr int kGroupStreams = 4;  // the most member groups a step is issued in: one stream each (spd_model: cstream, cev)

// Members never exchange data, so the step is issued group by group on separate streams: every group runs the same
// six launches on its own members, and the groups' kernels overlap on the GPU.
// Rounds (see block_members): the members of a round go through all steps of the call before the next round starts.
struct Partition {
    int M = 1, G = 1, rounds = 1;
    // the members of round r, and of group g of a round of n members: the counts differ by at most one, the larger ones first,
    // so an empty group can only be a trailing one
    int round_count(int r) const { return M / rounds + (r < M % rounds ? 1 : 0); }
    int group_count(int n, int g) const { return n / G + (g < n % G ? 1 : 0); }
};
// one_group: the call runs as one group whatever nchunks says (the split-launch mode, profiling)
// (a call of ONE step forks and joins the group streams around that step -- two dependent cross-stream hand-overs per
// step cost more than the overlap gains: measured +12 % at 64 members through spd_parallel_step -- so it is issued serially)
// Rounds also with ONE group when the caller says so by setting member_groups to 1 on a large model -- the outer boundary does for
// the two device models it keeps a large ensemble in, which are each other's groups: csrc/driver.cpp -- but never while profiling
// or in the split-launch mode, whose single group is the whole model by definition.
inline Partition partition_members(int M, int nchunks, int block_members, int nsteps, bool one_group) {
    Partition p;
    p.M = M;
    p.G = (one_group || nsteps == 1) ? 1 : nchunks;
    const bool may_round = p.G > 1 || (nchunks == 1 && !one_group);
    if (may_round && nsteps > 1 && block_members > 0 && M >= 4 * block_members)
        p.rounds = (M + p.G * block_members - 1) / (p.G * block_members);
    return p;
}

// The longwave transmissivities of the steps between two shortwave steps (every third step computes them; the reference keeps
// them in rad_tau2): inside a segment of two steps or more the fused column kernel hands them on as the compact record they
// are made of and recomputes (physics.hip, COMPACT; option tau_recompute).  The schedule is the segment's own -- every round
// and member group follows it, and nothing is carried from call to call: a host may have written rad_tau2 in between,
// through device views as well.
//   a step without shortwave uses the record when a shortwave step of this segment came before it, rad_tau2 otherwise;
//   a shortwave step stores the record unless it is the segment's last step (nobody would read it), and
//   stores rad_tau2 when no later shortwave step of the segment will overwrite it (or diag_every_step says so):
// at the end of every segment rad_tau2 is what the array form leaves, and only there can anybody look at it -- snapshots,
// container copies, get(), the physics replay; no recorder can name it (kStatsCatalogue, kAccNames).
// A round takes part from kTauFromMembers members up -- the size from which the default plan steps the members in groups whose
// launches overlap and the column kernel waits on memory.  Below that it runs at the issue rate of one wavefront per SIMD and
// the exponentials cost more than the bytes save: measured +1.9 % per step at one member, +1 % at 8, +1.5 % at 16, against
// -0.5 ... -3 % from 20 up (profiles/tau_recompute_ab.txt).  Option value 2: rounds of any size.
constexpr int kTauFromMembers = 20;  // members of a round from which the compact form is used
struct TauPlan {                     // how a step's column launch keeps the transmissivities; the default is the array form
    bool compact = false;                             // the launch uses the compact record instead of rad_tau2
    bool store_record = false, store_array = false;  // (compact shortwave steps) what the step leaves behind
};
// the first shortwave step (0-based) of a segment that starts at step counter c0
inline int tau_first_sw(int c0) { return ((3 - c0 % 3) % 3 + 3) % 3; }
// step `it` of a segment of nsteps whose first shortwave step is first_sw; sw: `it` is a shortwave step
inline TauPlan tau_plan(bool takes_part, bool sw, int it, int nsteps, int first_sw, bool diag_every_step) {
    TauPlan tau;
    if (takes_part && sw && it != nsteps - 1) {
        tau.compact = tau.store_record = true;
        tau.store_array = it + 3 > nsteps - 1 || diag_every_step;
    } else if (takes_part && !sw && it > first_sw) {
        tau.compact = true;
    }
    return tau;
}

// a recorder with period `every` is due after the step that leaves the counter at c + 1
inline bool due_after(int c, int every) { return (c + 1) % every == 0; }
// The ensemble tape folds sample number n of a segment that starts at counter c0 with `taken0` samples taken, unless a later sample
// of the SAME segment takes its slot again: nobody can read such a sample, and with rounds its members would otherwise land in the
// partials of the sample that replaced it.
inline bool enstape_folds(long long n, long long taken0, int c0, int nsteps, int every, int capacity) {
    const long long last = taken0 + (static_cast<long long>(c0) + nsteps) / every - c0 / every;  // the segment's last sample
    return n + capacity > last;
}

}  // namespace spd
