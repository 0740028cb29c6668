// The model object and what the translation units that work on it share (internal, host only): struct spd_model; the checks and
// the carving of an allocation that every in-loop feature's _configure and _read run around their own work; the front end of a
// sample that the statistics and four of the tapes share (defined in model.hip).  model.hip holds the model's life, its registry,
// the step loop and the rest of the C ABI; the host code of each in-loop feature lies behind its kernels in the feature's own file
// (stats.hip, tape.hip, spectra.hip, enstape.hip, acctape.hip, wintape.hip, projtape.hip, tracktape.hip, filtape.hip, nudge.hip, breed.hip, assim.hip, verif.hip, qtape.hip, plev.hip,
// derive.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "../../include/pyspeedy_amd.h"
#include "context.hpp"
#include "model.hpp"
#include "plev.hpp"
#include "derive.hpp"
#include "stats.hpp"
#include "spectra.hpp"
#include "tape.hpp"
#include "enstape.hpp"
#include "acctape.hpp"
#include "nudge.hpp"
#include "breed.hpp"
#include "assim.hpp"
#include "wintape.hpp"
#include "projtape.hpp"
#include "tracktape.hpp"
#include "filtape.hpp"
#include "verif.hpp"
#include "qtape.hpp"
#include "ring.hpp"
#include "entry_front.hpp"
#include "surface.hpp"

using namespace spd;  // (every file that includes this header is written inside or against namespace spd)

namespace spd {
constexpr int NG = IX * IL;
constexpr size_t C = 2;  // doubles per complex

// an entry of the projection tape, the assimilation and the verification tape: a plane under a weight map
struct PatternEntry {
    int name, level, pattern;  // name: catalogue id
};

struct RegEntry {
    void *ptr;            // device base
    size_t bytes_member;  // bytes per member (as fp64: the size the registry and the C boundary speak of)
    bool f32 = false;     // stored as fp32 (in the first half of the allocation) while the model's physics precision is fp32
};
}  // namespace spd

struct spd_model {
    spd_context *ctx = nullptr;
    int M = 0;
    ModelPtrs P{};
    const spd_dyn_tables *dyn = nullptr;            // the context's tables of the current time step (nullptr: none set yet)
    std::unique_ptr<spd_dyn_tables> dyn_private;    // only when the context already holds kMaxDynSteps other time steps
    DynDeviceTables D{};
    spd_physics_args pa{};
    // Device memory of the model: a few large zero-filled blocks the arrays are carved from (arena_alloc).  A model has some 170
    // arrays and tables; one hipMalloc + hipMemset + hipFree each made creating and closing a state container the most
    // expensive calls of a host that follows the reference's sequence (1.3 ms and 1.8 ms per one-member model).
    struct Block {
        char *base;
        size_t size, used;
    };
    std::vector<Block> blocks;
    std::map<std::string, RegEntry> reg;
    FieldDesc *inv_table[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};  // [dynamics time level j2 (0-based)][phi buffer]
    FieldDesc *inv_table_sppt[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};  // the same + 8 SPPT pattern transforms per member
    // ... and both with the physics-only outputs (time-level-1 T, q, phi, ln ps, lowest-level u, v) stored as fp32 (cfg 5)
    FieldDesc *inv_table32[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}}, *inv_table_sppt32[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};
    FieldDesc *fwd_table = nullptr;
    FieldDesc *fwd_table_products = nullptr;  // the same transforms, the 40 products formed while staging (fused column kernel)
    // Geopotential, double-buffered.  spectral_step_kernel ends by computing the geopotential the NEXT step needs (from the
    // temperature it has just advanced) into the buffer that is not in use; the next step switches to it instead of running
    // geopotential_kernel.  The registry's "phi" is always the buffer the last step USED (the reference's state%phi after a
    // step).  phi_ahead is dropped whenever something outside the step may have changed the temperature.
    double *phi_buf[2] = {nullptr, nullptr};
    int phi_cur = 0;
    // fold_geo: on by default for small ensembles (<= 8 members), where the step is bound by launch and dependent-latency
    // chains and one launch less is worth 1-3 %; at 64 members the longer spectral_step_kernel costs 2 % more than the
    // geopotential launch it saves (A/B in one session, profiles/).  PYSPEEDY_AMD_FOLD_GEO=0 / 1 overrides.
    bool phi_ahead = false, fold_geo = true;
    bool groups_apart = true;  // every group stream created so far was measured to run side by side with the others
    int *d_err = nullptr;
    double *d_diag = nullptr;
    // The quiet rim: one flag per member, armed and established by the device inside a multi-step call (step_impl) and valid in
    // that call only.  rim_call: the last call of spd_model_step / _step_checked_begin used the flags (option "quiet_rim_members").
    int *d_rim = nullptr;
    bool rim_call = false;
    // asynchronous range check (spd_model_check_begin / _end): two pinned result slots with their events
    int *h_err[2] = {nullptr, nullptr}, *h_err_sync = nullptr;  // (h_err_sync: pinned staging of the synchronous check)
    hipEvent_t err_event[2] = {nullptr, nullptr};
    int next_slot = 0;
    bool slot_busy[2] = {false, false};  // begun and not yet ended
    int check_ticket = 0, slot_ticket[2] = {0, 0};  // every range-check launch publishes its codes under a ticket of its own
    // A check whose launch is put off until the next step (spd_model_check_defer): it then rides in that step's spectral -> grid
    // launch.  Launched on its own as soon as anything else would look at or change the state first (settle_deferred_check).
    struct DeferredCheck {
        bool active = false;
        int slot = -1, time_level = 2;
        hipStream_t stream = nullptr;
    } deferred;
    hipStream_t slot_stream[2] = {nullptr, nullptr};  // the stream a slot's launch went out on
    bool slot_rode[2] = {false, false};               // ... inside a step's launch (no completion event of its own)
    int checks_alone = 0, checks_rode = 0;            // range checks launched on their own / carried by a step's launch
    double air_absortivity_co2 = 6.0;  // model_state_def.py:320 default
    // device copies of the dt-dependent tables (re-uploaded by set_time_step)
    // surface / coupler state, calendar and run control (do_single_step, speedy.f90:20-74)
    SurfacePtrs S{};
    Calendar cal;
    int current_step = 0;
    bool initialized = false;
    // SPPT (csrc/sppt.hip): AR(1) spectral pattern [M][8][992] complex, its grid-space image [M][8][NG]
    bool sppt_on = false, sppt_first = true;
    unsigned long long sppt_seed = 0;
    long long sppt_member_base = 0, sppt_step = 0;
    double *sppt_spec = nullptr, *sppt_grid = nullptr;
    // Members are stepped in `nchunks` groups on separate HIP streams (spd_model_step): a group's kernels overlap with
    // the other groups' (different kernels, complementary resources, no idle tail between dependent launches).
    // spectral -> grid transforms per member and step: 77 = the reference's 91 minus the 14 whose results nothing reads (u, v
    // above the lowest level at the physics' time level: physics.f90:93-94 computes them, get_surface_fluxes only uses level
    // kx; every registry variable stays bitwise identical, tests/test_run_gpu.py).  PYSPEEDY_AMD_PRUNE_DEAD=0 restores all 91.
    int inv_per_member = 77;
    int nchunks = 1;
    // Large ensembles in multi-step calls: from 4 x `block_members` members up, spd_model_step(m, n) takes the members in ROUNDS of
    // nchunks x block_members -- a round through ALL n steps before the next round starts (members never exchange data).  A group's
    // spectral step is then followed on its stream by the spectral -> grid launch of its own next step, which reads what was just
    // written while it is still in the 256 MB Infinity Cache, as in a 64-member ensemble; with 128 members per group it is not,
    // and a member-step costs 5-10 % more (profiles/r05_members_per_gpu.txt).  The host-side state of the step (calendar, step
    // counter, geopotential buffer, SPPT counter, CO2) is rewound for every round.  0: off (PYSPEEDY_AMD_BLOCK_MEMBERS, option
    // "block_members").
    int block_members = 32;
    hipStream_t cstream[kGroupStreams] = {};
    hipEvent_t cev[kGroupStreams] = {}, ev_start = nullptr, ev_offset = nullptr;
    bool split_dyn_physics = false;  // PYSPEEDY_AMD_SPLIT_DYN=1: separate dynamics and physics launches (for measurements)
    // spd_model_set_physics_precision (BASELINE cfg 5): column physics arithmetic in fp32 AND fp32 storage of what only the
    // column physics reads back (RegEntry::f32: its time-level-1 inputs, the persisted radiation state, diagnostics-only outputs)
    int phys_fp32 = 0;
    bool phys_store32 = true;  // option physics_storage32 / PYSPEEDY_AMD_PHYS_STORE32: 0 keeps fp64 storage under the fp32 physics
    bool stored32 = false;     // how the RegEntry::f32 arrays are stored right now (= phys_fp32 && phys_store32)
    // A change of that storage converts the arrays in place, one by one; a device error in the middle leaves some of them
    // converted and `stored32` unable to say which.  The model then refuses every call that would read or advance its state.
    std::string poisoned;
    // ... and a device error in the middle of a step (some launches of it out, others not; or one member group a step ahead of
    // another): the STATE is then inconsistent, not the storage -- spd_model_init, which rebuilds every array from the boundary
    // fields, makes the model usable again; nothing else does.
    std::string step_poison;
    int fail_launch_after = -1;  // fault injection for tests (option "fail_launch_after"): the n-th step_range of the next call fails
    // spd_model_step_checked_begin / _end: the range check of EVERY step of a multi-step call, recorded by the device into pinned
    // host memory [steps][M] (4 * ticket + flag, as the single checks do) by check blocks that ride in the next step's
    // spectral -> grid launch; the last step's check is a launch of its own behind the call.
    int *h_steps_err = nullptr;
    int steps_cap = 0, steps_pending = 0, steps_ticket = 0;
    hipEvent_t steps_event = nullptr;
    std::vector<int32_t> steps_accepted;  // [steps + 1][7]: step counter, y, m, d, h, min, month_idx before the call and after each step
    // Dead-store elimination inside multi-step calls (PYSPEEDY_AMD_DIAG_EVERY_STEP=1 switches it off): only the LAST step
    // of a spd_model_step call stores the physics outputs that no later kernel reads -- the host can only look at the
    // state between calls, and every earlier value would be overwritten before that.
    bool diag_every_step = false;
    // The longwave transmissivities between shortwave steps of a multi-step call (option "tau_recompute", PYSPEEDY_AMD_TAU_RECOMPUTE;
    // DESIGN section 4): a shortwave step leaves the ten values per column they are made of in `tau_rec` ([M][10][4608], stored
    // like rad_tau2; scratch that means something only inside a call, not a registry variable) and the next two steps recompute
    // them; rad_tau2 itself is stored by the last shortwave step of a call only.  0: every shortwave step stores rad_tau2 and
    // every other step loads it, as the one-step calls and the separate physics launch always do.  1: where 20 members and more
    // step together (the whole ensemble, or a round of a large one).  2: whatever the size.
    int tau_recompute = 1;
    double *tau_rec = nullptr;
    // The coupler's climatology interpolation is valid for a day (surface.hip): true after a coupling, false after anything
    // wrote to the state from outside the step
    bool surf_cache_valid = false;
    int spectral_early = -1;  // spectral_step_kernel with all loads up front: -1 = for launches of up to 8 members, 0 / 1 = never / always
    int land_coupling_flag = 1, sst_anomaly_flag = 1, increase_co2 = 0, anom_planes = 3;
    double ablco2_ref = 6.0;
    double *corh_t = nullptr, *corh_q = nullptr, *scratch_spec = nullptr;  // [M][NG], [M][NG], [2][M][992] complex
    double *orog = nullptr, *phi0 = nullptr, *fmask_orig = nullptr, *veg_high = nullptr, *veg_low = nullptr,
           *soil_wc_l1 = nullptr, *soil_wc_l2 = nullptr, *soil_wc_l3 = nullptr, *bmask_land = nullptr, *bmask_sea = nullptr;
    // optional profiling with HIP events on the launch stream: level 1 brackets the dominant kernel (the spec2grid table
    // launch) only, level 2 every kernel of the step (spd_model_profile; kernel ids SPD_K_* of pyspeedy_amd.h)
    int profile = 0;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_events;
    std::vector<int> prof_fields;  // fields of each profiled launch
    std::vector<int> prof_kernel;  // kernel id of each profiled launch
    size_t prof_used = 0;
    // grid-space copies of the prognostic variables in output units (prognostics.f90:125-219) and their transform tables
    double *u_grid = nullptr, *v_grid = nullptr, *t_grid = nullptr, *q_grid = nullptr, *phi_grid = nullptr, *ps_grid = nullptr;
    FieldDesc *exp_inv_table[2] = {nullptr, nullptr}, *exp_fwd_table[2] = {nullptr, nullptr};  // 41 / 40 per member; [phi buffer]
    // What the front end of a sample (statistics or tape) runs and where it writes: vort2vel when u or v is wanted, the export
    // transforms over a descriptor table ([phi buffer]) whose destinations are the slab [M][slab_fields][4608], and the
    // pressure-level kernel (raw = 1) from the slab's transformed planes into its further planes, then the derived-field kernel
    // (raw = 1) likewise.  The statistics, the tape and the ensemble tape each own one, in their own allocation.
    struct SampleFront {
        bool uv = false, precip = false;
        // slab_fields: planes of a member in the slab; the first xf_fields of them are written by the export transforms, the
        // others (pressure-level and derived variables only) by the pressure-level and derived-field kernels from those
        int slab_fields = 0, xf_fields = 0;
        PlevArgs plev{};      // (plev.mask != 0: a pressure-level variable is sampled)
        DeriveArgs derive{};  // (derive.mask != 0: a derived variable of the derived-field kernel is sampled)
        // a variable on the target levels of spd_model_plev_configure is sampled (of either kernel)
        bool holds_plev() const { return plev.mask != 0 || (derive.mask & kDerivePlevMask) != 0; }
        double *slab = nullptr;
        FieldDesc *table[2] = {nullptr, nullptr};
    };
    // Running time statistics (spd_model_stats_*): sampled by the step loop after every step that ends on a multiple of `every`,
    // behind each member group's last launch of that step on the group's stream.  One allocation (own hipMalloc, not the arena:
    // a reconfiguration frees it): the accumulators [variable][M][levels][4608] (mean, and M2 with variance), the sample slab
    // [M][slab_fields][4608] the export transforms write instead of the registry's grid arrays, their descriptor tables
    // ([phi buffer]) and the plane descriptors of the accumulate kernel.
    struct Stats : SampleFront {
        struct Var {
            int id, levels;
            size_t offset;  // doubles from `mean` / `m2` to member 0 of the variable
        };
        bool on = false, variance = false;
        int every = 1, nplanes = 0;
        long long samples = 0;
        Validity validity;
        std::vector<Var> vars;
        void *alloc = nullptr;
        double *mean = nullptr, *m2 = nullptr;
        StatsPlane *planes = nullptr;
    } stats;
    // The tape (spd_model_tape_*): a ring of the last `capacity` samples of chosen fields, taken where the statistics take theirs
    // (its own `every`, slab and tables).  One allocation of its own (hipMalloc): the ring, per variable [slot][M][levels][4608] in
    // `dtype`, then slab, tables and the plane descriptors of the store kernel.  Slots, and the step and date of each sample: `ring`
    // (ring.hpp).
    struct Tape : SampleFront {
        struct Var {
            int id, levels;
            size_t offset;  // elements from `data` to slot 0, member 0 of the variable
        };
        bool on = false;
        int every = 1, dtype = 0, nplanes = 0;
        SampleRing ring;  // rows [6]: absolute step after the sampled step, year, month, day, hour, minute
        Validity validity;
        std::vector<Var> vars;
        void *alloc = nullptr, *data = nullptr;
        TapePlane *planes = nullptr;
    } tape;
    // Spectra and global means of the spectral state (spd_model_spectra_*): a ring of the last `capacity` samples of the chosen
    // names, fp64, written by one launch per member group and sample behind the tape's (no transform, no slab: spectra.hip).  One
    // allocation of its own (hipMalloc): per name [slot][M][per] doubles.  Slots, and the step and date of each sample: `ring`.
    struct Spectra {
        bool on = false;
        int every = 1;
        unsigned mask = 0;
        SampleRing ring;  // rows [6]: absolute step after the sampled step, year, month, day, hour, minute
        Validity validity;
        void *alloc = nullptr;
        size_t offset[SPECTRA_NNAMES] = {};  // doubles from `alloc` to slot 0, member 0 of a name of the mask
    } spectra;
    // The ensemble tape (spd_model_enstape_*): a ring of the last `capacity` samples of the mean over all members and of the sum of
    // squared deviations from it (M2), per grid point, fp64, taken by the tape's rule (its own `every`, slab and tables) behind the
    // spectra's sample.  One allocation of its own (hipMalloc): mean and M2 rings, each [slot][4][planes][4608] -- one partial per
    // group stream, written only from that stream (enstape.hpp) --, then slab, tables and the plane descriptors of the fold kernel.
    // Slots, and the step and date of each sample: `ring`; the members already folded into each partial of a slot (`counts`) are
    // kept on the host at issue time as well.
    struct EnsTape : SampleFront {
        struct Var {
            int id, levels;
            size_t first_plane;  // planes of the variables before this one
        };
        bool on = false;
        int every = 1, nplanes = 0;
        SampleRing ring;  // rows [6]: absolute step after the sampled step, year, month, day, hour, minute
        Validity validity;
        std::vector<Var> vars;
        std::vector<int> counts;  // [capacity][4]: members folded into partial (slot, group)
        void *alloc = nullptr;
        double *mean = nullptr, *m2 = nullptr;
        EnsTapePlane *planes = nullptr;
    } enstape;
    // The accumulation tape (spd_model_acctape_*): window sums, means, minima and maxima of the column physics' 2-D outputs.  An
    // accumulate launch follows EVERY step while it is on (acctape.hip); a window closes by the tape's rule into the slot of
    // `ring`, which counts the windows closed since the last reset.  No front end: the values are read where the column
    // kernel stores them.  One allocation of its own (hipMalloc): ring (per entry [slot][M][planes][4608], float or double), the
    // fp64 accumulators some entry needs ([M][planes][4608] each), the plane descriptors.  The step the open window started at and
    // the rows of the closed ones (step, date, number of steps) are host state.
    struct AccTape {
        struct Entry {
            int name, op, planes;
            size_t offset;  // elements from `data` to slot 0, member 0 of the entry
        };
        bool on = false;
        int every = 1, dtype = SPD_TAPE_F32, nplanes = 0;
        int window_start = -1;  // absolute step counter the open window began at (-1: at the next step that runs)
        SampleRing ring;        // of closed windows; rows [7]: step after the window, year, month, day, hour, minute of that state, steps in it
        Validity validity;
        std::vector<Entry> entries;
        void *alloc = nullptr, *data = nullptr;
        AccTapePlane *planes = nullptr;
    } acctape;
    // The window tape (spd_model_wintape_*): window sums, means, extremes and threshold counts of the state's grid-space fields.
    // The tape's front end (its own slab and tables) and an accumulate launch follow every step that samples (the tape's rule
    // with `sample_every`); a window closes every `every` steps, at midnight or at month ends (wintape_advance) into the slot of
    // `ring`, which counts the windows closed since the last reset; a closing step that does not sample launches the
    // kernel alone.  One allocation of its own (hipMalloc): ring (per entry [slot][M][levels][4608], float or double), the fp64
    // accumulators some entry needs ([M][levels][4608] each), slab, tables, plane descriptors.  The step the open window started
    // at, its samples so far and the rows of the closed ones are host state.
    struct WinTape : SampleFront {
        struct Entry {
            int name, op, levels;  // name: catalogue id; behind the catalogue: wspd_grid, wspd_plev
            double threshold;
            size_t offset;  // elements from `data` to slot 0, member 0 of the entry
        };
        bool on = false;
        int window = SPD_WINDOW_STEPS, every = 1, sample_every = 1, dtype = SPD_TAPE_F32, nplanes = 0;
        int window_start = -1;  // absolute step counter the open window began at (-1: at the next step that runs)
        int samples = 0;        // samples the open window holds
        SampleRing ring;        // of closed windows; rows [8]: step after the window, year, month, day, hour, minute, samples, steps
        Validity validity;
        std::vector<Entry> entries;
        void *alloc = nullptr, *data = nullptr;
        WinTapePlane *planes = nullptr;
    } wintape;
    // The projection tape (spd_model_projtape_*): weighted sums of single planes of the state's grid-space fields under fixed weight
    // maps -- one double per entry, member and sample.  Sampled by the tape's rule (its own `every`, slab and tables) behind the
    // window tape's launch.  One allocation of its own (hipMalloc): the ring [slot][M][E] doubles, the patterns [P][4608], slab,
    // tables, the descriptors of the distinct planes and the entry list sorted by plane (projtape.hpp).  Slots, and the step and
    // date of each sample: `ring`.
    struct ProjTape : SampleFront {
        bool on = false;
        int every = 1, npatterns = 0, nplanes = 0;
        SampleRing ring;  // rows [6]: absolute step after the sampled step, year, month, day, hour, minute
        Validity validity;
        std::vector<PatternEntry> entries;
        void *alloc = nullptr;
        double *data = nullptr, *weights = nullptr;
        ProjTapePlane *planes = nullptr;
        ProjTapeItem *items = nullptr;
    } projtape;
    // The track tape (spd_model_tracktape_*): the minimum or maximum of single planes of the state's grid-space fields over regions,
    // where it lies and two sub-grid offsets -- four doubles per entry, member and sample --, optionally followed from sample to
    // sample inside a window round the last position.  Sampled by the tape's rule (its own `every`, slab and tables) behind the
    // projection tape's launch.  One allocation of its own (hipMalloc): the ring [slot][M][E][4] doubles, the regions [R][4608]
    // bytes, the follow-state `last` [M][E] int32 (-1: follows nothing), slab, tables, the descriptors of the distinct planes and
    // the entry list sorted by plane (tracktape.hpp).  Slots, and the step and date of each sample: `ring`.
    struct TrackTape : SampleFront {
        struct Entry {
            int name, level, region, op, radius;  // name: catalogue id; op: SPD_TRACK_*
        };
        bool on = false;
        int every = 1, nregions = 0, nplanes = 0;
        SampleRing ring;  // rows [6]: absolute step after the sampled step, year, month, day, hour, minute
        Validity validity;
        std::vector<Entry> entries;
        std::vector<unsigned char> host_masks;  // [R][4608]: the regions as the device holds them (a seed is checked against them)
        void *alloc = nullptr;
        double *data = nullptr;
        unsigned char *masks = nullptr;
        int *last = nullptr;
        TrackTapePlane *planes = nullptr;
        TrackTapeItem *items = nullptr;
    } tracktape;
    // The filter tape (spd_model_filtape_*): window means, covariances and last values of time-filtered planes of the state's
    // grid-space fields.  The tape's front end (its own slab and tables) and the filter launch follow every step that samples (the
    // tape's rule with `sample_every`); the accumulate launch follows a counted sample -- one behind the `spinup` filter samples
    // since _configure, _reset, spd_model_init or a step counter set by hand -- and a closing step (the window tape's schedule,
    // filtape_advance), behind the track tape's launch.  One allocation of its own (hipMalloc): ring (per entry [slot][M][4608],
    // float or double), the sections' state [M][F][S][2][4608], the filtered values [M][F][4608] and the accumulators [M][E][4608]
    // (fp64), slab, tables, the descriptors of the filtered planes and of the entries (filtape.hpp).  The step the open window
    // started at, its counted samples, the number of filter samples so far and the rows of the closed windows are host state.
    struct FilTape : SampleFront {
        struct Entry {
            int name, level, filter, op, name_b, level_b;  // names: catalogue ids (name_b -1: none); op: SPD_FIL_*
        };
        bool on = false;
        int window = SPD_WINDOW_STEPS, every = 1, sample_every = 1, spinup = 0, dtype = SPD_TAPE_F32;
        int nfilters = 0, nplanes = 0, smax = 0;
        int window_start = -1;          // absolute step counter the open window began at (-1: at the next step that runs, with filter sample 1)
        int samples = 0;                // counted samples the open window holds
        long long filter_samples = 0;   // filter samples since the filters last started (k of the definition)
        SampleRing ring;                // of closed windows; rows [8]: step after the window, year, month, day, hour, minute, counted samples, steps
        Validity validity;
        std::vector<Entry> entries;
        void *alloc = nullptr, *data = nullptr;
        double *state = nullptr, *y = nullptr, *acc = nullptr;
        FilTapePlane *planes = nullptr;
        FilTapeItem *items = nullptr;
    } filtape;
    // Nudging (spd_model_nudge_*): relaxation of the spectral state toward target fields, the one thing in the device loop that
    // WRITES the state.  In the in-loop mode a launch follows the step_range of every member group on the group's stream, in front
    // of the last step's range check and of every recorder (nudge.hip); spd_model_nudge_apply is the same launch once, on the state
    // as it stands.  One allocation of its own (hipMalloc): the target slots (per name [capacity][levels][992] complex128, shared by
    // all members, zero-filled), the gain rows and descriptors of the planes some gain of which is not zero, and the member mask.
    // The slots in use and their absolute step stamps are host state: the bracketing slots and the interpolation weight of a
    // step travel by value.
    struct Nudge {
        bool on = false, in_loop = false;
        int capacity = 0, in_use = 0, nplanes = 0;
        long long applied = 0;       // steps nudged so far: in-loop steps and calls of _apply that launched
        std::vector<int> names;      // 0 vor, 1 div, 2 t, 3 tr, 4 ps, in the caller's order
        std::vector<int> stamps;     // [in_use], strictly ascending
        size_t offset[5] = {};       // doubles from `targets` to slot 0 of a name
        void *alloc = nullptr;
        double *targets = nullptr;
        int *mask = nullptr;         // [M] on the device, or null: every member is nudged
        NudgePlane *planes = nullptr;
        bool loops() const { return on && in_loop && nplanes > 0; }  // a launch follows every step of spd_model_step
    } nudge;
    // Breeding (spd_model_breed_*): the perturbation of a bred member against its control is rescaled to `target` after every step
    // that leaves the step counter at a multiple of `every` (breed.hip).  The one operation that couples members across member
    // groups and rounds: a call with in-loop breeding is issued as segments that end at the rescale steps (step_impl), and the two
    // launches go out on the caller's stream behind the join of the group streams.  One allocation of its own (hipMalloc): the
    // plane descriptors with their weights, the compact list of (member, control), each member's index in that list, the partial
    // norms [bred][33] and the ring [capacity][2][M] of amplitudes and factors (`data`).  Slots, steps and dates of the events: `ring`.
    struct Breed {
        bool on = false, in_loop = false;
        int every = 0, nbred = 0;
        double target = 0.0;
        SampleRing ring;        // of events since _configure / _reset; rows [6]: step counter, y, m, d, h, min of an event's state
        long long applied = 0;  // rescales launched since _configure: in-loop ones and calls of _apply
        void *alloc = nullptr;
        BreedPlane *planes = nullptr;
        BreedPair *pairs = nullptr;
        int *slot_of = nullptr;
        double *partial = nullptr, *data = nullptr;
        std::vector<BreedPair> host_pairs;  // the pairs as _configure built them (ascending member index)
        // Orthonormalised breeding (spd_model_breed_orthogonalize): a second allocation with the families, their
        // member list, each member's (family, position), the Gram partials [pairs][33], C [families][64][64] and the ranks.
        struct Ortho {
            bool on = false;
            int families = 0, largest = 0;
            long pairs = 0;
            void *alloc = nullptr;
            BreedFamily *fams = nullptr;
            int *members = nullptr, *place = nullptr, *rank = nullptr;
            double *partial = nullptr, *coef = nullptr;
        } ortho;
        bool loops() const { return on && in_loop && nbred > 0; }  // spd_model_step is issued in segments
    } breed;
    // Assimilation (spd_model_assim_*): a serial ensemble square-root filter over the masked members, after every step that leaves
    // the step counter at a multiple of `every` AND carries a row of observations (assim.hip).  Like breeding it couples members
    // across member groups and rounds, so a call with in-loop assimilation is issued as segments that end at those steps
    // (step_impl) and the event goes out on the caller's stream behind the join.  One allocation of its own (hipMalloc): the ring
    // [capacity][E][4] (`data`), the patterns [P][4608], slab, tables, the projection kernel's plane descriptors and entry list,
    // the one-slot projection ring [M][E] (`yraw`), Y [E][r], W [64][64], the member list and the transform's plane descriptors.
    // The observation table is host state: the row of an event travels to the weights kernel by value.
    struct Assim : SampleFront {
        bool on = false, in_loop = false;
        int every = 0, npatterns = 0, nplanes = 0, r = 0;
        double inflation = 1.0;
        SampleRing ring;  // of executed events since _configure / _reset; rows [6]: step counter, y, m, d, h, min of an event's state
        Validity validity;
        long long applied = 0, skipped = 0;  // events executed since _configure; in-loop events without a row since _configure / _reset
        std::vector<PatternEntry> entries;
        MemberSet set;                              // the masked members (r of them) and their runs
        std::vector<int> obs_steps;                 // [T], strictly ascending
        std::vector<double> obs_yo, obs_var;        // [T][E]
        void *alloc = nullptr;
        double *data = nullptr, *weights = nullptr, *yraw = nullptr, *Y = nullptr, *W = nullptr;
        int *member_list = nullptr;
        ProjTapePlane *planes = nullptr;
        ProjTapeItem *items = nullptr;
        AssimPlane *xplanes = nullptr;
        bool loops() const { return on && in_loop; }  // spd_model_step is issued in segments
    } assim;
    // The verification tape (spd_model_verif_*): scores of the masked members against a truth member of the same model, after every
    // step that leaves the step counter at a multiple of `every` (verif.hip).  It reads members of every member group and round, so
    // a call with in-loop verification is issued as segments that end at those steps (step_impl), and the event goes out on the
    // caller's stream behind the join -- in front of breeding's or the assimilation's event of the same step, and once more behind
    // an analysis that was applied there.  It writes nothing into the model.  One allocation of its own (hipMalloc): the rings
    // [capacity][2][E][4] doubles (`data`) and [capacity][2][E][66] int32 (`counts`), the patterns [P][4608], slab, tables, the
    // distinct planes' sources, the entry list, the member list, and the point kernel's scratch [planes][4][4608] doubles
    // (`point`) and [planes][4608] int32 (`bin`).
    struct Verif : SampleFront {
        bool on = false, in_loop = false;
        int every = 0, npatterns = 0, nplanes = 0, r = 0, truth = -1;
        SampleRing ring;  // of events since _configure / _reset; rows [7]: step counter, y, m, d, h, min of the state, analysis (0 / 1)
        Validity validity;
        long long applied = 0;  // events recorded since _configure: in-loop ones and calls of _apply
        std::vector<PatternEntry> entries;
        MemberSet set;  // the masked members (r of them); the runs cover the truth as well
        void *alloc = nullptr;
        double *data = nullptr, *weights = nullptr, *point = nullptr;
        int *counts = nullptr, *bin = nullptr, *member_list = nullptr;
        SampleSource *planes = nullptr;
        VerifItem *items = nullptr;
        bool loops() const { return on && in_loop; }  // spd_model_step is issued in segments
    } verif;
    // The quantile tape (spd_model_qtape_*): order statistics over the masked members per grid point -- minimum, maximum, quantiles,
    // exceedance probabilities --, after every step that leaves the step counter at a multiple of `every` (qtape.hip).  It reads
    // members of every member group and round, so a call with the in-loop quantile tape is issued as segments that end at those
    // steps (step_impl), and the event goes out on the caller's stream behind the join, in front of every other joined consumer's
    // event of the same step.  It writes nothing into the model.  One allocation of its own (hipMalloc): the ring
    // [capacity][E][4608] doubles (`data`), slab, tables, the distinct planes with their sources, the entry descriptors sorted by
    // plane, and the member list.
    struct Qtape : SampleFront {
        struct Entry {
            int name, level, op;  // name: catalogue id; op: SPD_Q_*
            double param;
        };
        bool on = false, in_loop = false;
        int every = 0, nplanes = 0, r = 0;
        SampleRing ring;  // of events since _configure / _reset; rows [6]: step counter, y, m, d, h, min of the sampled state
        Validity validity;
        long long applied = 0;  // events recorded since _configure: in-loop ones and calls of _apply
        std::vector<Entry> entries;
        MemberSet set;  // the masked members (r of them) and their runs
        void *alloc = nullptr;
        double *data = nullptr;
        int *member_list = nullptr;
        QtapePlane *planes = nullptr;
        QtapeItem *items = nullptr;
        bool loops() const { return on && in_loop; }  // spd_model_step is issued in segments
    } qtape;
    // spd_model_assim_transform, which works without an assimilation configured: the transform's plane descriptors, a member list
    // and W [64][64] in a small allocation of their own, made at the first call.
    struct AssimTransform {
        void *alloc = nullptr;
        AssimPlane *xplanes = nullptr;
        int *member_list = nullptr;
        double *W = nullptr;
    } assim_xf;
    // Pressure-level fields (spd_model_plev_*): the target levels and the result arrays [M][n][4608] (mslp: [M][4608]), carved
    // from the arena the first time a variable is computed (and again only if a later configuration has more levels).
    struct Plev {
        int n = 0;
        double levels[kPlevMaxLevels] = {}, lnp[kPlevMaxLevels] = {};
        double *out[PLEV_NVARS] = {};
        int cap[PLEV_NVARS] = {};     // levels the allocation holds
        bool have[PLEV_NVARS] = {};   // computed since the levels were configured
    } plev;
    // Derived fields (spd_model_derive_*): the result arrays [M][levels][4608] of vor_grid, div_grid ([0], [1]) and of the kernel's
    // outputs ([2 + DeriveVar]), carved from the arena the first time a name is computed (the pressure-level ones again only if a
    // later configuration has more levels), and grad ln ps [2][M][4608], transformed by a descriptor table of its own.
    struct Derive {
        double *out[2 + DRV_NVARS] = {};
        int cap[2 + DRV_NVARS] = {};    // levels the allocation holds
        bool have[2 + DRV_NVARS] = {};  // computed (the pressure-level ones: since the levels were configured)
        double *grad = nullptr;
        FieldDesc *table = nullptr;     // [M][18]: vor, div (8 levels each), px, py of a member
    } derive;
};

namespace spd {

inline int m_fail(int code, const std::string &msg) { return spd_set_error(code, msg); }
inline int usable(const spd_model *m, const char *who, bool about_to_init = false) {
    if (!m->poisoned.empty()) return m_fail(SPD_E_DEVICE, std::string(who) + ": this model is unusable: " + m->poisoned);
    if (!about_to_init && !m->step_poison.empty())
        return m_fail(SPD_E_ARG, std::string(who) + ": this model is unusable until it is initialised again (spd_model_init): " + m->step_poison);
    return SPD_OK;
}
inline int member_range(spd_model_handle m, int first, int count, const char *who) {
    if (!m) return m_fail(SPD_E_ARG, std::string(who) + ": null model");
    if (first < 0 || count < 0 || first + count > m->M) return m_fail(SPD_E_ARG, std::string(who) + ": member range out of bounds");
    return usable(m, who);
}
// (model.hip) `doubles` of zero-filled device memory that lives as long as the model (arena_alloc), registered under `name` if given
int dalloc(spd_model *m, size_t doubles, double **out, const char *name = nullptr, size_t bytes_member = 0);
// (model.hip) a range check that was put off (spd_model_check_defer) goes out now: for whatever reads or writes the state
int settle_deferred_check(spd_model *m);

// (A failed runtime call also leaves its code behind as the thread's "last error", and the launch wrappers of the kernels report
// hipGetLastError(): a hipMalloc that ran out of memory would come back as the "failure" of the next launch of an unrelated model.
// The code is reported HERE, once, and cleared.)
#define M_HIP(call)                                                                   \
    do {                                                                              \
        hipError_t e_ = (call);                                                       \
        if (e_ != hipSuccess) {                                                       \
            (void)hipGetLastError();                                                  \
            return m_fail(SPD_E_DEVICE, std::string(#call) + ": " + hipGetErrorString(e_)); \
        }                                                                             \
    } while (0)

// ---- the in-loop features (statistics, tapes, spectra, nudging, breeding): what every _configure does around its own work ----
// A _configure call, behind its argument checks: the model is there, usable and not inside a checked call ...
inline int configure_allowed(const spd_model *m, const char *who) {
    if (!m) return m_fail(SPD_E_ARG, std::string(who) + ": null model");
    if (int rc = usable(m, who)) return rc;
    if (m->steps_pending) return m_fail(SPD_E_ARG, std::string(who) + ": a checked multi-step call is in flight; end it first");
    return SPD_OK;
}
// ... and, behind the checks that need the model: the feature as it was configured goes.  It is OFF before anything can fail --
// here or in the caller below -- so that no later step samples into, or reads, memory whose state is unknown.
template <class Feature>
int retire(spd_model *m, Feature &f) {
    M_HIP(hipSetDevice(m->ctx->device));
    M_HIP(hipDeviceSynchronize());  // (steps in flight may still use the allocation this one replaces)
    void *old = f.alloc;
    f = Feature{};
    if (old) M_HIP(hipFree(old));
    return SPD_OK;
}

constexpr size_t kSampleAlign = 256;
inline size_t sample_up(size_t b) { return (b + kSampleAlign - 1) / kSampleAlign * kSampleAlign; }
// the parts of a feature's one allocation, one behind the other, each starting on a kSampleAlign boundary
struct Carve {
    char *at;
    template <class T>
    T *take(size_t bytes) {
        T *part = reinterpret_cast<T *>(at);
        at += sample_up(bytes);
        return part;
    }
};

// ---- ... and what every _configure and _read does around its own work ----
// an upload into the new allocation `p` failed: the feature stays off
inline int upload_failed(const char *who, hipError_t e, void *p) {
    (void)hipGetLastError();
    (void)hipFree(p);
    return m_fail(SPD_E_DEVICE, std::string(who) + ": " + hipGetErrorString(e));
}

// A _read call of a model that is there: usable, the recorder on ("no ... configured (...)"), no checked call in flight, and
// nothing recorded behind a failed range check ("the ... invalid until spd_model_..._reset")
inline int read_allowed(const spd_model *m, const char *who, bool on, const char *off, const Validity &validity, const char *invalid) {
    if (int rc = usable(m, who)) return rc;
    if (!on) return m_fail(SPD_E_ARG, std::string(who) + ": " + off);
    if (m->steps_pending) return m_fail(SPD_E_ARG, std::string(who) + ": a checked multi-step call is in flight; end it first");
    if (!validity.valid) return m_fail(SPD_E_ARG, std::string(who) + ": " + invalid + ": " + validity.why);
    return SPD_OK;
}
// samples (windows, events) [t0, t0 + nt) of those the ring holds
inline int held_range(const char *who, const SampleRing &ring, int t0, int nt, const char *unit) {
    if (t0 < 0 || nt < 0 || static_cast<long long>(t0) + nt > ring.held())
        return m_fail(SPD_E_ARG, std::string(who) + ": " + unit + " range out of bounds (" + std::to_string(ring.held()) + " " + unit + "s held)");
    return SPD_OK;
}
// `need` bytes into the caller's device buffer
inline int destination_fits(const char *who, const void *dst_device, size_t dst_bytes, size_t need, size_t align) {
    if (!dst_device && need > 0) return m_fail(SPD_E_ARG, std::string(who) + ": null destination");
    if (dst_bytes < need) return m_fail(SPD_E_SIZE, std::string(who) + ": destination too small (" + std::to_string(need) + " bytes needed)");
    if (reinterpret_cast<uintptr_t>(dst_device) % align != 0)
        return m_fail(SPD_E_ARG, std::string(who) + ": the destination must be " + std::to_string(align) + "-byte aligned");
    return SPD_OK;
}

// ---- the catalogue of grid-space names that the statistics, the tapes and the pressure-level fields share ----
struct StatsCatalogueEntry {
    const char *name;
    int levels, unit;  // levels: 0 = the configured target levels; unit: as StatsPlane::unit
    int kind;          // CatKind
};
// where a name's planes come from: the export transforms (an XfSource), the column kernel's precipitation outputs, the
// pressure-level kernel (levels 0: the configured target levels; mslp one), the derived-field kernel (levels 0: likewise)
enum CatKind { CAT_XF = 0, CAT_PRECIP, CAT_PLEV, CAT_DERIVE };
// ids 0 ... 5: from the spectral state through the export transforms; 6, 7: the column kernel's precipitation outputs;
// 8 ... 13: the pressure-level variables (kPlevFirst + PlevVar; levels: the configured target levels, mslp one), written into the
// slab in export units by the pressure-level kernel; 14, 15: vorticity and divergence through the export transforms;
// 16 ... 27: the derived-field kernel's outputs (kDeriveFirst + DeriveVar), written into the slab in export units
constexpr StatsCatalogueEntry kStatsCatalogue[] = {
    {"u_grid", KX, 0, CAT_XF},       {"v_grid", KX, 0, CAT_XF},      {"t_grid", KX, 0, CAT_XF},     {"q_grid", KX, 1, CAT_XF},
    {"phi_grid", KX, 2, CAT_XF},     {"ps_grid", 1, 3, CAT_XF},      {"precnv", 1, 0, CAT_PRECIP},  {"precls", 1, 0, CAT_PRECIP},
    {"u_plev", 0, 0, CAT_PLEV},      {"v_plev", 0, 0, CAT_PLEV},     {"t_plev", 0, 0, CAT_PLEV},    {"q_plev", 0, 0, CAT_PLEV},
    {"z_plev", 0, 0, CAT_PLEV},      {"mslp", 1, 0, CAT_PLEV},       {"vor_grid", KX, 0, CAT_XF},   {"div_grid", KX, 0, CAT_XF},
    {"omega_grid", KX, 0, CAT_DERIVE}, {"rh_grid", KX, 0, CAT_DERIVE}, {"theta_grid", KX, 0, CAT_DERIVE}, {"tcwv", 1, 0, CAT_DERIVE},
    {"ivt_u", 1, 0, CAT_DERIVE},     {"ivt_v", 1, 0, CAT_DERIVE},    {"ke_col", 1, 0, CAT_DERIVE},  {"omega_plev", 0, 0, CAT_DERIVE},
    {"vor_plev", 0, 0, CAT_DERIVE},  {"div_plev", 0, 0, CAT_DERIVE}, {"rh_plev", 0, 0, CAT_DERIVE}, {"theta_plev", 0, 0, CAT_DERIVE}};
constexpr int kPlevFirst = 8, kVorGrid = 14, kDeriveFirst = 16;
// the derived names, and what every recorder's "unknown variable" message appends to the list it has always given
#define SPD_DERIVED_TAIL "; derived fields: " SPD_DERIVED_NAMES
#define SPD_DERIVED_NAMES \
    "vor_grid, div_grid, omega_grid, rh_grid, theta_grid, tcwv, ivt_u, ivt_v, ke_col, omega_plev, vor_plev, div_plev, rh_plev, theta_plev"
inline constexpr int cat_kind(int id) { return kStatsCatalogue[id].kind; }
// the name is computed at the target levels of spd_model_plev_configure (mslp, of one level, is the pressure-level kernel's as well)
inline constexpr bool cat_needs_levels(int id) {
    return cat_kind(id) == CAT_PLEV || (cat_kind(id) == CAT_DERIVE && kStatsCatalogue[id].levels == 0);
}
// What the export transforms can write into a slab: catalogue ids 0 ... 5, vorticity and divergence (catalogue ids 14, 15), and
// the two components of grad ln ps, which no recorder can name (the step's own entries of mode 3 / 4 with kcos = 2).
enum XfSource { XF_U = 0, XF_V, XF_T, XF_Q, XF_PHI, XF_PS, XF_VOR, XF_DIV, XF_PX, XF_PY, XF_N };
constexpr int kXfLevels[XF_N] = {KX, KX, KX, KX, KX, 1, KX, KX, 1, 1};
inline constexpr int xf_source(int id) { return id < 6 ? id : XF_VOR + (id - kVorGrid); }  // of a CAT_XF name
// the XfSource of each sigma-level input of the derived-field kernel (DeriveIn)
constexpr int kDeriveInXf[DIN_N] = {XF_U, XF_V, XF_T, XF_Q, XF_VOR, XF_DIV};
// sigma-level inputs (catalogue ids 0 ... 5, as bits) of each pressure-level variable: ps always; T with Z (both extrapolations)
constexpr int kPlevNeeds[PLEV_NVARS] = {1 << 0 | 1 << 5, 1 << 1 | 1 << 5, 1 << 2 | 1 << 5, 1 << 3 | 1 << 5, 1 << 2 | 1 << 4 | 1 << 5,
                                        1 << 2 | 1 << 5};
constexpr int kStatsCatalogueSize = sizeof(kStatsCatalogue) / sizeof(kStatsCatalogue[0]);
inline int stats_id(const char *name) {
    for (int v = 0; v < kStatsCatalogueSize; ++v)
        if (std::strcmp(name, kStatsCatalogue[v].name) == 0) return v;
    return -1;
}

// ---- the front end of a sample (spd_model::SampleFront), shared by the statistics and the tapes; defined in model.hip ----
struct SamplePlan {
    struct Var {
        int id, levels;
        size_t first_plane;  // planes of the variables before this one (of one member)
    };
    std::vector<Var> vars;
    // what the export transforms write into the slab (XfSource), in slab order: the variables asked for, then those only a
    // pressure-level or derived variable needs; xf_at[x]: first slab plane of source x (-1: not transformed)
    std::vector<int> xf;
    int xf_at[XF_N] = {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1};
    size_t planes = 0;                        // planes of all variables of one member
    size_t slab_bytes = 0, table_bytes = 0;   // of the slab and of ONE descriptor table, rounded up to kSampleAlign
};
// the list of names of a _configure call -> catalogue ids
int sample_ids(const char *who, const char *const *names, int n_names, std::vector<int> &ids);
// the variables `ids` of the model's M members: which planes the slab holds and how large slab and tables are
void plan_sample(const spd_model *m, const std::vector<int> &ids, spd_model::SampleFront &front, SamplePlan &plan);
// uploads the descriptor tables of a front end whose slab and tables point into the caller's allocation; sources: per plane of
// plan.vars, where its value is read from and its unit (sample_source.hpp)
hipError_t build_sample_front(const spd_model *m, const SamplePlan &plan, spd_model::SampleFront &front, std::vector<SampleSource> &sources);
// the launches of a front end for the members [first, first + count) on `s`
hipError_t sample_front(spd_model *m, const spd_model::SampleFront &f, int first, int count, hipStream_t s);
// slab | tables[2] of a front end
inline void carve_front(Carve &carve, const SamplePlan &plan, spd_model::SampleFront &front) {
    front.slab = carve.take<double>(plan.slab_bytes);
    front.table[0] = carve.take<FieldDesc>(plan.table_bytes);
    front.table[1] = carve.take<FieldDesc>(plan.table_bytes);
}

// ---- the entry recorders (projection tape, assimilation, verification tape, quantile tape): the checks of their lists, one per
// check so that each _configure keeps its documented order; the tables built from the lists are entry_front.hpp's ----
#define SPD_CATALOGUE_LIST \
    "u_grid, v_grid, t_grid, q_grid, phi_grid, ps_grid, precnv, precls, u_plev, v_plev, t_plev, q_plev, z_plev, mslp)" SPD_DERIVED_TAIL
// the catalogue id of an entry's name, or -1 behind m_fail; list: the names the recorder takes, from behind the opening bracket
inline int entry_id(const char *who, const char *name, const char *list) {
    const int id = name ? stats_id(name) : -1;
    if (id < 0) m_fail(SPD_E_ARG, std::string(who) + ": unknown variable '" + (name ? name : "(null)") + "' (" + list);
    return id;
}
inline std::string entry_text(int k, const char *name) { return "entry " + std::to_string(k) + " ('" + name + "')"; }
// (against the name's fixed count; a pressure-level name's count is the model's: check_plev_entries)
inline int check_entry_level(const char *who, int k, const char *name, int id, int level) {
    const int fixed = kStatsCatalogue[id].levels;
    if (level < 0 || (fixed > 0 && level >= fixed))
        return m_fail(SPD_E_ARG, std::string(who) + ": level " + std::to_string(level) + " of " + entry_text(k, name) + " is out of range" +
                                     (fixed > 0 ? " (0 ... " + std::to_string(fixed - 1) + ")" : ""));
    return SPD_OK;
}
inline int check_entry_pattern(const char *who, int k, const char *name, int pattern, int n_patterns) {
    if (pattern < 0 || pattern >= n_patterns)
        return m_fail(SPD_E_ARG, std::string(who) + ": pattern " + std::to_string(pattern) + " of " + entry_text(k, name) +
                                     " is out of range (0 ... " + std::to_string(n_patterns - 1) + ")");
    return SPD_OK;
}
// weights: [n_patterns][4608], finite
inline int check_weight_maps(const char *who, const double *weights, int n_patterns) {
    for (int p = 0; p < n_patterns; ++p)
        for (int q = 0; q < NG; ++q)
            if (!std::isfinite(weights[static_cast<size_t>(p) * NG + q]))
                return m_fail(SPD_E_ARG, std::string(who) + ": weight of pattern " + std::to_string(p) + " at point " + std::to_string(q) + " (row " +
                                             std::to_string(q / IX) + ", column " + std::to_string(q % IX) + ") is not finite");
    return SPD_OK;
}
// mask: [members] of 0 / 1 with 2 ... max ones; takes: who takes that many ("the scores take")
inline int check_member_mask(const char *who, const int32_t *mask, int members, int max, const char *takes) {
    int r = 0;
    for (int i = 0; i < members; ++i) {
        if (mask[i] != 0 && mask[i] != 1)
            return m_fail(SPD_E_ARG, std::string(who) + ": the mask of member " + std::to_string(i) + " (" + std::to_string(mask[i]) + ") is not 0 or 1");
        r += mask[i];
    }
    if (r < 2 || r > max)
        return m_fail(SPD_E_ARG, std::string(who) + ": " + std::to_string(r) + " members are masked in: " + takes + " 2 ... " + std::to_string(max));
    return SPD_OK;
}
// a name on the target levels of spd_model_plev_configure while there are none
inline int levels_first(const char *who, const char *name) {
    return m_fail(SPD_E_ARG, std::string(who) + ": '" + name + "' needs target levels (spd_model_plev_configure) first");
}
// once the model is known: the entries on the target levels of spd_model_plev_configure (entries: anything with .name and .level)
template <class Entry>
int check_plev_entries(const spd_model *m, const char *who, const char *const *names, const std::vector<Entry> &entries) {
    for (size_t k = 0; k < entries.size(); ++k) {
        if (!cat_needs_levels(entries[k].name)) continue;  // (mslp, of one level, is the pressure-level kernel's as well)
        if (m->plev.n == 0) return levels_first(who, names[k]);
        if (kStatsCatalogue[entries[k].name].levels == 0 && entries[k].level >= m->plev.n)
            return m_fail(SPD_E_ARG, std::string(who) + ": level " + std::to_string(entries[k].level) + " of " + entry_text(static_cast<int>(k), names[k]) +
                                         " is out of range (0 ... " + std::to_string(m->plev.n - 1) + ")");
    }
    return SPD_OK;
}
// where a plane of a planned name is read from; sources: as build_sample_front left them
inline const SampleSource &plane_source(const SamplePlan &plan, const std::vector<SampleSource> &sources, int name, int level) {
    const auto var = std::find_if(plan.vars.begin(), plan.vars.end(), [&](const SamplePlan::Var &v) { return v.id == name; });
    return sources[var->first_plane + static_cast<size_t>(level)];
}
// a call that reads or moves the state of a model that is there: usable, the feature on, initialised, no checked call in flight
inline int state_call_allowed(const spd_model *m, const char *who, bool on, const char *off) {
    if (int rc = usable(m, who)) return rc;
    if (!on) return m_fail(SPD_E_ARG, std::string(who) + ": " + off);
    if (!m->initialized) return m_fail(SPD_E_ARG, std::string(who) + ": model state not initialized");
    if (m->steps_pending) return m_fail(SPD_E_ARG, std::string(who) + ": a checked multi-step call is in flight; end it first");
    return SPD_OK;
}
// _reset and _rows / _times of a ring recorder (`feature`: its member of spd_model, with on, ring and validity); no device work
template <class Feature>
int ring_reset(spd_model *m, const char *who, Feature spd_model::*feature, const char *off) {
    if (!m) return m_fail(SPD_E_ARG, std::string(who) + ": null model");
    if (!(m->*feature).on) return m_fail(SPD_E_ARG, std::string(who) + ": " + off);
    if (m->steps_pending) return m_fail(SPD_E_ARG, std::string(who) + ": a checked multi-step call is in flight; end it first");
    (m->*feature).ring.clear();
    (m->*feature).validity.clear();
    return SPD_OK;
}
template <class Feature>
int ring_rows(const spd_model *m, const char *who, Feature spd_model::*feature, const char *off, int32_t *rows, int max_rows) {
    if (!m) return m_fail(SPD_E_ARG, std::string(who) + ": null model");
    if (!(m->*feature).on) return m_fail(SPD_E_ARG, std::string(who) + ": " + off);
    if (max_rows < 0 || (max_rows > 0 && !rows)) return m_fail(SPD_E_ARG, std::string(who) + ": bad destination");
    return (m->*feature).ring.copy_rows(rows, max_rows);
}
// The held slots [t0, t0 + nt) of a ring [slot][slot_stride] into dst [members][nt][per]: of each slot, `members` runs of `per`
// doubles from ring_base on, one behind the other (the spectra's gather; a ring of one block per slot is one "member")
inline int gather_slots(const spd_model *m, const char *who, const double *ring_base, size_t per, size_t slot_stride, int members, int t0, int nt,
                        const SampleRing &ring, void *dst, void *stream) {
    if (members == 0 || nt == 0) return SPD_OK;
    M_HIP(hipSetDevice(m->ctx->device));
    const hipError_t e = run_spectra_gather(ring_base, static_cast<double *>(dst), static_cast<int>(per), static_cast<long>(slot_stride), members, nt,
                                            ring.slot_of_held(t0), ring.capacity, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return m_fail(SPD_E_DEVICE, std::string(who) + ": " + hipGetErrorString(e));
    return SPD_OK;
}

}  // namespace spd
