/* pyspeedy_amd -- C ABI of the MI355X-native SPEEDY hot path (spectral transforms + column physics).
 *
 * Drop-in boundary, operator level ("inner boundary"): every entry point replaces
 * one type-bound procedure of the reference's ModSpectral_t (speedy.f90/spectral.f90:19-31) or the
 * column-physics driver (speedy.f90/physics.f90:14), with an explicit batch count added.  A Fortran
 * host binds these with ISO_C_BINDING (INTEGRATION.md shows the interface block); the Python host in
 * pyspeedy_amd/ binds them with ctypes.
 *
 * Conventions
 *   - All field pointers are DEVICE pointers (hipMalloc'ed memory on the handle's device) unless the
 *     name ends in _host.  Nothing is retained after a call returns; all work is ordered on `stream`
 *     (a hipStream_t passed as void*; NULL = the default stream).  No call synchronises the device.
 *   - Layout: batch slowest, the reference's Fortran order inside one field:
 *       spectral field  complex(8) (mx=31, nx=32)  -> 992 complex = 15872 B, index m + 31*n, re/im interleaved
 *       Fourier plane   real(8)    (2*mx=62, il=48)-> 23808 B, index r + 62*j
 *       grid field      real(8)    (ix=96, il=48)  -> 36864 B, index i + 96*j   (j=0 southernmost)
 *   - Return value: 0 = success, negative = SPD_E_* below.  No exceptions, no process exit.
 *   - Thread safety: calls on different handles are independent; a handle may be shared by host threads
 *     (it is immutable after spd_create).
 */
#ifndef PYSPEEDY_AMD_H
#define PYSPEEDY_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPD_IX 96
#define SPD_IL 48
#define SPD_IY 24
#define SPD_KX 8
#define SPD_MX 31
#define SPD_NX 32
#define SPD_TRUNC 30

#define SPD_OK 0
#define SPD_E_ARG (-1)    /* bad argument (null pointer, negative count, unknown name) */
#define SPD_E_DEVICE (-2) /* HIP runtime error (no device, launch failure, ...) */
#define SPD_E_SIZE (-3)   /* caller buffer too small */
#define SPD_E_TIMEOUT (-4) /* a collective did not complete inside its bound; work of unknown state is left on the devices it ran on */

typedef struct spd_context *spd_handle;

/* ---- lifecycle ------------------------------------------------------------------------------
 * spd_create: builds the transform / geometry / radiation tables on the host exactly as the reference's
 * ModGeometry_initialize (geometry.f90:67), ModLegendre_initialize (legendre.f90:38), rffti1
 * (fftpack.f90:1), ModSpectral_initialize (spectral.f90:39) and radset (longwave_radiation.f90:208) do,
 * and uploads them to device `device`.  Replaces state%mod_geometry/mod_spectral%initialize
 * (initialization.f90:41-44). */
int spd_create(spd_handle *out, int device);
int spd_destroy(spd_handle h);
int spd_device(spd_handle h);
const char *spd_last_error(void);
const char *spd_version(void);

/* Host copy of a table by the reference's name ("sia_half", "cpol", "work", "el2", "fband", ...).
 * Doubles, Fortran order.  Integer tables ("nsh2", "ifac") are returned converted to double.
 * Returns the element count, or a negative error.  With buf == NULL only the count is returned.
 * h may be NULL: the tables are then built on the host without touching any device. */
long spd_get_table_host(spd_handle h, const char *name, double *buf_host, size_t buf_elems);

/* Host-only (no device is touched): the model calendar, model_control.f90:79-185 -- initialize_control at the given start date,
 * then `nsteps` times advance_date (one 40-minute step each: February has 29 days when mod(year, 4) == 0, :135-142; the month
 * counter month_idx keeps counting across the year end, :153-157) with update_forcing_params (:162-185: imont1, tmonth, tyear in
 * the reference's default-real arithmetic).  Row 0 of every output is the state after initialize_control, row s the state
 * after s steps; ymdhm is [nsteps + 1][5] (year, month, day, hour, minute).  Any output pointer may be NULL.  This is the
 * calendar spd_model_step advances on the host beside the device state. */
int spd_calendar_walk(int year, int month, int day, int hour, int minute, int nsteps, int32_t *ymdhm, int32_t *month_idx,
                      int32_t *imont1, double *tmonth, double *tyear);
/* Host-only: the zonally uniform daily forcing of set_forcing / get_zonal_average_fields (forcing.f90:84-101,
 * shortwave_radiation.f90:218-322) for a fraction of the year `tyear`: out[5][48] = flux_solar_in, flux_ozone_upper,
 * flux_ozone_lower, zenit_correction, stratospheric_correction by latitude (south to north), as the model uploads them once
 * per simulated day. */
int spd_daily_forcing_host(double tyear, double *out);

/* ---- spectral transforms (spectral.f90:251-273, legendre.f90:130-221, fourier.f90:63-123) ---- */
/* spec2grid: kcos == 1 -> no scaling, otherwise multiply row j by cosgr(j) (fourier.f90:87-91). */
int spd_spec2grid(spd_handle h, const double *spec, double *grid, int kcos, int nfields, void *stream);
int spd_grid2spec(spd_handle h, const double *grid, double *spec, int nfields, void *stream);
/* the two stages separately (same kernels, one stage disabled); `four` is the Fourier plane */
int spd_legendre_inv(spd_handle h, const double *spec, double *four, int nfields, void *stream);
int spd_legendre(spd_handle h, const double *four, double *spec, int nfields, void *stream);
int spd_fourier_inv(spd_handle h, const double *four, double *grid, int kcos, int nfields, void *stream);
int spd_fourier(spd_handle h, const double *grid, double *four, int nfields, void *stream);

/* ---- spectral-space operators (spectral.f90:134-317) ------------------------------------------ */
int spd_vort2vel(spd_handle h, const double *vor, const double *div, double *ucos, double *vcos, int nfields,
                 void *stream);
int spd_vel2vort(spd_handle h, const double *ucos, const double *vcos, double *vor, double *div, int nfields,
                 void *stream);
/* grid_vel2vort: kcos == 2 -> pre-multiply by cosgr, otherwise by cosgr2 (spectral.f90:229-243)
 * spd_grid_vel2vort and spd_grid_filter keep their spectral intermediates in ONE scratch buffer per handle, which lives until
 * spd_destroy and only ever grows.  Calls of either on one handle must therefore be ordered on one stream (or by the caller's
 * own events): two of them in flight on different streams would share the buffer.  A call with a larger batch than any before
 * it on that handle frees and reallocates the buffer and synchronises the DEVICE first (hipDeviceSynchronize: it is not
 * stream-ordered and cannot be captured into a graph); size the buffer beforehand with one call of spd_grid_vel2vort at the
 * largest batch.  spd_grid_filter may work in place (fg1 == fg2). */
int spd_grid_vel2vort(spd_handle h, const double *ug, const double *vg, double *vor, double *div, int kcos,
                      int nfields, void *stream);
int spd_gradient(spd_handle h, const double *psi, double *psdx, double *psdy, int nfields, void *stream);
int spd_laplacian(spd_handle h, const double *in, double *out, int inverse, int nfields, void *stream);
int spd_truncate(spd_handle h, double *field, int nfields, void *stream);
int spd_grid_filter(spd_handle h, const double *fg1, double *fg2, int nfields, void *stream);

/* ---- column physics (physics.f90:14-256 from line 107 on; the 41 spec2grid calls of lines 89-101 are
 *      issued by the caller through spd_vort2vel / spd_spec2grid so that they can be batched) ----------
 * One call processes `nmembers` ensemble members; every array below is member-major:
 * [nmembers][...reference shape...].  Shapes in comments are the reference's (Fortran order). */
typedef struct spd_physics_args {
    /* grid-point state at time level 1 (physics.f90:89-101) */
    const double *ug, *vg, *tg, *qg, *phig; /* (ix,il,kx) */
    const double *pslg;                     /* (ix,il)  log surface pressure */
    /* dynamics tendencies, updated in place (physics.f90:31-34) */
    double *utend, *vtend, *ttend, *qtend; /* (ix,il,kx) */
    /* surface and forcing fields (physics.f90:177-185) */
    const double *fmask_land, *phis0, *forog, *sst_am, *alb_land, *alb_sea, *snowc, *land_temp, *soil_avail_water;
    /* daily shortwave forcing (shortwave_radiation.f90:88-168, 212) -- read only when compute_shortwave != 0 */
    const double *flux_solar_in, *flux_ozone_upper, *flux_ozone_lower, *zenit_correction, *stratospheric_correction,
        *alb_surface;
    /* outputs written every step (ModelState_t fields of the same names) */
    double *precnv, *precls, *cbmf, *slrd, *slr, *olr;   /* (ix,il) */
    double *slru, *ustr, *vstr, *shf, *evap, *hfluxn;    /* (ix,il,3) ; hfluxn planes 1:2 written */
    double *rad_st4a;                                     /* (ix,il,kx,2) */
    double *rad_flux;                                     /* (ix,il,4) */
    /* radiation state that persists between shortwave steps (written when compute_shortwave != 0) */
    double *tt_rsw;         /* (ix,il,kx) */
    double *rad_tau2;       /* (ix,il,kx,4) */
    double *rad_strat_corr; /* (ix,il,2) */
    double *tsr, *ssrd, *ssr, *qcloud_equiv; /* (ix,il) */
    /* optional diagnostics, may be NULL: iptop/icltop as doubles would lose nothing but stay int32 */
    int32_t *iptop, *icltop;                  /* (ix,il) */
    double *ts, *tskin, *u0, *v0, *t0, *cloudc, *clstr; /* (ix,il) */
    double air_absortivity_co2; /* state%air_absortivity_co2 */
    int32_t compute_shortwave;  /* state%compute_shortwave (speedy.f90:53) */
    int32_t fp32; /* != 0: column arithmetic in single precision (cfg 5); inputs / outputs stay double */
    /* SPPT pattern (ix,il,kx), values outside [-1, 1] are clipped; NULL = off (physics.f90:234-248, sppt_on = .false.) */
    const double *sppt_pattern;
} spd_physics_args;

int spd_physics(spd_handle h, const spd_physics_args *args, int nmembers, void *stream);

/* ---- streaming-rate probe (measurement infrastructure; no counterpart in the reference -- SURVEY.md section 8d: "report
 *      measured copy / triad bandwidth on the box and use the spec peak for the contract fraction") -------------------------
 * What a kernel that only moves bytes reaches on this device in a given SHAPE, with kernels of this library (csrc/
 * stream_probe.hip): one wavefront per 64-thread workgroup; a wavefront requests `in_flight` rows (64 lanes x lane_bytes,
 * contiguous) of each of its `reads` input streams back to back, adds them and stores `in_flight` rows to each of its
 * `writes` output streams, and repeats until it has touched about `rows_per_wave` rows of all its streams together (1: a
 * plain copy kernel's one row and out; 243: the column kernel's life).  The streams lie far apart in memory.  The probe
 * allocates total_bytes itself, launches 2 + reps times and times every launch by the time stamps of its dispatch packet.
 * The step's kernels are priced against 8 TB/s in bench.py's `roofline`; this is the ceiling to read those fractions against. */
typedef struct spd_stream_probe_args {
    int32_t reads, writes;  /* streams: 1:1 (copy), 2:1 (the column kernel's mix), 3:2, 1:0 (read only), 0:1 (write only) */
    int32_t lane_bytes;     /* 8 (the column kernel: one double per lane) or 16 (the transforms' staging) */
    int32_t in_flight;      /* rows per stream requested before the first use: 1, 2, 4, 8, 16 */
    int32_t nontemporal;    /* 0 / 1: the non-temporal hint on loads and stores (csrc/stream_store.hpp) */
    int32_t waves_per_simd; /* 1 ... 8 wavefronts per SIMD, held there by dynamic LDS (2: the column kernel at 256 VGPRs) */
    int32_t rows_per_wave;  /* rows of all streams together a wavefront works through before it ends */
    int32_t reps;           /* timed launches, 1 ... 1000 */
    int32_t layout;         /* 0: a wavefront walks a contiguous chunk of its own in every stream; 1: the column kernel's -- row r of every
                             * wavefront lies in array r of the stream, consecutive wavefronts side by side inside each array */
    int32_t reserved;
    uint64_t total_bytes;   /* bytes one launch moves, reads + writes (rounded down to whole wavefronts) */
} spd_stream_probe_args;
/* mean and minimum duration of a launch in microseconds; optionally the bytes a launch really moved and its workgroups */
int spd_stream_probe(spd_handle h, const spd_stream_probe_args *args, double *mean_us, double *min_us, uint64_t *bytes_moved,
                     uint64_t *workgroups);

/* ---- ensemble model object: device-resident state of M members and the model time step ------------------------
 * Replaces, for M members at once, the reference's ModelState_t container (model_state.f90) and
 * time_stepping.f90:38-147 `step` (get_tendencies -> horizontal diffusion -> leapfrog + Robert/Williams filter), i.e. what
 * speedy_driver.f90.j2:43-79 (`step`, `parallel_step`) reach through do_single_step.  The state never leaves HBM; every
 * array is member-major with the reference's Fortran order inside a member, so get/set are plain copies.
 * Variable names are the registry names of registry/model_state_def.py (vor, div, t, tr, ps, phi, phis, precnv, ...,
 * rad_tau2, ...); two arrays the registry does not expose are added: tcorh, qcorh (mod_implicit%tcorh/qcorh,
 * forcing.f90:84,101). */
typedef struct spd_model *spd_model_handle;

int spd_model_create(spd_handle h, int nmembers, spd_model_handle *out);
/* (waits for the device; the model's memory block is kept by its context for the next model of the same size, up to 1 GiB per
 * context, and returned to the device with the context) */
int spd_model_destroy(spd_model_handle m);
int spd_model_members(spd_model_handle m);
/* device memory of the model, all members: bytes reserved (a few large blocks the arrays are carved from) and bytes in use */
int spd_model_memory(spd_model_handle m, size_t *bytes_reserved, size_t *bytes_used);
/* bytes of one member's copy of `name`, or a negative error */
long spd_model_var_bytes(spd_model_handle m, const char *name);
/* host <-> device copy of one member's array (get_<v>/set_<v> of speedy_driver.f90.j2:250-334); member = -1 in
 * spd_model_set broadcasts the same host array to every member.  Synchronous. */
int spd_model_set(spd_model_handle m, const char *name, int member, const void *host_buf, size_t bytes);
int spd_model_get(spd_model_handle m, const char *name, int member, void *host_buf, size_t bytes);
/* Device base pointer of a registry array ([nmembers][...]), for zero-copy users.  Contract:
 *  - the address stays valid (and stays the array of that name) until spd_model_destroy, except "sst_anom" after
 *    spd_model_init_sst_anom and the SPPT arrays before spd_model_set_sppt;
 *  - taking the address of "phi" pins the geopotential to one buffer: the model stops alternating between two (the
 *    look-ahead it otherwise uses for launches of up to 8 members), which costs such ensembles 1-3 % per step;
 *  - the kernels of a step are stream-ordered on the stream given to spd_model_step: read or write through the pointer
 *    on that stream, or synchronise first;
 *  - the call itself drops what the model had derived from the state (look-ahead geopotential, the day's interpolated
 *    climatologies).  A caller that WRITES through a pointer it obtained earlier -- spectral t / phis, a climatology or
 *    anomaly field, anything -- must call spd_model_invalidate before the next step, or the step uses the stale values. */
void *spd_model_device_ptr(spd_model_handle m, const char *name);
/* the state was changed behind the model's back (a write through a device pointer): drop everything derived from it */
int spd_model_invalidate(spd_model_handle m);
int spd_model_set_co2(spd_model_handle m, double air_absortivity_co2);
/* current value (the daily forcing raises it when increase_co2 is set, forcing.f90:52-57) */
double spd_model_co2(spd_model_handle m);
/* ModImplicit_set_time_step (implicit.f90:83-218): rebuilds the dt-dependent tables (8x8 inversions on the host) */
int spd_model_set_time_step(spd_model_handle m, double dt);
/* time_stepping.f90 `step(state, j1, j2, dt)` for all members; j1, j2 = 1 or 2 as in the reference */
int spd_model_step_dynamics(spd_model_handle m, int j1, int j2, double dt, int compute_shortwave, void *stream);
/* check_diagnostics (diagnostics.f90:16-76) for every member: error_codes_host[i] = 0 or -2; diag_host may be NULL or
 * receive [nmembers][3][kx] (eddy KE of vor, of div, global-mean T).  Synchronises `stream`. */
int spd_model_check(spd_model_handle m, int time_level, int32_t *error_codes_host, double *diag_host, void *stream);
/* The same check without stalling the launch pipeline: _begin enqueues it and returns a slot (0 or 1, whichever is
 * free; at most two in flight: a third _begin fails with SPD_E_ARG until one has been ended), _end waits for that slot only.  Begin the check of
 * step k, launch step k + 1, then end the check of step k. */
int spd_model_check_begin(spd_model_handle m, int time_level, void *stream);
int spd_model_check_end(spd_model_handle m, int slot, int32_t *error_codes_host);
/* spd_model_check_begin without a launch of its own: the check is put off and rides in the first launch of the NEXT
 * spd_model_step on this stream (`members` more workgroups of its spectral -> grid launch), on the state exactly as it is now --
 * for hosts that collect the check of step k after they have enqueued step k + 1 (spd_parallel_step_begin / _end: the range check
 * then costs the step's stream nothing, 5 % of the step at 64 members, 11 % at one).  Anything else that would read or change the
 * state first -- spd_model_set, the export transforms, member copies, a call of several steps in member groups, spd_model_check_end
 * itself -- makes it a launch of its own there and then.  Returns the slot for spd_model_check_end. */
int spd_model_check_defer(spd_model_handle m, int time_level, void *stream);
/* launches the check spd_model_check_defer put off under `slot` (-1: whichever one is waiting) now, if it is still waiting for a
 * step to carry it; a check put off under another slot keeps waiting for its step.  Afterwards spd_model_check_end of that slot
 * is a pure wait (a host may then make that call outside the lock it serialises its other calls on this model with) */
int spd_model_check_settle(spd_model_handle m, int slot);
/* how many of the model's begun / deferred range checks went out as launches of their own and how many rode in a step's launch */
int spd_model_check_counts(spd_model_handle m, int32_t *alone, int32_t *rode);
int spd_model_checks_in_flight(spd_model_handle m); /* 0, 1 or 2: checks begun and not yet ended */

/* initialize_state (initialization.f90:13-91) for every member from the boundary fields stored beforehand with
 * spd_model_set (orog, fmask_orig, alb0, veg_high, veg_low, stl12, snowd12, soil_wc_l1, soil_wc_l2, sst12,
 * sea_ice_frac12 and optionally sst_anom, i.e. what pyspeedy/speedy.py:279-296 sets): land/sea preprocessing, spectrally
 * truncated orography, resting reference atmosphere, coupler initialisation, forcing, first_step. */
int spd_model_init(spd_model_handle m, int year, int month, int day, int hour, int minute, void *stream);
/* do_single_step (speedy.f90:20-74) `nsteps` times for all members: daily forcing, shortwave every third step, leapfrog
 * step, date advance, land/sea coupling.  Stream-ordered, no synchronisation; returns SPD_E_ARG when the state was not
 * initialised (the reference's error code -1).  spd_model_check runs the reference's per-step range check on demand.
 * A call of several steps on a model of 20 members or more issues the members in 2 or 3 groups on streams of the model's own
 * (forked from and joined to `stream` around the call).  The FIRST such call creates them and spends a few milliseconds making
 * sure they sit on different hardware queues (it measures: HIP's hand-out depends on every stream the process created before,
 * and two group streams on one queue run one after the other); that first call blocks the host for that long. */
int spd_model_step(spd_model_handle m, int nsteps, void *stream);
/* The same `nsteps` steps with the range check of EVERY step (diagnostics.f90:16-76, which the reference's time loop runs after each
 * do_single_step: pyspeedy/speedy.py:396-405) recorded by the device: for hosts that know they will not look at the state before
 * nsteps steps have passed (no callback due before).  One call instead of nsteps -- with the member groups and rounds of the
 * multi-step plan -- and still every step's code: the check of step k rides in the spectral -> grid launch of step k + 1, the last
 * one is a launch of its own.  _begin enqueues everything and returns; _end waits and reports per member the first step of the call
 * whose check failed (0-based; -1: none) and, in `accepted` ([members][7], may be NULL), the model's step counter, date (year,
 * month, day, hour, minute) and month index after the member's last ACCEPTED step (the one before its first failure, else the
 * last of the call).  The device does not stop at a failed check: the steps behind it run on a state the model does not accept;
 * after a failure the only defined continuation is spd_model_init.  One such call may be in flight per model; nsteps <= 4096. */
int spd_model_step_checked_begin(spd_model_handle m, int nsteps, void *stream);
int spd_model_step_checked_end(spd_model_handle m, int32_t *first_failed_step, int32_t *accepted);
int spd_model_current_step(spd_model_handle m);
int spd_model_get_date(spd_model_handle m, int *ymdhm /* 5 ints */);
/* declare a state loaded through spd_model_set as initialised at the START of a run: step counter and date as given, month
 * index 1, CO2 reference = the current absorptivity (what set_forcing(imode = 0) does, forcing.f90:40) */
int spd_model_mark_initialized(spd_model_handle m, int current_step, int year, int month, int day, int hour, int minute);
/* Everything the model keeps on the host between steps (ControlParams_t / Datetime_t of model_control.f90:19-47, the
 * registry scalars of model_state_def.py:305-423 and the SPPT generator position).  Together with the registry arrays
 * (spd_model_get / _set) this IS the state of a run: _get + the arrays make a checkpoint, _set + the arrays resume it
 * bit for bit at any step -- after a month boundary (month_idx selects the sst_anom planes), with the CO2 trend on
 * (ablco2_ref is the untrended reference value) and with SPPT on (the AR(1) pattern sppt_spec continues at sppt_step).
 * spd_model_set_control marks the model initialised and resets nothing. */
typedef struct spd_model_control {
    int32_t current_step;
    int32_t year, month, day, hour, minute; /* model date */
    int32_t month_idx;                      /* months started since the run began, + 1: plane of sst_anom */
    int32_t land_coupling_flag, sst_anomaly_coupling_flag, increase_co2;
    int32_t sppt_on, sppt_first, physics_fp32;
    int32_t reserved;
    int64_t sppt_step, sppt_first_member_id;
    uint64_t sppt_seed;
    double air_absortivity_co2, ablco2_ref;
} spd_model_control;
int spd_model_get_control(spd_model_handle m, spd_model_control *out);
int spd_model_set_control(spd_model_handle m, const spd_model_control *in);
/* measurement hook: HIP events on the launch stream for the kernels of every step.  level 0 = off, 1 = the dominant kernel
 * only (the 77*M-field spectral->grid launch), 2 = every kernel of the step.  The events of a step kernel are attached to its
 * dispatch (hipExtLaunchKernel): they hold the kernel's own begin / end time stamps, as rocprofv3's kernel trace does, and no
 * marker packets sit between the launches (only the daily forcing, three launches, is bracketed by recorded events).  While the level
 * is not 0 the step is issued as ONE member group on the caller's stream (the serial plan), whatever "member_groups" says:
 * kernels of overlapping groups share the GPU and their durations would not be their own.
 * _read synchronises the events of the spectral->grid launches and returns their mean time in ms;
 * _read_kernels returns, per kernel id SPD_K_*, mean and minimum bracket time in ms, the number of brackets and the units
 * (fields for the transforms, members otherwise) one bracket processed; all four arrays hold SPD_K_COUNT entries. */
#define SPD_K_GEOPOTENTIAL 0  /* geopotential_kernel */
#define SPD_K_SPEC2GRID 1     /* spec2grid_table_kernel, 91 (77 pruned) fields per member */
#define SPD_K_COLUMN_SW 2     /* fused grid-point dynamics + column physics, shortwave step */
#define SPD_K_COLUMN 3        /* the same on the two steps out of three without shortwave */
#define SPD_K_GRID2SPEC 4     /* grid2spec_table_kernel, 73 fields per member */
#define SPD_K_SPECTRAL_STEP 5 /* spectral_step_kernel */
#define SPD_K_COUPLER 6       /* coupler_kernel */
#define SPD_K_FORCING 7       /* daily: forcing_kernel + the two 1-field-per-member transforms of tcorh / qcorh */
#define SPD_K_SPPT 8          /* SPPT on: AR(1) update + 8 fields per member spectral->grid */
#define SPD_K_DYN_GRID 9      /* split mode: dyn_grid_kernel */
#define SPD_K_PHYSICS_SW 10   /* split mode: physics_kernel, shortwave step */
#define SPD_K_PHYSICS 11      /* split mode: physics_kernel, other steps */
#define SPD_K_COUNT 12
int spd_model_profile(spd_model_handle m, int level);
int spd_model_profile_read(spd_model_handle m, double *mean_ms, int *launches, int *fields_per_launch);
int spd_model_profile_read_kernels(spd_model_handle m, double *mean_ms, double *min_ms, int *launches, int *units);
/* how the step is configured (environment switches read at spd_model_create): cfg[0] = spectral->grid transforms per member
 * and step (77, or the reference's 91 with PYSPEEDY_AMD_PRUNE_DEAD=0), cfg[1] = 1 when every step stores the diagnostics-only
 * physics outputs (PYSPEEDY_AMD_DIAG_EVERY_STEP=1; default 0: only the last step of a multi-step call does), cfg[2] = member
 * groups stepped on separate streams (PYSPEEDY_AMD_CHUNKS / "member_groups"; the configured number), cfg[3] = 1 for separate dynamics / physics launches, cfg[4] = 1
 * when spectral_step_kernel also computes the next step's geopotential, cfg[5] = 1: it carries the land / sea-ice coupling (always),
 * cfg[6] = 1 for fp32 arithmetic in the column physics, cfg[7] = 1 while the arrays only the column physics reads back are stored
 * as fp32 (spd_model_set_physics_precision) */
int spd_model_get_config(spd_model_handle m, int32_t *cfg /* 8 */);
/* the streams the member groups of multi-step calls are issued on: how many the model has created so far, and whether each was
 * measured to run side by side with the others when it was created (0: after several replacements two of them still shared a
 * hardware queue -- their groups then run one after the other; PYSPEEDY_AMD_STREAMS_APART=2 reports the measurements) */
int spd_model_group_streams(spd_model_handle m, int32_t *created, int32_t *apart);
/* The launch-plan switches that can change on a live model, by name (the environment variables of README.md set the same
 * fields when the model is created; none of them changes the state a step leaves behind):
 *   "diag_every_step"      0 / 1   store the diagnostics-only physics outputs on every step of a multi-step call
 *   "spectral_early"      -1 / 0 / 1   spectral_step_kernel with all loads up front: automatic (up to 8 members) / never / always
 *   "split_dyn"            0 / 1   separate launches for grid-point dynamics and column physics (fp64 physics only; the dynamics kernel
 *                                  then stores the flux and kinetic-energy products and the forward transforms read them, where
 *                                  the fused launch leaves them to be formed inside the transforms: same bits)
 *   "member_groups"        1 ... 4 the members are stepped in that many groups on separate HIP streams (default: 1 below 20
 *                                  members, 2 for 20 ... 23 and from 64 up, 3 for 24 ... 63; always 1 while spd_model_profile is on, for calls of a single step and with split_dyn)
 *   "block_members"        0, n    (default 32, PYSPEEDY_AMD_BLOCK_MEMBERS) from 4 n members up a multi-step spd_model_step takes the
 *                                  members in rounds of member_groups x n, a round through all steps of the call before the next
 *                                  starts (the cross-step hand-over of a group's spectral state then stays in the Infinity Cache;
 *                                  bitwise the same state); 0: everybody together
 *   "physics_storage32"    0 / 1   (default 1, PYSPEEDY_AMD_PHYS_STORE32) with spd_model_set_physics_precision(m, 1): keep the arrays
 *                                  only the column physics reads back as fp32 in memory (1) or as fp64 (0: same arithmetic, same
 *                                  bits in the state, 13 % more bytes in the column kernel); converts the arrays when it changes
 *   "tau_recompute"        0 / 1 / 2   (default 1, PYSPEEDY_AMD_TAU_RECOMPUTE) inside a multi-step call the fused column kernel hands the
 *                                  longwave transmissivities from a shortwave step to the next two steps as the ten values per
 *                                  column they are made of and recomputes them (same bits), and stores rad_tau2 itself on the
 *                                  call's last shortwave step only -- 1: where 20 members and more step together (the
 *                                  ensemble, or a round of it), from where the kernel waits on memory; 2: whatever the size; 0: every
 *                                  shortwave step stores rad_tau2, every other step loads it
 *   "prepare_multi_step"   1       create the streams of the member groups now instead of at the first multi-step call (write-only)
 *   "fail_launch_after"    n, -1   fault injection for tests: the (n + 1)-th launch sequence of a member group from now on fails like a
 *                                  device error (-1: off); spd_model_init clears it (write-only)
 * Returns SPD_E_ARG for an unknown name or a value outside the list.  What is fixed at creation (the pruned transform
 * table, the geopotential fold) is read from the environment only. */
int spd_model_set_option(spd_model_handle m, const char *name, int32_t value);
/* ... and read back, by the same names.  Two names are read-only:
 *   "staged_products"      1 when the step's grid -> spectral launch forms the 40 flux / kinetic-energy products of a member itself,
 *                          from the four grid fields they are products of (the fused column kernel does not store them); 0 when
 *                          it reads them from memory (split_dyn with the fp64 physics)
 *   "quiet_rim_members"    the number of members whose coefficients beyond the truncation's halo (m + n >= 33) the last call of
 *                          spd_model_step / spd_model_step_checked_begin found to be all-zero bits at its first step, and whose
 *                          dead coefficient blocks its later steps therefore left alone; -1 when that call did not look (a call of
 *                          one step, or launches that fold the geopotential: ensembles of up to 8 members).  Waits for the device. */
int spd_model_get_option(spd_model_handle m, const char *name, int32_t *value);
/* BASELINE cfg 5: fp32 != 0 runs the arithmetic of the column physics (physics.f90:107-256 and the schemes it calls) in
 * single precision; the model state, the grid-point dynamics and the tendencies handed to the transforms stay fp64 (the
 * physics increment is formed in fp32 and added to the fp64 dynamics tendency).  Not bitwise comparable with the reference:
 * tests/test_cfg5_gpu.py states the error bounds.  Default 0.
 * The arrays that only the column physics reads back change their STORAGE with it: its grid-point inputs at the physics' time
 * level (the work arrays t/q/phi/u/v_grid_phys, pslg_phys), the radiation state a shortwave step leaves for the next two steps
 * (tt_rsw, rad_tau2, rad_strat_corr) and the diagnostics-only outputs rad_st4a, rad_flux, precnv, precls, cbmf, slrd, slr, olr,
 * slru, ustr, vstr are kept as fp32 in the first half of their allocations (the fp32 kernel narrows each of these values before
 * it uses it and computes each one it stores in fp32: nothing is lost, 13 % of the column kernel's and 11 % of the
 * spectral -> grid launch's bytes are).  spd_model_get / _set (and the driver's spd_get / spd_set) keep speaking fp64 and
 * convert; spd_model_device_ptr hands out the array as stored: ask spd_model_var_storage (8 or 4 bytes per element).
 * Switching converts the arrays in place (synchronises the device); spd_model_set_control with another physics_fp32 switches
 * the model first, and spd_model_copy_member makes the receiving model take over the source's physics precision (its members
 * then all run with it: members of one model share their control block). */
int spd_model_set_physics_precision(spd_model_handle m, int fp32);
int spd_model_var_storage(spd_model_handle m, const char *name);
/* registry scalars land_coupling_flag, sst_anomaly_coupling_flag, increase_co2 (model_state_def.py:305-418) */
int spd_model_set_flags(spd_model_handle m, int land_coupling_flag, int sst_anomaly_coupling_flag, int increase_co2);

/* Grid-space views of the prognostic state in output units, members [first, first + count)
 * (prognostics.f90:125-219; `transform_spectral2grid`, `transform_grid2spectral`, `apply_grid_filter` of
 * speedy_driver.f90.j2:94-125).  Variables u_grid, v_grid, t_grid, q_grid (kg/kg), phi_grid (m), ps_grid (Pa). */
int spd_model_spectral2grid(spd_model_handle m, int first, int count, void *stream);
int spd_model_grid2spectral(spd_model_handle m, int first, int count, void *stream);
int spd_model_grid_filter(spd_model_handle m, int first, int count, void *stream);
/* One grid-space registry variable ((ix, il) or (ix, il, kx) per member, e.g. "t_grid" after spd_model_spectral2grid) of the
 * members [first, first + count) as a NetCDF-3 file carries it -- float32, BIG-endian, vertical levels bottom-up (the reference's
 * export conventions, pyspeedy/speedy.py:415-477) -- into dst_device[count][levels][48][96] (4 bytes each), stream-ordered.  For
 * hosts that write files: narrowing, level order and byte order happen on the GPU, and what crosses PCIe is the file's payload. */
int spd_model_export_pack(spd_model_handle m, const char *name, int first, int count, void *dst_device, size_t dst_bytes,
                          void *stream);
/* Time-mean statistics of grid-space fields, accumulated on the device inside spd_model_step / spd_model_step_checked_begin calls
 * of any length: per member and grid point the number of samples, the mean and (optionally) the unbiased time variance, fp64
 * (Welford's update).  Variables: any of u_grid, v_grid, t_grid, q_grid, phi_grid (kx levels), ps_grid, precnv, precls (and the
 * pressure-level variables of spd_model_plev_* below), in the
 * units and layout spd_model_spectral2grid + spd_model_get give (q kg/kg, phi m, ps Pa; precnv / precls as the column physics
 * stores them).  A sample is taken after every step that leaves the model's absolute step counter at a multiple of `every` --
 * whatever way the host cuts its calls -- and equals what spd_model_spectral2grid would give if the call had ended there.
 * Sampling changes nothing of the run: the state and every registry variable, u_grid ... ps_grid included, are bitwise those of a
 * run without statistics.  Each member group samples its own members on its own stream behind its last launch of the step.
 *   _configure  allocates the accumulators (synchronises the device) and starts a new period; n_names = 0 switches sampling off.
 *               SPD_E_ARG for an unknown or repeated name, every < 1, or while a checked call is in flight.
 *   _reset      starts a new averaging period (host only, no device work).  spd_model_init does the same.
 *   _samples    samples taken since the period started.
 *   _read       members [first, first + count) of one variable, kind SPD_STATS_MEAN or SPD_STATS_VARIANCE, as fp64 into
 *               dst_device[count][levels][48][96] (the layout of the registry variable), stream-ordered.
 *   _ensemble   over all members of the model, per point: kind SPD_STATS_MEAN (the mean of the members' time means) or
 *               SPD_STATS_STD (their standard deviation, ddof 1) into dst_device[levels][48][96], fp64, stream-ordered.
 * Reads fail (SPD_E_ARG, with the reason) before configuring, for a variable that is not configured, before the first sample
 * (before the second for the variance), while a checked call is in flight, and after a checked call that reported a failed
 * range check: the samples behind a failed step are garbage; the statistics stay invalid until _reset or spd_model_init.
 * spd_model_copy_member does not carry statistics, and the outer boundary (spd_parallel_step*, include/pyspeedy_amd_driver.h)
 * does not keep them across the models it merges and splits. */
#define SPD_STATS_MEAN 0
#define SPD_STATS_VARIANCE 1
#define SPD_STATS_STD 2
int spd_model_stats_configure(spd_model_handle m, const char *const *names, int n_names, int every, int with_variance);
int spd_model_stats_reset(spd_model_handle m);
int spd_model_stats_samples(spd_model_handle m);
int spd_model_stats_read(spd_model_handle m, const char *name, int kind, int first, int count, void *dst_device, size_t dst_bytes,
                         void *stream);
int spd_model_stats_ensemble(spd_model_handle m, const char *name, int kind, void *dst_device, size_t dst_bytes, void *stream);
/* Pressure-level fields and mean sea-level pressure, computed on the device from the sigma-level grid fields in export units
 * (what spd_model_spectral2grid leaves: T in K, u, v in m/s, q in kg/kg, phi_grid in m, ps_grid in Pa).  Target pressures p_j in
 * Pa (the Python layer speaks hPa), at most 32, strictly positive, strictly increasing or strictly decreasing; results keep the
 * caller's order.  Per member and column, with s = ln(p_j / ps) and the full levels at sigl[k] = ln(fsg[k]) (k = 0 top ... 7):
 *   inside  (sigl[0] <= s <= sigl[7])  X[k] + w (X[k+1] - X[k]), w = (s - sigl[k]) / (sigl[k+1] - sigl[k]): linear in ln p
 *   above   (s < sigl[0])              u, v, T, q of level 0; Z = Z[0] + (R/g) T[0] (sigl[0] - s)        (isothermal)
 *   below   (s > sigl[7])              u, v, q of level 7; T = T[7] exp(kappa (s - sigl[7])), Z = Z[7] - (T - T[7]) / gamma,
 *                                      kappa = R gamma / g                               (constant lapse rate, hydrostatic)
 *   mslp    ps (1 + gamma z_s / T_s)^(g / (R gamma)), T_s = T[7] exp(-kappa sigl[7]), z_s = phis0 / g
 * with the library's R, g and gamma = 6 K/km.  Points under the ground (p_j > ps) are extrapolated like any other point below
 * level 7: they are NOT masked; ps_grid tells which they are.  Names: u_plev, v_plev, t_plev, q_plev, z_plev (n levels), mslp.
 * They are derived fields, not state: spd_model_get / _set, restarts and spd_model_copy_member do not know them.
 *   _configure  sets the target levels (n = 0 clears them; host only).  SPD_E_ARG for more than 32, a non-positive or unsorted
 *               level, and while statistics of a pressure-level variable are configured.
 *   _levels     the configured levels into out[0 .. cap); returns their number.
 *   _compute    members [first, first + count): with refresh = 1 first spd_model_spectral2grid of those members; with
 *               refresh = 0 the grid arrays are taken as they are (the caller has just made that call, or has written fields of
 *               its own there).  Then one kernel from u_grid ... ps_grid and phis0 into the result arrays, which are allocated
 *               the first time a variable is asked for.  n_names = 0: all six.  The spectral state is not touched.
 *   _read       a computed result as fp64 into dst_device[count][n][48][96] (mslp: [count][48][96]), device to device,
 *               stream-ordered.
 * spd_model_stats_configure takes the six names next to its own once levels are configured: a sample then also transforms T, phi
 * and ln ps where a pressure-level variable needs them, and the pressure-level kernel runs on the group's stream between the
 * transforms and the accumulation.  spd_model_stats_read / _ensemble give [count][n][48][96] / [n][48][96] for them. */
int spd_model_plev_configure(spd_model_handle m, const double *levels_pa, int n);
int spd_model_plev_levels(spd_model_handle m, double *out, int cap);
int spd_model_plev_compute(spd_model_handle m, const char *const *names, int n_names, int first, int count, int refresh,
                           void *stream);
int spd_model_plev_read(spd_model_handle m, const char *name, int first, int count, void *dst_device, size_t dst_bytes,
                        void *stream);
/* Derived fields, computed on the device from the sigma-level grid fields in export units, vorticity, divergence and grad ln ps.
 * Fourteen names, which the statistics, the tapes, the projection tape and spd_model_assim_configure take next to their own
 * (a sample then also transforms what a name needs, and the derived-field kernel runs on the group's stream behind the
 * pressure-level kernel).  With dhs[k], fsg[k] the model's layer thicknesses and full levels (k = 0 top ... 7), g and kappa the
 * library's, p0 = 1e5 Pa, q in kg/kg and ps in Pa, every sum over k sequential from k = 0:
 *   vor_grid, div_grid [8]  1/s       the state's vorticity and divergence through the export transform (no kernel)
 *   omega_grid [8]          Pa/s      the model's own discrete continuity equation on the exported time level: with px, py the
 *                                     components of grad ln ps as the step transforms them, D = div_grid,
 *                                       ubar = sum u[k] dhs[k], vbar, Dbar likewise; puv[k] = (u[k] - ubar) px + (v[k] - vbar) py
 *                                       sd[0] = 0, sd[k+1] = sd[k] - dhs[k] (puv[k] + D[k] - Dbar)    (sd[8] is not forced to 0)
 *                                       dlnps = -ubar px - vbar py - Dbar
 *                                       omega[k] = ps (fsg[k] (dlnps + u[k] px + v[k] py) + (sd[k] + sd[k+1]) / 2)
 *   rh_grid [8]             1         (1000 q) / qsat(T, fsg[k] ps / p0), the model's saturation formula (g/kg); not clipped
 *   theta_grid [8]          K         T (p0 / (fsg[k] ps))^kappa
 *   tcwv                    kg/m^2    (ps / g) sum q[k] dhs[k]
 *   ivt_u, ivt_v            kg/(m s)  (ps / g) sum q[k] u[k] dhs[k], and with v
 *   ke_col                  J/m^2     (ps / g) sum (u[k]^2 + v[k]^2) / 2 dhs[k]
 *   omega_plev, vor_plev, div_plev, rh_plev, theta_plev [n]   the sigma-level field at the target levels of
 *                                     spd_model_plev_configure: linear in ln p inside the full levels with the layer search and
 *                                     weight of the pressure-level fields above; the value of level 0 above the top full level
 *                                     and of level 7 below the lowest (no extrapolation); points under the ground are NOT masked.
 * They are derived fields, not state: spd_model_get / _set, restarts and spd_model_copy_member do not know them.
 *   _compute    members [first, first + count).  SPD_E_ARG, in this order: an unknown name, a name twice, a null model or a bad
 *               member range, a pressure-level name without configured levels.  With refresh = 1 first spd_model_spectral2grid
 *               of those members where a name reads u_grid ... ps_grid; with refresh = 0 the grid arrays are taken as they are.
 *               Vorticity, divergence and grad ln ps are always transformed from the spectral state (time level 1) into arrays
 *               of this call's own, made at first use.  Then one launch of the kernel per family ({omega_grid, omega_plev}; the
 *               rest) into the result arrays, which are allocated the first time a name is asked for.  n_names = 0: every name
 *               (the pressure-level ones only where target levels are configured).  The spectral state is not touched.
 *   _read       a computed result as fp64 into dst_device[count][levels][48][96] ([count][48][96] for the column integrals),
 *               device to device, stream-ordered. */
int spd_model_derive_compute(spd_model_handle m, const char *const *names, int n_names, int first, int count, int refresh,
                             void *stream);
int spd_model_derive_read(spd_model_handle m, const char *name, int first, int count, void *dst_device, size_t dst_bytes,
                          void *stream);
/* The tape: time series of fields recorded on the device inside spd_model_step / spd_model_step_checked_begin calls of any length.
 * A ring buffer in device memory, per model, holds the last `capacity` samples of the chosen variables for every member; one
 * sample is taken after every step that leaves the model's absolute step counter at a multiple of `every` (the statistics' rule),
 * by each member group on its own stream behind its last launch of that step, so an output every few steps no longer ends the
 * call.  Variables: the fourteen names of the statistics (the six pressure-level ones after spd_model_plev_configure), in export
 * units.  A sample of u_grid ... ps_grid holds what spd_model_spectral2grid would leave in the grid arrays if the call ended at
 * that step; of precnv / precls what the column physics stored at that step; of a pressure-level name what spd_model_plev_compute
 * would give there.  Storage: SPD_TAPE_F64, those values; SPD_TAPE_F32, each rounded to the nearest float (half the memory: what
 * the export writes).  Recording changes nothing of the run, and statistics and tape are independent: each has its own `every`,
 * and on a step both sample each runs its own transforms.
 *   _configure  allocates the ring (capacity x members x planes x 4608 elements, one hipMalloc of its own; synchronises the
 *               device) and empties it; n_names = 0 switches the tape off and frees it.  SPD_E_ARG for an unknown or repeated name,
 *               every < 1, capacity < 1, an unknown dtype, a pressure-level name before spd_model_plev_configure, or while a
 *               checked call is in flight.  SPD_E_DEVICE with the number of bytes asked for when the allocation fails: the tape is
 *               then off and the model as usable as before.  spd_model_plev_configure is refused while the tape holds a
 *               pressure-level name.
 *   _reset      empties the tape (host only, no device work).  spd_model_init does the same.
 *   _info       taken: samples since the last reset; held = min(taken, capacity); any pointer may be NULL.
 *   _times      rows[held][6] for the held samples, oldest first: the absolute step counter after the sampled step, then year,
 *               month, day, hour, minute of the sampled state (host memory; kept on the host when the sample is issued).  Returns
 *               the number of rows written (at most max_rows).
 *   _read       members [first, first + count) and samples [t0, t0 + nt) of the held ones, oldest first, of one variable into
 *               dst_device[count][nt][levels][48][96] ([count][nt][48][96] for ps_grid, precnv, precls, mslp) in the tape's dtype,
 *               stream-ordered; dst_device must be 16-byte aligned.  SPD_E_SIZE when dst_bytes is too small.
 * Reads fail (SPD_E_ARG, with the reason) while a checked call is in flight and after a checked call that reported a failed range
 * check (the message names the member and the step): the tape stays invalid until _reset or spd_model_init.  Samples issued by
 * unchecked calls on a stream are read behind them on the same stream.  spd_model_copy_member does not carry the tape, and the
 * outer boundary (spd_parallel_step*) does not keep it across the models it merges and splits. */
#define SPD_TAPE_F32 0
#define SPD_TAPE_F64 1
int spd_model_tape_configure(spd_model_handle m, const char *const *names, int n_names, int every, int capacity, int dtype);
int spd_model_tape_reset(spd_model_handle m);
int spd_model_tape_info(spd_model_handle m, long long *taken, int *held, int *capacity, int *every, int *dtype);
int spd_model_tape_times(spd_model_handle m, int32_t *rows, int max_rows);
int spd_model_tape_read(spd_model_handle m, const char *name, int first, int count, int t0, int nt, void *dst_device, size_t dst_bytes,
                        void *stream);
/* The ensemble tape: time series of the ensemble mean and spread, recorded on the device inside spd_model_step /
 * spd_model_step_checked_begin calls of any length.  A third ring in device memory, per model, holds for each of the last `capacity`
 * samples and each chosen variable the mean over ALL members of the model and the sum of squared deviations from that mean (M2), per
 * grid point, fp64 -- two planes per sample where the tape holds one per member.  Variables: the fourteen names of the statistics
 * (the six pressure-level ones after spd_model_plev_configure), in export units.  Sampling rule: the tape's, with the ensemble tape's
 * own `every`; each member group takes the sample on its own stream behind the spectra's.  The value of member j that enters sample
 * n is exactly what an fp64 tape would hold for member j at that sample; the reduction (Welford's update over the members of a
 * launch, in member order) is the only new arithmetic.  Recording changes nothing of the run; statistics, tape, spectra and ensemble
 * tape are independent (own `every`, slab and tables), and with the ensemble tape off no launch of a step changes.
 * Members reach a sample in pieces -- member groups on up to 4 streams, rounds of block_members one after the other on them -- so a
 * slot holds one partial (mean, M2) per group stream, written from that stream only (no atomics, no waits between streams), and a
 * read merges the partials in the fixed order of the groups with Chan's formula.  For a given launch plan (members, member groups,
 * block_members, the lengths of the calls) the result is repeatable bit for bit; between plans mean and M2 differ at round-off
 * level.  Memory: capacity x 4 x planes x 4608 x 16 bytes, whatever the number of members.
 *   _configure  allocates the ring (one hipMalloc of its own with slab and tables; synchronises the device) and empties it;
 *               n_names = 0 switches the ensemble tape off and frees it.  SPD_E_ARG, checked in this order before a model or a device
 *               is needed: an unknown name, a name given twice, every < 1, capacity < 1, a null model; then a pressure-level name
 *               before spd_model_plev_configure, or a checked call in flight.  SPD_E_DEVICE with the number of bytes asked for when
 *               the allocation fails: the ensemble tape is then off and the model as usable as before.  spd_model_plev_configure is
 *               refused while the ensemble tape holds a pressure-level name.
 *   _reset      empties the ring (host only, no device work).  spd_model_init does the same.
 *   _info       taken: samples since the last reset; held = min(taken, capacity); members: what a sample reduces over; any pointer
 *               may be NULL.
 *   _times      rows[held][6] for the held samples, oldest first: the absolute step counter after the sampled step, then year,
 *               month, day, hour, minute of the sampled state (host memory).  Returns the number of rows written (<= max_rows).
 *   _read       samples [t0, t0 + nt) of the held ones, oldest first, of one variable into dst_device[nt][levels][48][96] doubles
 *               ([nt][48][96] for ps_grid, precnv, precls, mslp), stream-ordered; dst_device must be 16-byte aligned.  kind:
 *               SPD_ENS_MEAN, SPD_ENS_M2, or SPD_ENS_STD, the unbiased standard deviation sqrt(M2 / (members - 1)) (one member:
 *               NaN, as spd_model_stats_ensemble).  SPD_E_SIZE when dst_bytes is too small.  (members, mean, M2) of several
 *               models combine into the moments of all their members by the same formula (pyspeedy_amd.ensemble.merge_moments).
 * Reads fail (SPD_E_ARG, with the reason) while a checked call is in flight and after a checked call that reported a failed range
 * check (the message names the member and the step): the ring stays invalid until _reset or spd_model_init.
 * spd_model_copy_member does not carry the ring, and the outer boundary (spd_parallel_step*) does not keep it across the models
 * it merges and splits. */
#define SPD_ENS_MEAN 0
#define SPD_ENS_STD 1
#define SPD_ENS_M2 2
int spd_model_enstape_configure(spd_model_handle m, const char *const *names, int n_names, int every, int capacity);
int spd_model_enstape_reset(spd_model_handle m);
int spd_model_enstape_info(spd_model_handle m, long long *taken, int *held, int *capacity, int *every, int *members);
int spd_model_enstape_times(spd_model_handle m, int32_t *rows, int max_rows);
int spd_model_enstape_read(spd_model_handle m, const char *name, int kind, int t0, int nt, void *dst_device, size_t dst_bytes,
                           void *stream);
/* The accumulation tape: window sums, means, minima and maxima of the column physics' 2-D outputs, accumulated on the device behind
 * EVERY step of spd_model_step / spd_model_step_checked_begin calls of any length.  The other recorders sample the state as it
 * stands on every n-th step; this one keeps what fell or flowed in between: the precipitation of a day, the mean outgoing longwave
 * of a month, the strongest convective rain of a day.  An entry is a pair (name, op).  Names, one plane each: precnv, precls, cbmf,
 * olr, tsr, ssr, ssrd, slr, slrd; three planes each (land, sea, weighted by the land fraction, the registry's order): ustr, vstr,
 * shf, evap, slru.  hfluxn and qcloud_equiv are refused by name: not every plane of them is stored on every step.  Ops: SPD_ACC_SUM,
 * SPD_ACC_MEAN, SPD_ACC_MIN, SPD_ACC_MAX.  Values are in the registry's own unit (these names carry no export conversion).
 * A window closes after every step that leaves the model's absolute step counter at a multiple of `every` (the tape's rule) and
 * holds the values the column physics stored in each step since the previous close; the first window after _configure, _reset or
 * spd_model_init (or after the step counter was set by spd_model_mark_initialized / spd_model_set_control) starts at the model's
 * current step and may be shorter than `every`; its number of steps n is kept beside the slot.  Windows run across call boundaries:
 * the accumulators are device memory.  The arithmetic is fixed, so the result does not depend on the launch plan (members, member
 * groups, block_members, the lengths of the calls): sum in fp64, the values added in step order starting from the first value
 * itself; mean, that sum divided by n (one IEEE division at the close); min / max, acc = x < acc ? x : acc and acc = x > acc ? x :
 * acc starting from the first value; sources stored as fp32 (physics_storage32) are widened to fp64 first.  Window k (from 1 since
 * the last reset) lies in ring slot (k - 1) % capacity; the ring holds, per entry, [slot][members][planes][4608] elements,
 * SPD_TAPE_F64 (the fp64 results) or SPD_TAPE_F32 (each rounded to the nearest float).  While the recorder is on every step stores
 * its diagnostics-only outputs (as the option diag_every_step does), which changes no state; nothing else of a step changes, and
 * with the recorder off no launch of a step changes.  It is independent of statistics, tape, spectra and ensemble tape.
 *   _configure  allocates ring, accumulators (only those an entry needs) and tables in one hipMalloc of its own (synchronises the
 *               device) and empties the ring; n_entries = 0 switches the recorder off and frees it.  SPD_E_ARG, checked in this order
 *               before a model or a device is needed: an unknown (or refused) name, an unknown op, the same (name, op) twice,
 *               every < 1, capacity < 1, an unknown dtype, a null model; then a checked call in flight.  SPD_E_DEVICE with the
 *               number of bytes asked for when the allocation fails: the recorder is then off and the model as usable as before.
 *   _reset      empties the ring and starts a new window at the model's current step (host only, no device work).
 *               spd_model_init does the same.
 *   _info       taken: windows closed since the last reset; held = min(taken, capacity); any pointer may be NULL.
 *   _times      rows[held][7] for the held windows, oldest first: the absolute step counter after the window's last step, then
 *               year, month, day, hour, minute of that state, then n, the number of steps in the window (host memory).  Returns the
 *               number of rows written (at most max_rows).
 *   _read       members [first, first + count) and windows [t0, t0 + nt) of the held ones, oldest first, of one entry into
 *               dst_device[count][nt][planes][48][96] ([count][nt][48][96] for a one-plane name) in the ring's dtype, stream-ordered;
 *               dst_device must be 16-byte aligned.  SPD_E_SIZE when dst_bytes is too small.
 * Reads fail (SPD_E_ARG, with the reason) while a checked call is in flight and after a checked call that reported a failed range
 * check (the message names the member and the step): the series stays invalid until _reset or spd_model_init.
 * spd_model_copy_member does not carry the recorder, and the outer boundary (spd_parallel_step*) does not keep it across the
 * models it merges and splits. */
#define SPD_ACC_SUM 0
#define SPD_ACC_MEAN 1
#define SPD_ACC_MIN 2
#define SPD_ACC_MAX 3
int spd_model_acctape_configure(spd_model_handle m, const char *const *names, const int *ops, int n_entries, int every, int capacity,
                                int dtype);
int spd_model_acctape_reset(spd_model_handle m);
int spd_model_acctape_info(spd_model_handle m, long long *taken, int *held, int *capacity, int *every, int *dtype);
int spd_model_acctape_times(spd_model_handle m, int32_t *rows, int max_rows);
int spd_model_acctape_read(spd_model_handle m, const char *name, int op, int first, int count, int t0, int nt, void *dst_device,
                           size_t dst_bytes, void *stream);
/* The window tape: window sums, means, minima, maxima and threshold counts of the STATE's grid-space fields, accumulated on the
 * device inside spd_model_step / spd_model_step_checked_begin calls of any length: the monthly mean of z_plev at 500 hPa, the day's
 * lowest t_grid, the month's strongest wind, the samples of a month below 273.15 K.  A sixth recorder, independent of statistics,
 * tape, spectra, ensemble tape and accumulation tape (its own front end, slab, tables and allocation); with it off no launch of a
 * step changes, and recording changes nothing of the run.
 * An entry is (name, op[, threshold]).  Names: the fourteen of the tape (u_grid, v_grid, t_grid, q_grid, phi_grid, ps_grid, precnv,
 * precls, u_plev, v_plev, t_plev, q_plev, z_plev, mslp; the pressure-level ones after spd_model_plev_configure) and two of this
 * recorder only: wspd_grid (8 levels) and wspd_plev (the configured levels), sqrt(u * u + v * v) of u_grid, v_grid and of u_plev,
 * v_plev.  Ops: SPD_WIN_SUM, SPD_WIN_MEAN, SPD_WIN_MIN, SPD_WIN_MAX (the numbers of SPD_ACC_*), SPD_WIN_COUNT_ABOVE (samples with
 * x > threshold) and SPD_WIN_COUNT_BELOW (x < threshold); thresholds[k] is read for the two count ops only, must be finite, and is
 * in the entry's own unit.  The value sampled is exactly what an fp64 tape of the same name holds (export units); a wind speed is
 * formed from those fp64 values of u and v by four correctly rounded IEEE operations (two products, their sum, the square root; no
 * fused multiply-add).
 * Sampling: after every step that leaves the model's absolute step counter at a multiple of `sample_every` (the tape's rule).
 * Windows, one kind for the whole recorder: SPD_WINDOW_STEPS closes after a step that leaves the counter at a multiple of `every`;
 * SPD_WINDOW_DAY after a step whose resulting date is 00:00; SPD_WINDOW_MONTH after a step whose resulting date is 00:00 on day 1
 * (the model's own calendar); `every` is 0 for the two calendar kinds.  Closing and sampling are separate decisions: a closing step
 * that is not sampled closes what was accumulated, and a window without a sample closes with 0 samples: sum and counts 0, mean,
 * minimum and maximum quiet NaN.  The first window after _configure, _reset or spd_model_init (or after the step counter was set by
 * spd_model_mark_initialized / spd_model_set_control) starts at the model's current step and may be short; windows run across call
 * boundaries.  The arithmetic is fixed, so the result does not depend on the launch plan: sum in fp64 in sample order starting from
 * the first sample itself; mean, that sum divided by the number of samples (one IEEE division at the close); min / max, acc = x <
 * acc ? x : acc and acc = x > acc ? x : acc from the first sample; counts as fp64 integers.  Window k (from 1 since the last reset)
 * lies in ring slot (k - 1) % capacity; the ring holds, per entry, [slot][members][levels][4608] elements, SPD_TAPE_F64 (the fp64
 * results) or SPD_TAPE_F32 (each rounded to the nearest float).  On a sampled step the diagnostics-only outputs are stored when
 * precnv or precls is an entry (the tape's rule).
 *   _configure  allocates ring, accumulators (only those an entry needs), slab and tables in one hipMalloc of its own (synchronises
 *               the device) and empties the ring; n_entries = 0 switches the recorder off and frees it.  SPD_E_ARG, checked in this
 *               order before a model or a device is needed: a bad list; an unknown name; an unknown op; a count op without a finite
 *               threshold (thresholds may be NULL when no entry counts); the same (name, op) twice; an unknown window kind; `every`
 *               (at least 1 for SPD_WINDOW_STEPS, 0 otherwise); sample_every < 1; capacity < 1; an unknown dtype; a null model; then
 *               a pressure-level name (wspd_plev included) before spd_model_plev_configure, or a checked call in flight.
 *               SPD_E_DEVICE with the number of bytes asked for when the allocation fails: the recorder is then off and the model
 *               as usable as before.  spd_model_plev_configure is refused while the recorder holds a pressure-level name.
 *   _reset      empties the ring and starts a new window at the model's current step (host only, no device work).
 *               spd_model_init does the same.
 *   _info       taken: windows closed since the last reset; held = min(taken, capacity); any pointer may be NULL.
 *   _times      rows[held][8] for the held windows, oldest first: the absolute step counter after the window's last step, then
 *               year, month, day, hour, minute of that state, then the number of samples and the number of steps in the window
 *               (host memory).  Returns the number of rows written (at most max_rows).
 *   _read       members [first, first + count) and windows [t0, t0 + nt) of the held ones, oldest first, of one entry into
 *               dst_device[count][nt][levels][48][96] ([count][nt][48][96] for ps_grid, precnv, precls, mslp) in the ring's dtype,
 *               stream-ordered; dst_device must be 16-byte aligned.  SPD_E_SIZE when dst_bytes is too small.
 * Reads fail (SPD_E_ARG, with the reason) while a checked call is in flight and after a checked call that reported a failed range
 * check (the message names the member and the step): the series stays invalid until _reset or spd_model_init.
 * spd_model_copy_member does not carry the recorder, and the outer boundary (spd_parallel_step*) does not keep it across the
 * models it merges and splits.
 * spd_wintape_plan is the recorder's schedule, the same code the step loop takes its decisions from, for hosts that want to know
 * the windows ahead: from the date y-m-d h:min and the step counter step0, over nsteps steps of 40 minutes, it returns the number
 * of windows that close and fills rows[min(that number, max_rows)][8] as _times does (the first window starts at step0).  It needs
 * no model and no device; SPD_E_ARG for a bad date, step0 < 0, nsteps < 0, a bad destination, or the window kind, `every` and
 * sample_every that _configure refuses. */
#define SPD_WIN_SUM 0
#define SPD_WIN_MEAN 1
#define SPD_WIN_MIN 2
#define SPD_WIN_MAX 3
#define SPD_WIN_COUNT_ABOVE 4
#define SPD_WIN_COUNT_BELOW 5
#define SPD_WINDOW_STEPS 0
#define SPD_WINDOW_DAY 1
#define SPD_WINDOW_MONTH 2
int spd_model_wintape_configure(spd_model_handle m, const char *const *names, const int *ops, const double *thresholds, int n_entries,
                                int window, int every, int sample_every, int capacity, int dtype);
int spd_model_wintape_reset(spd_model_handle m);
int spd_model_wintape_info(spd_model_handle m, long long *taken, int *held, int *capacity, int *window, int *every, int *sample_every,
                           int *dtype);
int spd_model_wintape_times(spd_model_handle m, int32_t *rows, int max_rows);
int spd_model_wintape_read(spd_model_handle m, const char *name, int op, int first, int count, int t0, int nt, void *dst_device,
                           size_t dst_bytes, void *stream);
int spd_wintape_plan(int year, int month, int day, int hour, int minute, int step0, int nsteps, int window, int every,
                     int sample_every, int32_t *rows, int max_rows);
/* The projection tape: scalar time series taken from grid-space fields -- box, band and global means, differences of boxes,
 * station values, any fixed linear functional of one plane -- formed on the device behind the sampled steps of spd_model_step /
 * spd_model_step_checked_begin calls of any length and kept in a ring in device memory.  Off unless configured; a model that never
 * configures it issues the launches it always issued.
 * Definition.  P weight maps (patterns), 1 <= P <= 64, each fp64 [48][96] in the layout of one level of a tape sample (row j = 0
 * the southernmost Gaussian latitude, column i at 3.75 i degrees east), uploaded once and shared by all members; every weight must
 * be finite.  E entries (name, level, pattern), 1 <= E <= 1024: name one of the tape's fourteen catalogue names, level from 0 up
 * to the name's level count (8 for the sigma fields, 1 for ps_grid, precnv, precls, mslp, the configured count for *_plev, which
 * need spd_model_plev_configure first), pattern an index into the maps.  x[p], p = 96 j + i, is exactly what an fp64 tape of that
 * name holds at that level after the sampled step, in export units (precnv / precls widened from float first under
 * physics_storage32; a sampled step stores the diagnostics-only outputs when either is an entry).  The result of an entry is one
 * double per member and sample, summed in a fixed order with every product and every sum rounded on its own (no contraction):
 *   lane t of 256:  s_t = w[t] x[t];  for r = 1 ... 17 in that order  s_t = s_t + w[t + 256 r] x[t + 256 r]
 *   tree[t] = s_t;  for half = 128, 64, ..., 1:  tree[t] = tree[t] + tree[t + half] for t < half;  result = tree[0]
 * All 4608 = 18 x 256 terms take part; a zero weight is not skipped.  The result does not depend on the launch plan (member
 * groups, rounds, checked or plain calls), and a numpy restatement of the order reproduces it bit for bit.
 * Sampling is the tape's: after every step that leaves the absolute step counter at a multiple of `every`, with the recorder's own
 * slab and tables, behind the other recorders' launches of that step on each member group's stream.  Sample n (from 1 since the
 * last reset) lies in slot (n - 1) % capacity of the ring [slot][M][E] doubles.
 *   _configure  weights[n_patterns][48][96] (host memory), names / levels / patterns[n_entries]; allocates (one hipMalloc of the
 *               recorder's own, synchronises the device) and empties the ring; n_entries = 0 switches the recorder off and frees
 *               it (the other arguments are then not looked at).  SPD_E_ARG, checked in this order before a model or a device is
 *               needed: every < 1; capacity < 1; n_patterns outside 1 ... 64; n_entries outside 0 ... 1024; null weights; a null
 *               names, levels or patterns; a weight that is not finite (the message names pattern and point); an unknown name
 *               (with the catalogue's list); per entry a level below 0 or, for a name of fixed level count, beyond it, then a
 *               pattern index outside the maps; then a null model or a checked call in flight; then a pressure-level name (mslp included)
 *               before spd_model_plev_configure or with a level beyond the configured count.  SPD_E_DEVICE with the number of bytes asked
 *               for when the allocation fails: the recorder is then off and the model as usable as before.
 *               spd_model_plev_configure is refused while the recorder holds a pressure-level name.
 *   _reset      empties the ring (host only, no device work).  spd_model_init does the same.
 *   _info       taken: samples since the last reset; held = min(taken, capacity); any pointer may be NULL.
 *   _times      rows[held][6] for the held samples, oldest first: the absolute step counter after the sampled step, then year,
 *               month, day, hour, minute of that state (host memory).  Returns the number of rows written (at most max_rows).
 *   _read       members [first, first + count) and samples [t0, t0 + nt) of the held ones, oldest first, of every entry in the
 *               configured order into dst_device[count][nt][n_entries] doubles, stream-ordered; dst_device must be 8-byte aligned.
 *               SPD_E_SIZE when dst_bytes is too small.
 * Reads fail (SPD_E_ARG, with the reason) while a checked call is in flight and after a checked call that reported a failed range
 * check (the message names the member and the step): the series stays invalid until _reset or spd_model_init.
 * spd_model_copy_member does not carry the recorder, and the outer boundary (spd_parallel_step*) does not keep it across the
 * models it merges and splits. */
int spd_model_projtape_configure(spd_model_handle m, const double *weights, int n_patterns, const char *const *names, const int *levels,
                                 const int *patterns, int n_entries, int every, int capacity);
int spd_model_projtape_reset(spd_model_handle m);
int spd_model_projtape_info(spd_model_handle m, long long *taken, int *held, int *capacity, int *every, int *n_patterns, int *n_entries);
int spd_model_projtape_times(spd_model_handle m, int32_t *rows, int max_rows);
int spd_model_projtape_read(spd_model_handle m, int first, int count, int t0, int nt, void *dst_device, size_t dst_bytes, void *stream);
/* The track tape: the minimum or maximum of a plane of the state's grid-space fields over a region, where it lies and two sub-grid
 * offsets, per member, inside spd_model_step / spd_model_step_checked_begin calls of any length -- how deep the low is and where,
 * the track of a storm, the jet or rain maximum -- as 32 bytes per entry, member and sample instead of a taped plane and an argmin
 * on the host.  The operator is not linear: no weight map of the projection tape expresses it.  Off unless configured; a model
 * without it issues exactly the launches it issued before.
 * Configuration.  R regions, 1 <= R <= 64: the projection tape's weight maps (fp64 [48][96], finite, shared by all members); a point
 * belongs to a region where its weight is not zero (the device keeps one byte per point), and a region without a point is refused.
 * E entries (name, level, region, op, radius), 1 <= E <= 1024: name and level exactly as the projection tape takes them, region an
 * index into the maps, op SPD_TRACK_MIN or SPD_TRACK_MAX, radius 0 ... 24 grid points (0: the entry never follows).
 * Value.  x[p], p = 96 j + i, row 0 southernmost, is exactly what an fp64 tape of that name holds at that level after the sampled
 * step, in export units (precnv / precls widened from float first under physics_storage32; a sampled step stores the
 * diagnostics-only outputs when either is an entry).  For member m and entry e, with the follow-state last[m][e] = q:
 *   1. candidates: the points of the region whose value is not NaN; if radius > 0 and q >= 0, only those with |j - j_q| <= radius
 *      and a circular distance of i and i_q <= radius (rows end at 0 and 47, longitude wraps).  q lies in the region.
 *   2. winner: the candidate with the smallest (MIN) or largest (MAX) value, infinities as numbers; among equal values the smallest
 *      p.  Without a candidate (every region point NaN): value NaN, index -1, offsets 0.
 *   3. offsets from the winner's four neighbours in the plane, candidates or not, every operation rounded on its own:
 *      a = x[j][(i + 95) % 96], b = x[p], c = x[j][(i + 1) % 96];  den = (a - 2 b) + c;  num = 0.5 (a - c);  di = num / den where
 *      den is finite and not zero and the quotient is finite, else 0; then clamped to [-0.5, 0.5].  dj likewise from rows j - 1 and
 *      j + 1; dj = 0 on rows 0 and 47.
 *   4. the ring slot gets four doubles (value, p, di, dj), and last[m][e] = p (-1 when nothing was found).
 * The order (value, p) is total, so the result does not depend on the launch plan (member groups, rounds, checked or plain
 * calls), and a numpy restatement reproduces it bit for bit.  Sampling is the tape's: after every step that leaves the absolute
 * step counter at a multiple of `every`, with the recorder's own slab and tables, behind the projection tape's launch of that step on
 * each member group's stream.  Sample n (from 1 since the last reset) lies in slot (n - 1) % capacity of the ring [slot][M][E][4].
 * The follow-state is int32 [M][E] in device memory, -1 (follows nothing: the next sample looks at the whole region) after
 * _configure, _reset and spd_model_init.
 *   _configure  regions[n_regions][48][96] (host memory), names / levels / region_of / ops / radii[n_entries]; allocates (one hipMalloc
 *               of the recorder's own, synchronises the device) and empties the ring; n_entries = 0 switches the recorder off and
 *               frees it (the other arguments are then not looked at).  SPD_E_ARG, checked in this order before a model or a device
 *               is needed: every < 1; capacity < 1; n_regions outside 1 ... 64; n_entries outside 0 ... 1024; null regions; a null
 *               list; a weight that is not finite (the message names pattern and point); a region without a point; an unknown name
 *               (with the catalogue's list); per entry a level below 0 or, for a name of fixed level count, beyond it, then a region
 *               index outside the maps ("pattern ..."), then an op that is neither constant, then a radius outside 0 ... 24; then a null
 *               model or a checked call in flight; then a pressure-level name (mslp included) before spd_model_plev_configure or with
 *               a level beyond the configured count.  SPD_E_DEVICE with the number of bytes asked for when the allocation fails: the
 *               recorder is then off and the model as usable as before.  spd_model_plev_configure is refused while the recorder
 *               holds a pressure-level name.
 *   _reset      empties the ring and sets the follow-state to -1 (synchronises the device).  spd_model_init does the same.
 *   _info       taken: samples since the last reset; held = min(taken, capacity); any pointer may be NULL.
 *   _times      rows[held][6] for the held samples, oldest first, as the projection tape's.  Returns the number of rows written.
 *   _read       members [first, first + count) and samples [t0, t0 + nt) of the held ones, oldest first, of every entry in the
 *               configured order into dst_device[count][nt][n_entries][4] doubles, stream-ordered; dst_device must be 8-byte
 *               aligned.  SPD_E_SIZE when dst_bytes is too small.  Fails like the projection tape's while a checked call is in
 *               flight and after one that reported a failed range check, until _reset or spd_model_init.
 *   _positions  the follow-state of members [first, first + count) into dst[count][n_entries] (host memory, room for `max` values;
 *               SPD_E_SIZE when that is too few); synchronises the device; returns the number of values written.
 *   _seed       src[count][n_entries] (host memory) becomes the follow-state of those members: -1 or 0 ... 4607, a point of the
 *               entry's region (SPD_E_ARG otherwise, nothing is written); synchronises the device.  Seeding is how a caller picks
 *               WHICH low an entry with radius > 0 follows.
 *   spd_track_point_host  steps 1 ... 3 for one plane as the device runs them, compiled for the host: plane[4608], mask[4608] bytes
 *               (non-zero: in the region), prev -1 or 0 ... 4607, radius 0 ... 24 -> out4 = value, p, di, dj.
 * spd_model_copy_member does not carry the recorder, and the outer boundary (spd_parallel_step*) does not keep it across the
 * models it merges and splits. */
#define SPD_TRACK_MIN 0
#define SPD_TRACK_MAX 1
int spd_model_tracktape_configure(spd_model_handle m, const double *regions, int n_regions, const char *const *names, const int *levels,
                                  const int *region_of, const int *ops, const int *radii, int n_entries, int every, int capacity);
int spd_model_tracktape_reset(spd_model_handle m);
int spd_model_tracktape_info(spd_model_handle m, long long *taken, int *held, int *capacity, int *every, int *n_regions, int *n_entries);
int spd_model_tracktape_times(spd_model_handle m, int32_t *rows, int max_rows);
int spd_model_tracktape_read(spd_model_handle m, int first, int count, int t0, int nt, void *dst_device, size_t dst_bytes, void *stream);
int spd_model_tracktape_positions(spd_model_handle m, int first, int count, int32_t *dst, int max);
int spd_model_tracktape_seed(spd_model_handle m, int first, int count, const int32_t *src);
int spd_track_point_host(const double *plane, const unsigned char *mask, int prev, int radius, int op, double *out4);
/* The filter tape: window means, covariances and last values of TIME-FILTERED grid-space fields, formed on the device inside
 * spd_model_step / spd_model_step_checked_begin calls of any length: the variance of the 2-6-day band-passed z_plev at 500 hPa (the
 * storm track), the transient eddy fluxes v'T' and u'v' of band-passed winds and temperature, the variance of a 10-day low-passed
 * field.  A recursive filter keeps two planes of state per second-order section, not a window of samples.  An eighth sampled
 * recorder, independent of the others (its own front end, slab, tables and allocation); it joins no member groups and writes nothing
 * into the model; off unless configured, and with it off no launch of a step changes.
 * Filters.  1 ... 8 filters, each a cascade of 1 ... 4 second-order sections.  A section is five fp64 numbers b0, b1, b2, a1, a2
 * (a0 = 1): sections[sum of n_sections][5], filter after filter; n_sections[n_filters].  A section is refused unless all five are
 * finite and it is stable: |a2| < 1 and |a1| < 1 + a2.  The library forms each section's zero-frequency gain once on the host,
 * every operation rounded on its own: g = ((b0 + b1) + b2) / ((1 + a1) + a2).
 * Filtered planes.  A filtered plane is one (name, level, filter) among the entries; each distinct combination is filtered once, at
 * most 32 of them.  Names: the fourteen of the tape and the fourteen derived names (the pressure-level ones after
 * spd_model_plev_configure); levels are 0-based levels of the name, by the projection tape's rules.  The value x fed in is exactly
 * what an fp64 tape of that name holds (export units; precnv / precls widened from their stored precision).
 * The filter step, per filtered plane and point, for filter sample k; k counts from 1 since _configure, _reset, spd_model_init or a
 * step counter set by spd_model_mark_initialized / spd_model_set_control.  The sections run in order, each section's y the next
 * section's x; every operation below is one correctly rounded IEEE operation, nothing is fused.
 *   k = 1, the steady state of a constant input, so that a field with a large mean does not ring:
 *       y = g x;  s1 = y - b0 x;  s2 = b2 x - a2 y
 *   k > 1, transposed direct form II, both state updates from the state before this sample:
 *       y = b0 x + s1;  s1 <- (b1 x - a1 y) + s2;  s2 <- b2 x - a2 y
 * Spin-up.  Samples with k <= spinup update the filters and are counted in no window.
 * Entries.  1 ... 64 entries (name_a, level_a, filter, op[, name_b, level_b]); names_b may be NULL, and names_b[k] NULL or "" means
 * that entry k names no second field (levels_b[k] is then not read).
 *   SPD_FIL_MEAN  value y_a; the window's result is the sum of the counted values in sample order, starting from the first counted
 *                 value itself, divided once by their number n at the close
 *   SPD_FIL_COV   value y_a * y_b (one multiplication), both through the entry's filter; without a second field b = a, a variance;
 *                 summed and divided as SPD_FIL_MEAN.  It is a second moment about ZERO: for a filter that passes the mean (a
 *                 low-pass) the caller subtracts the product of the two SPD_FIL_MEAN entries.
 *   SPD_FIL_LAST  y_a of the window's last counted sample; with a window equal to the sampling interval the recorder is a tape of
 *                 the filtered field
 * A window without a counted sample closes as quiet NaN under all three ops.  Window number w (from 1 since the last reset) lies in
 * ring slot (w - 1) % capacity; the ring holds, per entry, [slot][members][4608] elements, SPD_TAPE_F64 (the fp64 results) or
 * SPD_TAPE_F32 (each rounded to the nearest float).
 * Sampling and windows are the window tape's, from the same code: a sample after every step that leaves the absolute step counter at
 * a multiple of sample_every; SPD_WINDOW_STEPS / _DAY / _MONTH with `every` as spd_model_wintape_configure takes it; the first window
 * starts at the model's current step; spd_wintape_plan tells a host which windows a run closes (its column 6 counts all samples, the
 * recorder's the counted ones).  On a sampled step the diagnostics-only outputs are stored when precnv or precls is a name.
 *   _configure  allocates ring, filter state, accumulators, slab and tables in one hipMalloc of its own (synchronises the device) and
 *               empties the ring.  SPD_E_ARG, checked in this order before a model or a device is needed (spd_filtape_check runs
 *               exactly these checks and nothing else): n_filters outside 1 ... 8 or a null list of filters; a filter with fewer
 *               than 1 or more than 4 sections; per section, in order, a coefficient that is not finite, then a section that is not
 *               stable; n_entries outside 1 ... 64 or a null list of entries; an unknown name (a's, then b's); then per entry
 *               level_a, level_b, the filter index, the op, a second field on SPD_FIL_MEAN / SPD_FIL_LAST; more than 32 distinct
 *               filtered planes; spinup < 0; the window kind, `every` and sample_every as the window tape refuses them;
 *               capacity < 1; an unknown dtype.  Then a null model; a checked call in flight; a pressure-level name before
 *               spd_model_plev_configure or a level beyond the configured ones.  SPD_E_DEVICE with the number of bytes asked for
 *               when the allocation fails: the recorder is then off and the model as usable as before.
 *               spd_model_plev_configure is refused while an entry names a pressure-level plane.
 *   _off        switches the recorder off and frees it (synchronises the device).
 *   _reset      empties the ring, starts a new window at the model's current step and restarts the filters: the next sample is
 *               filter sample 1 (host only, no device work).  spd_model_init does the same.
 *   _info       taken: windows closed since the last reset; held = min(taken, capacity); n_planes: distinct filtered planes;
 *               filter_samples: k of the last sample; any pointer may be NULL.
 *   _times      rows[held][8] for the held windows, oldest first: the absolute step counter after the window's last step, then
 *               year, month, day, hour, minute of that state, then the number of counted samples and the number of steps in the
 *               window (host memory).  Returns the number of rows written (at most max_rows).
 *   _read       members [first, first + count) and windows [t0, t0 + nt) of the held ones, oldest first, of entry `entry` (0-based,
 *               the caller's order) into dst_device[count][nt][48][96] in the ring's dtype, stream-ordered; dst_device must be
 *               16-byte aligned.  SPD_E_SIZE when dst_bytes is too small.
 *   spd_filtape_filter_host  the filter step as the device runs it, compiled for the host, over a scalar series from filter sample 1
 *               on: sections[n_sections][5], x[n] -> y[n].  SPD_E_ARG for n_sections outside 1 ... 4, a null argument, a
 *               coefficient that is not finite, a section that is not stable, n < 0.
 * Reads fail (SPD_E_ARG, with the reason) while a checked call is in flight and after a checked call that reported a failed range
 * check (the message names the member and the step): the series stays invalid until _reset or spd_model_init.
 * spd_model_copy_member does not carry the recorder, and the outer boundary (spd_parallel_step*) does not keep it across the
 * models it merges and splits. */
#define SPD_FIL_MEAN 0
#define SPD_FIL_COV 1
#define SPD_FIL_LAST 2
int spd_model_filtape_configure(spd_model_handle m, const double *sections, const int *n_sections, int n_filters, const char *const *names_a,
                                const int *levels_a, const int *filters, const int *ops, const char *const *names_b, const int *levels_b,
                                int n_entries, int window, int every, int sample_every, int spinup, int capacity, int dtype);
int spd_model_filtape_off(spd_model_handle m);
int spd_model_filtape_reset(spd_model_handle m);
int spd_model_filtape_info(spd_model_handle m, long long *taken, int *held, int *capacity, int *window, int *every, int *sample_every,
                           int *spinup, int *dtype, int *n_filters, int *n_planes, int *n_entries, long long *filter_samples);
int spd_model_filtape_times(spd_model_handle m, int32_t *rows, int max_rows);
int spd_model_filtape_read(spd_model_handle m, int entry, int first, int count, int t0, int nt, void *dst_device, size_t dst_bytes,
                           void *stream);
int spd_filtape_check(const double *sections, const int *n_sections, int n_filters, const char *const *names_a, const int *levels_a,
                      const int *filters, const int *ops, const char *const *names_b, const int *levels_b, int n_entries, int window,
                      int every, int sample_every, int spinup, int capacity, int dtype);
int spd_filtape_filter_host(const double *sections, int n_sections, const double *x, int n, double *y);
/* Nudging: operator-split Newtonian relaxation of the spectral state toward target fields, on the device inside spd_model_step /
 * spd_model_step_checked_begin calls of any length (in-loop mode) or once on the state as it stands (_apply): replay experiments,
 * spectral nudging of the large scales, the cheapest form of data assimilation.  The only thing in the device loop that WRITES the
 * state; off unless configured, and a model that never configures it issues the launches it always issued.
 * Definition.  After a model step that leaves the absolute step counter at n, for every nudged variable X of vor, div, t, tr, ps,
 * every level k, BOTH time levels, every coefficient (m, nn) with total wavenumber l = m + nn <= 31 and every member whose mask
 * entry is 1:
 *     T  = T0 + a * (T1 - T0)          real and imaginary part separately
 *     X' = X + g[X][k][l] * (T - X)
 * Every operation is an IEEE fp64 operation rounded on its own (no fused multiply-add), so that a host restatement -- numpy's
 * x + g * ((t0 + a * (t1 - t0)) - x) on the real and imaginary parts -- gives the same bits.  Both time levels move alike, so the
 * leapfrog's computational mode is not excited.  Coefficients with m + nn >= 32 are neither loaded nor stored.
 * Targets are `capacity` slots of spectral fields shared by all members, complex128 in the registry's layout without the
 * time-level axis: (31, 32, 8) in Fortran order for vor, div, t, tr and (31, 32) for ps, in the state's stored units.  The first
 * in_use slots carry strictly ascending absolute step stamps (_set_times).  T0 and T1 are the slots whose stamps s0 < n < s1
 * bracket n and a = (n - s0) / (s1 - s0), computed on the host in fp64 and handed to the launch by value.  Before the first stamp
 * T is the first slot, at or after the last stamp the last slot, at a slot's own stamp that slot: T = T0 then, without the
 * interpolation line.  Gains are gains[n_names][8][32] fp64 in [0, 1], by name in the order given, level and total wavenumber
 * (ps reads the first of its eight rows); a plane whose 32 gains are all zero is not part of the launch, and a table that is zero
 * everywhere launches nothing at all.
 * In-loop mode: one launch per member group and step directly behind the group's step on its stream, in front of the range checks
 * of a checked call and of every recorder's sample, which therefore see the nudged state -- the state a host that nudged between
 * one-step calls would see, bit for bit, whatever the launch plan (groups, rounds, checked calls).  While in-loop nudging with a
 * non-zero gain is configured the spectral step does not compute the next step's geopotential ahead (spd_model_get_config reports
 * the fold as off): it would be that of the temperature before the nudge.  The quiet rim keeps working: nothing beyond m + nn = 31
 * is touched.  spd_model_step_dynamics is never nudged.
 *   _configure  n_names = 0 switches nudging off and frees it.  Otherwise allocates the slots (zero-filled), gain rows and the mask
 *               in one hipMalloc of its own (synchronises the device), with no slot in use and `applied` 0; member_mask is
 *               int32[members] of 0 / 1 or NULL for all members; in_loop = 0 keeps gains and targets for _apply only.  SPD_E_ARG,
 *               checked in this order before a model or a device is needed: a bad list (n_names > 5 too); an unknown name; a name
 *               twice; null gains; a gain that is not finite or outside [0, 1] (the message names variable, level and wavenumber);
 *               capacity < 1; in_loop neither 0 nor 1; a null model; then a mask entry other than 0 / 1, or a checked call in flight.
 *   _set_times  declares the first n <= capacity slots in use with the stamps steps[n] (host state; n = 0: none in use).
 *   _set_target copies one slot of one configured name from host memory (bytes must be 16 * 992 * levels; synchronises the device).
 *   _apply      the same kernel once for the members [first, first + count) on the state as it stands, with n the current step
 *               counter, stream-ordered; drops the look-ahead geopotential as spd_model_set does (phi itself is recomputed by the
 *               next step, not here).
 *   _info       names configured (0: off), capacity, slots in use, the mode, and `applied`: the steps nudged so far (in-loop steps
 *               and _apply calls that launched) since _configure; any pointer may be NULL.
 * _apply, and spd_model_step / spd_model_step_checked_begin in the in-loop mode, fail (SPD_E_ARG) while no slot is in use.
 * spd_model_copy_member does not carry the configuration, and the outer boundary (spd_parallel_step*) does not keep it across the
 * models it merges and splits. */
int spd_model_nudge_configure(spd_model_handle m, const char *const *names, int n_names, const double *gains, const int32_t *member_mask,
                              int capacity, int in_loop);
int spd_model_nudge_set_times(spd_model_handle m, const int32_t *steps, int n);
int spd_model_nudge_set_target(spd_model_handle m, int slot, const char *name, const void *host, size_t bytes);
int spd_model_nudge_apply(spd_model_handle m, int first, int count, void *stream);
int spd_model_nudge_info(spd_model_handle m, int *n_names, int *capacity, int *in_use, int *in_loop, long long *applied);
/* Breeding: the perturbation of a bred member against its control run is rescaled to a fixed amplitude, on the device inside
 * spd_model_step / spd_model_step_checked_begin calls of any length (in-loop mode) or once on the state as it stands (_apply): the
 * breeding cycle of bred vectors, for ensemble initialisation and error-growth studies.  Off unless configured, and a model that
 * never configures it issues the launches it always issued.
 * Definition.  control[M] (int32) names each member's control run, or -1 for a member that is not bred; a control must itself have
 * -1, control[i] != i, and the indices are in range.  For a bred member p with control c take D = X_p - X_c on time level 1 (the
 * level the spectra read), w_m = 1 for m = 0 and 2 otherwise, and sum over the 527 coefficients (m, nn) with m + nn <= 31:
 *     E(vor | div, k) = 1/4 sum elm2(m + nn) w_m |D|^2     the kinetic energy of the difference wind (the model's own elm2 table)
 *     E(t | tr | ps, k) = 1/2 sum w_m |D|^2                 the area mean square
 *     A = sqrt(sum over names and levels of weights[name][k] * E(name, k)),   s = target / A
 * weights[5][8] >= 0 by name in the order vor, div, t, tr, ps and level (ps reads entry 0 of its row; a plane of weight zero takes
 * no part).  sqrt and the division are the correctly rounded ones.  If A is zero or not finite, s = 1 and the member is left
 * alone.  The order of summation is fixed by the kernels (breed.hip: a lane's four coefficients, a tree over the 256 lanes, the 33
 * planes ascending) and depends on nothing else: A is the same bits whatever the member groups, the rounds, the call length or
 * the set of bred members, and within 34 782 * 2^-53 of the exact sum of its terms.  The rescale moves all five variables, all
 * levels, BOTH time levels, at the coefficients with m + nn <= 31 only:
 *     X_p' = X_c + s * (X_p - X_c)          real and imaginary part separately
 * every operation an IEEE fp64 operation rounded on its own (no fused multiply-add): given s, numpy's xc + s * (xp - xc) gives the
 * same bits.  Coefficients with m + nn >= 32 are neither loaded nor stored (the quiet rim stays valid); controls, members that are
 * not bred and every other registry variable are untouched -- the surface models' prognostic anomalies (land and sea temperatures)
 * among them.
 * In-loop mode: after the step that leaves the absolute step counter at n with n % every == 0 every bred member is rescaled
 * before step n + 1 starts.  A control may lie in another member group or round than its bred member, so such a call is issued in
 * segments that end at the rescale steps: the group streams join the caller's stream (no host synchronisation), the two breeding
 * launches go out there, the next segment forks again.  The range check of step n and every recorder's sample at step n see the
 * state the step left.  A multi-step call is bit for bit the host loop  step(k); _apply; step(k); ...  -- checked calls with all
 * their rows, `accepted` and codes included.  Nudging and breeding may be on together: the nudge follows every step, the rescale
 * comes behind it at the segment's end.  spd_model_step_dynamics is never bred.
 * Each rescale writes one slot of a ring of `capacity` events: fp64 amplitude[M], the A before the rescale (0.0 for a member that
 * is not bred), and factor[M], the s (1.0 for a member that is not bred); the step counter and date of an event are kept on the
 * host (_rows: 6 int32 per event, oldest first -- step, year, month, day, hour, minute; returns the number written).
 *   _configure  a null `control` switches breeding off and frees everything.  Otherwise one hipMalloc of its own (synchronises the
 *               device); the ring is empty and `applied` 0.  in_loop = 0 keeps the configuration for _apply / _compute only.  A
 *               configuration without a bred member launches nothing.  SPD_E_ARG, before anything is allocated: null weights; a
 *               weight that is negative or not finite; all weights zero; target not a finite number > 0; every < 1; capacity < 1;
 *               in_loop neither 0 nor 1; a null model; a checked call in flight; then, per member, a control out of range, a
 *               member that is its own control, a control that is itself bred.
 *   spd_breed_check  the same checks without a model, for `members` members (control may be NULL: only the rest is checked then;
 *               with a control its checks come first); the messages are those of _configure.
 *   _apply      rescale once on the state as it stands, stream-ordered; writes a ring slot; drops the look-ahead geopotential and
 *               the day's interpolated climatologies as spd_model_set does, and settles a deferred range check first.
 *   _compute    the amplitudes [M] (fp64, 0.0 for members that are not bred) of the state as it stands into device memory; writes no
 *               state and no ring.  It uses the configuration's scratch: order it against _apply and the steps by the stream.
 *   _read       what = 0: amplitude, 1: factor; the events [t0, t0 + nt) of the held ones, oldest first, as [nt][M] fp64.
 *   _reset      empties the ring (no device work).
 *   _info       bred members, every, capacity, events taken since _configure / _reset, the mode, and `applied`: the rescales
 *               launched since _configure; any pointer may be NULL; all zero without a configuration.
 * spd_model_copy_member does not carry the configuration, and the outer boundary (spd_parallel_step*) does not keep it. */
int spd_breed_check(const int32_t *control, int members, const double *weights, double target, int every, int capacity, int in_loop);
int spd_model_breed_configure(spd_model_handle m, const int32_t *control, const double *weights, double target, int every, int capacity,
                              int in_loop);
int spd_model_breed_apply(spd_model_handle m, void *stream);
int spd_model_breed_compute(spd_model_handle m, void *dst_device, size_t dst_bytes, void *stream);
int spd_model_breed_read(spd_model_handle m, int what, int t0, int nt, void *dst_device, size_t dst_bytes, void *stream);
int spd_model_breed_rows(spd_model_handle m, int32_t *rows, int max_rows);
int spd_model_breed_reset(spd_model_handle m);
int spd_model_breed_info(spd_model_handle m, int *bred, int *every, int *capacity, long long *taken, int *in_loop, long long *applied);
/* Orthonormalised breeding: the Gram-Schmidt cycle of the bred members that share a control, inside the same device loop -- the
 * perturbations stay orthonormal (backward Lyapunov vectors), the ring's growth rates are the leading local Lyapunov exponents,
 * and the Gram matrix is there to be read (bred-vector dimension).  Off unless switched on; plain breeding keeps its bits.
 * Definition.  A family is the set of bred members with one control c, in ascending member index p_1 < ... < p_r, r <= 64;
 * D_j = X_(p_j) - X_c.  Inner product, on time level 1, over the coefficients with m + n <= 31, with the planes, weights, w_m and
 * elm2 of the breeding configuration:
 *   B_P(i, j) = f_P sum_k [elm2(l)] w_m (Re D_i Re D_j + Im D_i Im D_j)      f = 1/4 for vor, div (with elm2), 1/2 for t, tr, ps
 *   G_ij      = sum_P weight_P B_P(i, j)                                      ascending plane order, planes of weight 0 skipped
 * A term is q = rn(rn(dx_i dx_j) + rn(dy_i dy_j)), times 2 if m != 0, times elm2 if kinetic; per (plane, pair) the terms are added
 * in the order of the plain amplitude's kernel (a lane's coefficients lane, + 256, + 512, + 768, then the tree 128 ... 1 over the
 * lanes), whatever the tiling, the family, the launch plan or the call length.  So B_P(j, j) is, bit for bit, the partial that
 * plain breeding computes, and sqrt(G_11) is _compute's amplitude of p_1.
 * Factor G = R^T R, R upper triangular, every operation rounded on its own:
 *   for j = 1 ... r:
 *       for i = 1 ... j-1:  acc = G_ij;  for k = 1 ... i-1: acc = acc - R_ki R_kj;   R_ij = acc / R_ii
 *       d = G_jj;  for k = 1 ... j-1: d = d - R_kj R_kj
 *       if not (d > 0 and d finite): the family BREAKS at j: members p_j ... p_r are left alone (not one bit loaded or stored,
 *                                    amplitude 0.0 and factor 1.0 in the ring); stop
 *       R_jj = sqrt(d)
 * Coefficients C = target R^-1 (upper triangular):
 *   C_jj = target / R_jj;   for i = j-1 ... 1:  acc = 0;  for k = i+1 ... j: acc = acc + R_ik C_kj;   C_ij = (-acc) / R_ii
 * Transform, on both time levels with the same C, real and imaginary parts separately, m + n <= 31 only, D of the members as
 * they stood:
 *   acc = C_1j D_1;  for i = 2 ... j: acc = acc + C_ij D_i;   X'_(p_j) = X_c + acc
 * A family of one member is plain breeding, bit for bit.  Ring: amplitude[p_j] = R_jj (the part of the grown perturbation that
 * is orthogonal to the earlier ones), factor[p_j] = target / R_jj.
 *   _orthogonalize  on = 1: allowed when breeding is configured and no checked call is in flight; builds the family and pair lists
 *               and allocates the Gram partials [pairs][33] and C [families][64][64] (one hipMalloc; synchronises the device).
 *               SPD_E_ARG with the control and the size for a family of more than 64 members.  From then on every rescale
 *               (in-loop and _apply) issues the Gram, factor and transform launches for the norm and rescale launches; schedule,
 *               ring slot, stamps and `applied` are as before.  on = 0 frees it; _configure retires it with the rest.
 *   _compute    keeps its meaning: A is the square root of the Gram matrix's diagonal, not R_jj.
 *   _gram       fp64 [M][M] into device memory: entry (a, b) is G of the two members if both are bred with the same control, else
 *               0.0; symmetric; writes neither state nor ring; stream-ordered with orthogonalisation on, and it synchronises with
 *               it off (its scratch lives for the call).
 *   spd_breed_family_check  without a model: the checks of a control list (the messages of _configure), then the size of the
 *               largest family, or -1 with _orthogonalize's message for a family of more than 64.
 *   spd_breed_factor_host  the factor routine of the device, compiled for the host: gram and coef row-major r x r (gram is read
 *               at i <= j), rdiag[r] = R's diagonal, *rank = the members transformed; rows and columns from the rank on are 0.0.
 *   _ortho_info on (0 or 1), the number of families and the size of the largest of the configuration; any pointer may be NULL. */
int spd_model_breed_orthogonalize(spd_model_handle m, int on);
int spd_model_breed_gram(spd_model_handle m, void *dst_device, size_t dst_bytes, void *stream);
int spd_breed_family_check(const int32_t *control, int members);
int spd_breed_factor_host(const double *gram, int r, double target, double *rdiag, double *coef, int *rank);
int spd_model_breed_ortho_info(spd_model_handle m, int *on, int *families, int *largest);
/* Assimilation: a serial ensemble square-root filter (EnSRF, Whitaker & Hamill 2002) with at most 64 scalar observations, taken
 * through projection-tape weight maps, and at most 64 members, computed and applied on the device at scheduled steps inside
 * spd_model_step / spd_model_step_checked_begin calls of any length (in-loop mode) or once on the state as it stands (_apply); and
 * the member-mixing transform on its own for a caller's matrix (_transform).  Off unless configured, and a model that never
 * configures it issues the launches it always issued.
 * Configuration.  P weight maps, 1 <= P <= 64, fp64 [48][96], finite: the projection tape's layout and rules.  E entries (name,
 * level, pattern), 1 <= E <= 64; name is one of the projection tape's names but precnv and precls (outputs of the column physics,
 * not functions of the state); the *_plev names and mslp need spd_model_plev_configure first.  mask[M] (int32, 0 or 1): the members
 * with mask 1 are a_0 < ... < a_(r-1), 2 <= r <= 64; a member with mask 0 (a nature run) is never loaded nor stored.  every >= 1;
 * capacity >= 1 slots of the diagnostics ring; inflation rho, finite and >= 1.
 * Observations.  A host table of n_rows rows: strictly ascending absolute step stamps steps[n_rows], values yo[n_rows][E] (NaN:
 * missing; an infinite value is refused) and error variances var[n_rows][E] (finite, > 0).  It may be replaced between calls.
 * Event.  In-loop, after the step that leaves the absolute step counter at n with n % every == 0: if a row is stamped exactly n
 * the analysis below runs before step n + 1 starts; if not, the event is skipped -- no launch, and `skipped` counts it.  _apply is
 * the same event once, refused if no row carries the current step.
 * 1 Observation-space ensemble.  Y[e][i] is the value of entry e for member a_i: exactly the projection tape's result for that
 *   entry (the same front end, export units, lane order and tree), by the projection tape's kernel into a one-slot ring.
 * 2 Weights, in fp64, every operation rounded on its own (no fused multiply-add), every sum sequential in ascending index and
 *   starting from its first term:
 *     a = (1 - rho) / r;   W[i][j] = a for i != j,   W[i][i] = a + rho                      (rho = 1: the exact identity)
 *     for e = 0 ... E-1:
 *       y_j = sum_i Y[e][i] W[i][j];   ybar = (sum_j y_j) / r;   d_j = y_j - ybar;   s = (sum_j d_j d_j) / (r - 1)
 *       the entry is UNUSED (W as it is) if yo[e] is NaN or s is not a finite number > 0; otherwise
 *       t = s + var[e];   alpha = 1 / (1 + sqrt(var[e] / t));   v = yo[e] - ybar;   q = (r - 1) t
 *       g_i = d_i / q;   c_j = v - alpha d_j;   u_k = sum_i W[k][i] g_i;   W[k][j] = W[k][j] + u_k c_j
 *   In exact arithmetic this is the EnSRF: the mean moves by the Kalman gain, the perturbations by alpha times it, and a later
 *   observation sees the updated ensemble (its prior is recomputed from Y and W, not carried along).
 * 3 Transform, for vor, div, t, tr, ps (33 planes), BOTH time levels, every coefficient with m + nn <= 31, real and imaginary part
 *   separately, X the members' states as they stood before the event:
 *     X'_(a_j) = (...((W[0][j] X_(a_0)) + W[1][j] X_(a_1)) + ...) + W[r-1][j] X_(a_(r-1))
 *   Coefficients with m + nn >= 32 are neither loaded nor stored (the quiet rim stays valid); members outside the mask and every
 *   other registry variable are untouched -- the surface models' prognostic anomalies among them.
 * 4 Ring: one slot per executed event, [E][4] fp64 = ybar, s, v, used (1.0 / 0.0); v is 0.0 for a missing observation.  The step
 *   counter and date of an event are kept on the host (_rows: 6 int32 per event, oldest first).  W [64][64] (zero beyond r) and
 *   Y [E][r] of the last event stay readable (_weights).
 * A call with in-loop assimilation is issued in segments that end at the multiples of `every`, as a call with in-loop breeding is;
 * it is bit for bit the host loop  step(k); _apply; step(k); ...  -- checked calls included.  In-loop assimilation and in-loop
 * breeding together are refused by whichever _configure comes second; nudging inside the segments is unaffected.  While
 * assimilation loops the geopotential look-ahead of small ensembles is off, as under in-loop nudging.
 *   _configure  one hipMalloc of its own (synchronises the device); the ring is empty, the observation table empty, `applied` 0.
 *               SPD_E_ARG, before anything is allocated, in this order: every < 1; capacity < 1; inflation not finite or < 1;
 *               in_loop neither 0 nor 1; n_patterns outside 1 ... 64; n_entries outside 1 ... 64; null weights; null lists; a
 *               weight that is not finite (pattern, point, row, column); per entry an unknown name, precnv / precls, a level or
 *               pattern out of range; a null mask; a null model; a checked call in flight; a mask entry that is not 0 or 1; r
 *               outside 2 ... 64; a pressure-level name without target levels; in-loop breeding configured.
 *   spd_assim_check  the same checks without a model, for `members` members (mask may be NULL: only the rest is checked then).
 *   _off        switches it off and frees everything.
 *   _set_observations  replaces the table (n_rows = 0 empties it).  SPD_E_ARG, in this order: n_rows < 0; n_entries outside
 *               1 ... 64; null arrays; stamps not strictly ascending (row named); a variance that is not a finite number > 0, an
 *               infinite observation (row and entry named); then a null model, a checked call in flight, no configuration,
 *               n_entries that is not the configuration's E.
 *   _apply      the event once on the state as it stands, stream-ordered; writes a ring slot; drops the look-ahead geopotential and
 *               the day's interpolated climatologies as spd_model_set does, and settles a deferred range check first.
 *   _compute    Y [E][r] (fp64) of the state as it stands into device memory; writes no state and no ring.  It uses the
 *               configuration's slab: order it against _apply and the steps by the stream.
 *   _transform  step 3 alone with the caller's finite matrix w[r][r] (row-major, host memory) for the distinct members
 *               members[r], 1 <= r <= 64, with or without an assimilation configured; the host waits for the stream once while
 *               its copies of w and members are taken, the launch itself is stream-ordered.
 *   _read       the events [t0, t0 + nt) of the held ones, oldest first, as [nt][E][4] fp64 into device memory; refused after a
 *               failed range check of a checked call until _reset or spd_model_init.
 *   _weights    W [64][64] and Y [E][r] of the last executed event into device memory (stream-ordered copies).
 *   _reset      empties the ring and `skipped` (no device work).
 *   _info       r, E, every, capacity, events taken and skipped since _configure / _reset, the mode, and `applied`: the events
 *               executed since _configure; any pointer may be NULL; all zero without a configuration.
 *   spd_assim_weights_host  step 2 as the device runs it, compiled for the host: y [E][r], yo[E], var[E] -> w_out [r][r] row-major
 *               and stats_out [E][4] as a ring slot.
 * spd_model_init empties the ring.  spd_model_copy_member does not carry the configuration, and the outer boundary
 * (spd_parallel_step*) does not keep it. */
int spd_assim_check(const double *weights, int n_patterns, const char *const *names, const int *levels, const int *patterns, int n_entries,
                    const int32_t *mask, int members, int every, int capacity, double inflation, int in_loop);
int spd_model_assim_configure(spd_model_handle m, const double *weights, int n_patterns, const char *const *names, const int *levels,
                              const int *patterns, int n_entries, const int32_t *mask, int every, int capacity, double inflation, int in_loop);
int spd_model_assim_off(spd_model_handle m);
int spd_model_assim_set_observations(spd_model_handle m, const int32_t *steps, int n_rows, const double *yo, const double *var, int n_entries);
int spd_model_assim_apply(spd_model_handle m, void *stream);
int spd_model_assim_compute(spd_model_handle m, void *dst_device, size_t dst_bytes, void *stream);
int spd_model_assim_transform(spd_model_handle m, const int32_t *members, int r, const double *w, void *stream);
int spd_model_assim_read(spd_model_handle m, int t0, int nt, void *dst_device, size_t dst_bytes, void *stream);
int spd_model_assim_weights(spd_model_handle m, void *w_device, size_t w_bytes, void *y_device, size_t y_bytes, void *stream);
int spd_model_assim_rows(spd_model_handle m, int32_t *rows, int max_rows);
int spd_model_assim_reset(spd_model_handle m);
int spd_model_assim_info(spd_model_handle m, int *r, int *n_entries, int *every, int *capacity, long long *taken, long long *skipped, int *in_loop,
                         long long *applied);
int spd_assim_weights_host(const double *y, int n_entries, int r, const double *yo, const double *var, double inflation, double *w_out,
                           double *stats_out);
/* The verification tape: bias, mean squared error, ensemble variance, CRPS and the rank histogram of a masked ensemble against a
 * truth member of the SAME model (typically a nature run that the assimilation's mask leaves alone), by variable, level and
 * region, recorded on the device at scheduled steps inside spd_model_step / spd_model_step_checked_begin calls of any length
 * (in-loop mode) or once on the state as it stands (_apply).  It writes nothing into the model.  Off unless configured, and a model
 * that never configures it issues the launches it always issued.
 * Configuration.  mask[M] (int32, 0 or 1): the members with mask 1 are the ensemble a_1 < ... < a_r, 2 <= r <= 64.  truth: a
 * member index with mask 0.  P weight maps, 1 <= P <= 64, fp64 [48][96], finite: the projection tape's layout and rules.  E
 * entries (name, level, pattern), 1 <= E <= 256; name is any name the projection tape accepts (precnv and precls included); the
 * *_plev names and mslp need spd_model_plev_configure first.  every >= 1; capacity >= 1 slots of the ring.
 * Value.  x_j[p] and y[p], p = 96 row + column, are what an fp64 tape of that name holds at that level for member a_j and for the
 * truth: the same front end (run over the member ranges that cover the mask and the truth), export units and stored precision of
 * precnv / precls.
 * Scores of a point, once per distinct (name, level), in fp64, every operation rounded on its own (no fused multiply-add):
 *     s = x_1;  s = s + x_j (j = 2 ... r);  mean = s / r;  e = mean - y;  se = e e
 *     a = (x_1 - mean)^2;  a = a + (x_j - mean)^2 (j = 2 ... r);  v = a / (r - 1)
 *     b = |x_1 - y|;  b = b + |x_j - y| (j = 2 ... r)
 *     c = 0;  c = c + |x_j - x_k| for j = 1 ... r - 1 (outer), k = j + 1 ... r (inner)
 *     crps = b / r - c / (r r);  rank = #{j : x_j < y};  tie = 1 if some x_j == y
 * An entry with the pattern w: bias, mse, variance, crps = the sums of w e, w se, w v, w crps over the 4608 points in exactly the
 * projection tape's order (lane sums over 18 passes, then the tree); and 66 int32 counts over the points with w != 0:
 * counts[k], k = 0 ... r, the points without a tie whose rank is k; counts[r + 1] the points with a tie; zero behind.
 * Ring.  One slot per event: [2 phases][E][4] fp64 and [2][E][66] int32.  Phase 0 is the state as the event finds it.  Phase 1 is
 * the state an in-loop analysis (spd_model_assim_*) left at the same step, front end and kernels run again; without one it reads
 * NaN / -1.  The step counter, the date and the flag `analysis` of an event are kept on the host (_rows: 7 int32, oldest first).
 * Schedule.  In-loop, after the step that leaves the absolute step counter at n with n % every == 0.  A call with in-loop
 * verification is issued in segments that end at the multiples of the `every` of each looping joined consumer (breeding or
 * assimilation, and verification); at such a step: the verification's phase 0 if due, the rescale or analysis if due, the
 * verification's phase 1 if an analysis was applied.  It is bit for bit the host loop  step(k); _apply; step(k); ...  -- checked
 * calls included --, and no state bit and no other recorder's ring differs from a run without it.
 *   _configure  one hipMalloc of its own (synchronises the device); the ring is empty, `applied` 0.  SPD_E_ARG, before anything is
 *               allocated, in this order: every < 1; capacity < 1; in_loop neither 0 nor 1; n_patterns outside 1 ... 64; n_entries
 *               outside 1 ... 256; null weights; null lists; a weight that is not finite (pattern, point, row, column); per entry
 *               an unknown name, a level or pattern out of range; a null mask; a null model; a checked call in flight; a mask
 *               entry that is not 0 or 1; r outside 2 ... 64; truth outside 0 ... M - 1; truth inside the mask; a pressure-level
 *               name without target levels.  SPD_E_DEVICE when the allocation fails: the tape is off, the model as usable as before.
 *   spd_verif_check  the same checks without a model, for `members` members (mask may be NULL: only the rest is checked then).
 *   _off        switches it off and frees everything.
 *   _reset      empties the ring (no device work).  spd_model_init does the same.
 *   _apply      one event (phase 0) on the state as it stands, stream-ordered; writes a ring slot and nothing else.
 *   _compute    the scores [E][4] fp64 and counts [E][66] int32 of the state as it stands into device memory; writes no ring.  It
 *               uses the configuration's slab and scratch: order it against _apply and the steps by the stream.
 *   _read       the events [t0, t0 + nt) of the held ones, oldest first, as [nt][2][E][4] fp64 (bias, mse, variance, crps) into
 *               device memory; _hist the same events as [nt][2][E][66] int32 (8-byte aligned).  Refused while a checked call is in
 *               flight and after a failed range check of a checked call until _reset or spd_model_init.
 *   _rows       rows[held][7] (host memory): step counter, year, month, day, hour, minute of the event's state, analysis (0 / 1).
 *   _info       r, truth, E, every, capacity, events taken since _configure / _reset, the mode, and `applied`: the events recorded
 *               since _configure; any pointer may be NULL; all zero and truth -1 without a configuration.
 *   spd_verif_host  one entry as the device forms it, compiled for the host: x [r][4608], y [4608], w [4608] -> out4 = bias, mse,
 *               variance, crps and hist66 as a ring slot's counts.
 * spd_model_plev_configure is refused while an entry is a pressure-level name.  spd_model_copy_member does not carry the
 * configuration, and the outer boundary (spd_parallel_step*) does not keep it. */
int spd_verif_check(const double *weights, int n_patterns, const char *const *names, const int *levels, const int *patterns, int n_entries,
                    const int32_t *mask, int members, int truth, int every, int capacity, int in_loop);
int spd_model_verif_configure(spd_model_handle m, const double *weights, int n_patterns, const char *const *names, const int *levels,
                              const int *patterns, int n_entries, const int32_t *mask, int truth, int every, int capacity, int in_loop);
int spd_model_verif_off(spd_model_handle m);
int spd_model_verif_reset(spd_model_handle m);
int spd_model_verif_apply(spd_model_handle m, void *stream);
int spd_model_verif_compute(spd_model_handle m, void *scores_device, size_t scores_bytes, void *hist_device, size_t hist_bytes, void *stream);
int spd_model_verif_read(spd_model_handle m, int t0, int nt, void *dst_device, size_t dst_bytes, void *stream);
int spd_model_verif_hist(spd_model_handle m, int t0, int nt, void *dst_device, size_t dst_bytes, void *stream);
int spd_model_verif_rows(spd_model_handle m, int32_t *rows, int max_rows);
int spd_model_verif_info(spd_model_handle m, int *r, int *truth, int *n_entries, int *every, int *capacity, long long *taken, int *in_loop,
                         long long *applied);
int spd_verif_host(const double *x, int r, const double *y, const double *w, double *out4, int32_t *hist66);
/* The quantile tape: the distribution over the members at every grid point -- minimum, maximum, quantiles and exceedance
 * probabilities of a masked ensemble --, recorded on the device at scheduled steps inside spd_model_step /
 * spd_model_step_checked_begin calls of any length (in-loop mode) or once on the state as it stands (_apply).  It writes nothing
 * into the model.  Off unless configured, and a model that never configures it issues the launches it always issued.
 * Configuration.  mask[M] (int32, 0 or 1): the members with mask 1 are the ensemble a_0 < ... < a_(r-1), 2 <= r <= 64; the others
 * are neither loaded nor stored.  E entries (name, level, op, param), 1 <= E <= 64; name is any name the verification tape accepts
 * (the statistics' catalogue, the derived and pressure-level names, precnv and precls in their stored precision); the names on
 * target levels and mslp need spd_model_plev_configure first.  op: SPD_Q_MIN, SPD_Q_MAX (param is not read), SPD_Q_QUANTILE (param
 * is q, 0 <= q <= 1), SPD_Q_PROB_ABOVE, SPD_Q_PROB_BELOW (param is a finite threshold in the unit an fp64 tape holds the name
 * in).  every >= 1; capacity >= 1 slots of the ring.
 * Value.  x_j[p], p = 96 row + column, is what an fp64 tape of that name holds at that level for member a_j at that step: the
 * same front end (run over the member ranges that cover the mask), export units and stored precision of precnv / precls.
 * s_0 ... s_(r-1) is the stable ascending order of x_0 ... x_(r-1): x_j stands before x_k iff x_j < x_k, or neither is less than
 * the other and j < k (numpy's sort(kind="stable"); where -0.0 and +0.0 meet, the member index decides which sign bit comes
 * first).  A state that the range check accepts holds no NaN, and what a NaN gives is not specified.
 *     min = s_0;  max = s_(r-1)
 *     quantile q:  h = fl(q (r - 1)), lo = floor(h), f = h - lo (exact), hi = min(lo + 1, r - 1), formed once on the host.
 *                  f == 0: s_lo, no arithmetic.  Otherwise v = s_lo + f (s_hi - s_lo) in fp64, the subtraction, the product and
 *                  the sum each rounded on its own (no fused multiply-add), then v = s_hi if v > s_hi.  So s_lo <= v <= s_hi, and
 *                  v does not decrease with q.
 *     prob_above thr:  #{j : x_j > thr} / r;   prob_below thr:  #{j : x_j < thr} / r   (strict; one division, one rounding)
 * No operation depends on the launch plan, so the bits are the same in every plan.
 * Ring.  One slot per event: [E][4608] fp64, entry k in the caller's order.  The step counter and the date of an event's state are
 * kept on the host (_rows: 6 int32, oldest first).
 * Schedule.  In-loop, after the step that leaves the absolute step counter at n with n % every == 0.  A call with the in-loop
 * quantile tape is issued in segments that end at the multiples of the `every` of each looping joined consumer (this one, breeding
 * or assimilation, verification); at such a step: the quantile sample if due, the verification's phase 0 if due, the rescale or
 * analysis if due, the verification's phase 1 if an analysis was applied.  The sample is always the state the step left, before
 * an in-loop analysis.  It is bit for bit the host loop  step(k); _apply; step(k); ...  -- checked calls included --, and no
 * state bit and no other recorder's ring differs from a run without it.
 *   _configure  one hipMalloc of its own (synchronises the device); the ring is empty, `applied` 0.  SPD_E_ARG, before anything is
 *               allocated, in this order: every < 1; capacity < 1; in_loop neither 0 nor 1; n_entries outside 1 ... 64; null
 *               lists; per entry an unknown name, a level out of range, an unknown op, a quantile that is not within 0 ... 1
 *               (NaN included), a threshold that is not finite; a null mask; a null model; a checked call in flight; a mask entry
 *               that is not 0 or 1; r outside 2 ... 64; a pressure-level name without target levels.  SPD_E_DEVICE when the
 *               allocation fails (the byte count is in the message): the tape is off, the model as usable as before.
 *   spd_qtape_check  the same checks without a model, for `members` members (mask may be NULL: only the rest is checked then).
 *   _off        switches it off and frees everything.
 *   _reset      empties the ring (no device work).  spd_model_init does the same.
 *   _apply      one event on the state as it stands, stream-ordered; writes a ring slot and nothing else.
 *   _compute    the planes [E][4608] fp64 of the state as it stands into device memory; writes no ring.  It uses the
 *               configuration's slab: order it against _apply and the steps by the stream.
 *   _read       the events [t0, t0 + nt) of the held ones, oldest first, of entry `entry` as [nt][4608] fp64 into device memory.
 *               Refused while a checked call is in flight and after a failed range check of a checked call until _reset or
 *               spd_model_init.
 *   _rows       rows[held][6] (host memory): step counter, year, month, day, hour, minute of the event's state.
 *   _info       r, E, every, capacity, events taken since _configure / _reset, the mode, and `applied`: the events recorded since
 *               _configure; any pointer may be NULL; all zero without a configuration.
 *   spd_qtape_host  one plane's entries as the device forms them, compiled for the host: x [r][4608] -> out [n_entries][4608].
 * spd_model_plev_configure is refused while an entry is a pressure-level name.  spd_model_copy_member does not carry the
 * configuration, and the outer boundary (spd_parallel_step*) does not keep it: order statistics of two ensembles do not merge. */
#define SPD_Q_MIN 0
#define SPD_Q_MAX 1
#define SPD_Q_QUANTILE 2
#define SPD_Q_PROB_ABOVE 3
#define SPD_Q_PROB_BELOW 4
int spd_qtape_check(const char *const *names, const int *levels, const int *ops, const double *params, int n_entries, const int32_t *mask,
                    int members, int every, int capacity, int in_loop);
int spd_model_qtape_configure(spd_model_handle m, const char *const *names, const int *levels, const int *ops, const double *params, int n_entries,
                              const int32_t *mask, int every, int capacity, int in_loop);
int spd_model_qtape_off(spd_model_handle m);
int spd_model_qtape_reset(spd_model_handle m);
int spd_model_qtape_apply(spd_model_handle m, void *stream);
int spd_model_qtape_compute(spd_model_handle m, void *dst_device, size_t dst_bytes, void *stream);
int spd_model_qtape_read(spd_model_handle m, int entry, int t0, int nt, void *dst_device, size_t dst_bytes, void *stream);
int spd_model_qtape_rows(spd_model_handle m, int32_t *rows, int max_rows);
int spd_model_qtape_info(spd_model_handle m, int *r, int *n_entries, int *every, int *capacity, long long *taken, int *in_loop, long long *applied);
int spd_qtape_host(const double *x, int r, const int *ops, const double *params, int n_entries, double *out);
/* Spectra by total wavenumber and global means of the spectral state, recorded on the device inside spd_model_step /
 * spd_model_step_checked_begin calls of any length, or computed on the state as it stands.  Plain sums over the spectral
 * coefficients of time level 1 (the level spd_model_spectral2grid exports): no transform.  A spectral field is complex [32 n][31 m],
 * the total wavenumber of an element is l = m + n, and with w_0 = 1, w_m = 2 otherwise, S_l(f) = sum over m = 0 ... min(l, 30) of
 * w_m |f_l^m|^2 (m ascending, fp64, one lane: a sample is the same bits whatever the launch plan).  Names, all fp64:
 *   ke_rot_spectrum [8][32]  1/4 elm2(l) S_l(vorticity), J/kg (elm2: a^2 / (l (l + 1)), 0 at l = 0)
 *   ke_div_spectrum [8][32]  the same of the divergence
 *   t_spectrum      [8][32]  1/2 S_l(T), K^2: its sum over l is the global area mean of T^2, bin 0 the squared mean
 *   q_spectrum      [8][32]  the same of the tracer in its stored unit (g/kg)
 *   lnps_spectrum   [32]     the same of the stored ln(ps / 1e5 Pa)
 *   t_mean, q_mean  [8]      the global area mean: Re f_0^0 * sqrt(1/2)
 *   lnps_mean       [1]      the same
 * A ring buffer in device memory, per model, holds the last `capacity` samples of the chosen names for every member; one sample is
 * taken after every step that leaves the model's absolute step counter at a multiple of `every`, by each member group on its own
 * stream behind its last launch of that step (and behind the statistics' and the tape's samples): one launch, no other launch of
 * the step changes, and nothing of the run does.
 *   _configure  allocates the ring (one hipMalloc of its own; synchronises the device) and empties it; n_names = 0 switches the
 *               spectra off and frees it.  SPD_E_ARG for an unknown or repeated name, every < 1, capacity < 1, a size beyond size_t,
 *               or while a checked call is in flight.  SPD_E_DEVICE with the number of bytes asked for when the allocation fails:
 *               the spectra are then off and the model as usable as before.
 *   _reset      empties the ring (host only, no device work).  spd_model_init does the same.
 *   _info       taken: samples since the last reset; held = min(taken, capacity); any pointer may be NULL.
 *   _times      rows[held][6] for the held samples, oldest first: the absolute step counter after the sampled step, then year,
 *               month, day, hour, minute of the sampled state (host memory).  Returns the number of rows written (<= max_rows).
 *   _read       members [first, first + count) and samples [t0, t0 + nt) of the held ones, oldest first, of one name into
 *               dst_device[count][nt][...] doubles, stream-ordered.  SPD_E_SIZE when dst_bytes is too small.
 *   _compute    the same kernel on the state as it stands, without a ring and without _configure: the members [first, first +
 *               count) of every name given into dst_device, [count][...] per name, one name after the other in the order given,
 *               stream-ordered.
 * Reads fail (SPD_E_ARG, with the reason) while a checked call is in flight and after a checked call that reported a failed range
 * check (the message names the member and the step): the series stays invalid until _reset or spd_model_init.
 * spd_model_copy_member does not carry the ring, and the outer boundary (spd_parallel_step*) does not keep it across the models
 * it merges and splits. */
int spd_model_spectra_configure(spd_model_handle m, const char *const *names, int n_names, int every, int capacity);
int spd_model_spectra_reset(spd_model_handle m);
int spd_model_spectra_info(spd_model_handle m, long long *taken, int *held, int *capacity, int *every);
int spd_model_spectra_times(spd_model_handle m, int32_t *rows, int max_rows);
int spd_model_spectra_read(spd_model_handle m, const char *name, int first, int count, int t0, int nt, void *dst_device,
                           size_t dst_bytes, void *stream);
int spd_model_spectra_compute(spd_model_handle m, const char *const *names, int n_names, int first, int count, void *dst_device,
                              size_t dst_bytes, void *stream);
/* modelstate_init_sst_anom (speedy_driver.f90.j2:225-237): sst_anom(ix, il, 0:n_months+1) per member, zero-filled */
int spd_model_init_sst_anom(spd_model_handle m, int n_months);
/* Stochastically perturbed parametrisation tendencies (sppt.f90; compile-time off and non-functional in the reference:
 * PARITY UNPINNED, see csrc/sppt.hip).  Deterministic: the noise is a function of (seed, first_member_id + member, step,
 * level, coefficient).  While on, every step advances the AR(1) spectral pattern (registry names sppt_spec, sppt_pattern). */
int spd_model_set_sppt(spd_model_handle m, int on, uint64_t seed, int64_t first_member_id);
/* device-to-device copy of every registered variable of one member into a member of another model on the same GPU (not its
 * time statistics: spd_model_stats_*) */
int spd_model_copy_member(spd_model_handle dst, int dst_member, spd_model_handle src, int src_member, void *stream);
/* the named registry variables only; the two models may live on different GPUs (device-to-device over xGMI,
 * hipMemcpyPeerAsync): how one process hands the shared boundary fields to the members it keeps on its other devices */
int spd_model_copy_vars(spd_model_handle dst, int dst_member, spd_model_handle src, int src_member, const char *const *names,
                        int n_names, void *stream);
/* the same copies enqueued only: no device is synchronised first, so the caller must have made sure that nothing in flight on
 * either device still uses the arrays (spd_broadcast_boundary synchronises every device once, then enqueues all its copies);
 * `stream` is a stream of the DESTINATION device, which is the current device when the call returns */
int spd_model_copy_vars_enqueue(spd_model_handle dst, int dst_member, spd_model_handle src, int src_member,
                                const char *const *names, int n_names, void *stream);
/* ONE collective broadcast of the named (fp64) variables between device models that live on different GPUs of this process:
 * member members[root] of models[root] into member members[i] of every other models[i] -- RCCL (ncclBroadcast in one group call,
 * single-process communicators) over xGMI, on each device's null stream; the caller synchronises the devices before and
 * after.  RCCL (librccl.so.1) is loaded when this is first called; SPD_E_DEVICE with the reason when it cannot be.  n = 1 is a
 * broadcast to nobody (it still initialises the communicator).  Every (variable, model) pair is validated before RCCL is
 * touched (SPD_E_ARG / SPD_E_SIZE: nothing was enqueued).  RCCL's initialisation, its group call and the completion of the
 * broadcasts are each waited for PYSPEEDY_AMD_RCCL_TIMEOUT seconds (default 30) at most: an initialisation that does not come
 * back gives SPD_E_DEVICE (nothing enqueued: the caller may copy point to point instead, and RCCL is not tried again in this
 * process), a group call or broadcast that does not come back SPD_E_TIMEOUT (nothing may be queued behind it). */
int spd_model_broadcast_vars(const spd_model_handle *models, const int *members, int n, int root, const char *const *names,
                             int n_names);

#ifdef __cplusplus
}
#endif
#endif /* PYSPEEDY_AMD_H */
