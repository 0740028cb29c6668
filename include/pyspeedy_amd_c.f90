!> ISO_C_BINDING interface to libpyspeedy_amd.so (include/pyspeedy_amd.h) for a Fortran host: what a maintainer of
!! speedy.f90 adds to call the MI355X backend.  The outer boundary (spd_model_*) takes HOST arrays in the reference's own
!! shapes and order, so a Fortran program drives whole model runs without any HIP call of its own; the operator-level entry
!! points (spd_spec2grid ...) take device pointers (type(c_ptr) from hipMalloc) and a stream.
!!
!! Replaces, call for call, the procedures of registry/templates/speedy_driver.f90.j2:
!!   modelstate_init -> spd_create + spd_model_create     set_<v> / get_<v> -> spd_model_set / spd_model_get
!!   init            -> spd_model_init                    step / parallel_step -> spd_model_step
!!   check           -> spd_model_check                   transform_spectral2grid ... -> spd_model_spectral2grid ...
!! and, without a counterpart there: time statistics on the device (spd_model_stats_*), pressure-level fields (spd_model_plev_*),
!! time series recorded on the device (spd_model_tape_*), spectra of the spectral state (spd_model_spectra_*), the series of
!! the ensemble mean and spread (spd_model_enstape_*), window sums, means and extremes of the physics fluxes (spd_model_acctape_*)
!! window means, extremes and threshold counts of the state's fields (spd_model_wintape_*, spd_wintape_plan), and nudging of the
!! spectral state toward target fields inside the device loop (spd_model_nudge_*), and breeding: the rescaling of member
!! perturbations against their control runs inside the device loop (spd_model_breed_*, spd_breed_check), orthonormalised on request,
!! and assimilation: an ensemble square-root filter inside the device loop (spd_model_assim_*, spd_assim_check), and the
!! verification tape: scores of an ensemble against a truth member inside the device loop (spd_model_verif_*, spd_verif_check),
!! and the quantile tape: minimum, maximum, quantiles and exceedance probabilities over the members at every grid point inside
!! the device loop (spd_model_qtape_*, spd_qtape_check)
module pyspeedy_amd_c
    use iso_c_binding
    implicit none

    integer(c_int), parameter :: SPD_OK = 0, SPD_E_ARG = -1, SPD_E_DEVICE = -2, SPD_E_SIZE = -3
    integer(c_int), parameter :: SPD_STATS_MEAN = 0, SPD_STATS_VARIANCE = 1, SPD_STATS_STD = 2
    integer(c_int), parameter :: SPD_TAPE_F32 = 0, SPD_TAPE_F64 = 1
    integer(c_int), parameter :: SPD_ENS_MEAN = 0, SPD_ENS_STD = 1, SPD_ENS_M2 = 2
    integer(c_int), parameter :: SPD_ACC_SUM = 0, SPD_ACC_MEAN = 1, SPD_ACC_MIN = 2, SPD_ACC_MAX = 3
    integer(c_int), parameter :: SPD_WIN_SUM = 0, SPD_WIN_MEAN = 1, SPD_WIN_MIN = 2, SPD_WIN_MAX = 3
    integer(c_int), parameter :: SPD_WIN_COUNT_ABOVE = 4, SPD_WIN_COUNT_BELOW = 5
    integer(c_int), parameter :: SPD_WINDOW_STEPS = 0, SPD_WINDOW_DAY = 1, SPD_WINDOW_MONTH = 2
    integer(c_int), parameter :: SPD_Q_MIN = 0, SPD_Q_MAX = 1, SPD_Q_QUANTILE = 2, SPD_Q_PROB_ABOVE = 3, SPD_Q_PROB_BELOW = 4
    integer(c_int), parameter :: SPD_TRACK_MIN = 0, SPD_TRACK_MAX = 1
    integer(c_int), parameter :: SPD_FIL_MEAN = 0, SPD_FIL_COV = 1, SPD_FIL_LAST = 2

    interface
        ! ---- context ------------------------------------------------------------------------------------------
        integer(c_int) function spd_create(handle, device) bind(C, name="spd_create")
            import :: c_ptr, c_int
            type(c_ptr), intent(out) :: handle
            integer(c_int), value :: device
        end function
        integer(c_int) function spd_destroy(handle) bind(C, name="spd_destroy")
            import :: c_ptr, c_int
            type(c_ptr), value :: handle
        end function
        type(c_ptr) function spd_last_error() bind(C, name="spd_last_error")
            import :: c_ptr
        end function
        integer(c_long) function spd_get_table_host(handle, name, buf, buf_elems) bind(C, name="spd_get_table_host")
            import :: c_ptr, c_long, c_char, c_double, c_size_t
            type(c_ptr), value :: handle
            character(kind=c_char), intent(in) :: name(*)
            real(c_double), intent(out) :: buf(*)
            integer(c_size_t), value :: buf_elems
        end function
        ! host only (no device): initialize_control + nsteps x advance_date / update_forcing_params, model_control.f90:79-185;
        ! row 1 of every output = after initialize_control, row s + 1 = after s steps; ymdhm(5, nsteps + 1)
        integer(c_int) function spd_calendar_walk(year, month, day, hour, minute, nsteps, ymdhm, month_idx, imont1, tmonth, tyear) &
                bind(C, name="spd_calendar_walk")
            import :: c_int, c_int32_t, c_double
            integer(c_int), value :: year, month, day, hour, minute, nsteps
            integer(c_int32_t), intent(out) :: ymdhm(5, *), month_idx(*), imont1(*)
            real(c_double), intent(out) :: tmonth(*), tyear(*)
        end function
        ! host only: get_zonal_average_fields (shortwave_radiation.f90:218-322) for a fraction of the year; out(48, 5) =
        ! flux_solar_in, flux_ozone_upper, flux_ozone_lower, zenit_correction, stratospheric_correction by latitude
        integer(c_int) function spd_daily_forcing_host(tyear, out) bind(C, name="spd_daily_forcing_host")
            import :: c_int, c_double
            real(c_double), value :: tyear
            real(c_double), intent(out) :: out(48, 5)
        end function

        ! ---- operator level: device pointers, explicit batch count, stream ------------------------------------------
        integer(c_int) function spd_spec2grid(handle, spec, grid, kcos, nfields, stream) bind(C, name="spd_spec2grid")
            import :: c_ptr, c_int
            type(c_ptr), value :: handle, spec, grid, stream
            integer(c_int), value :: kcos, nfields
        end function
        integer(c_int) function spd_grid2spec(handle, grid, spec, nfields, stream) bind(C, name="spd_grid2spec")
            import :: c_ptr, c_int
            type(c_ptr), value :: handle, grid, spec, stream
            integer(c_int), value :: nfields
        end function
        integer(c_int) function spd_vort2vel(handle, vor, div, ucos, vcos, nfields, stream) bind(C, name="spd_vort2vel")
            import :: c_ptr, c_int
            type(c_ptr), value :: handle, vor, div, ucos, vcos, stream
            integer(c_int), value :: nfields
        end function
        integer(c_int) function spd_grid_vel2vort(handle, ug, vg, vor, div, kcos, nfields, stream) &
                bind(C, name="spd_grid_vel2vort")
            import :: c_ptr, c_int
            type(c_ptr), value :: handle, ug, vg, vor, div, stream
            integer(c_int), value :: kcos, nfields
        end function

        ! ---- ensemble model: host arrays in the reference's shapes ---------------------------------------------------
        integer(c_int) function spd_model_create(handle, nmembers, model) bind(C, name="spd_model_create")
            import :: c_ptr, c_int
            type(c_ptr), value :: handle
            integer(c_int), value :: nmembers
            type(c_ptr), intent(out) :: model
        end function
        integer(c_int) function spd_model_destroy(model) bind(C, name="spd_model_destroy")
            import :: c_ptr, c_int
            type(c_ptr), value :: model
        end function
        integer(c_int) function spd_model_set(model, name, member, host_buf, bytes) bind(C, name="spd_model_set")
            import :: c_ptr, c_int, c_char, c_size_t
            type(c_ptr), value :: model
            character(kind=c_char), intent(in) :: name(*)
            integer(c_int), value :: member          ! 0-based; -1 = every member
            type(*), intent(in) :: host_buf(*)
            integer(c_size_t), value :: bytes
        end function
        integer(c_int) function spd_model_get(model, name, member, host_buf, bytes) bind(C, name="spd_model_get")
            import :: c_ptr, c_int, c_char, c_size_t
            type(c_ptr), value :: model
            character(kind=c_char), intent(in) :: name(*)
            integer(c_int), value :: member
            type(*) :: host_buf(*)
            integer(c_size_t), value :: bytes
        end function
        integer(c_int) function spd_model_init_sst_anom(model, n_months) bind(C, name="spd_model_init_sst_anom")
            import :: c_ptr, c_int
            type(c_ptr), value :: model
            integer(c_int), value :: n_months
        end function
        integer(c_int) function spd_model_init(model, year, month, day, hour, minute, stream) bind(C, name="spd_model_init")
            import :: c_ptr, c_int
            type(c_ptr), value :: model, stream
            integer(c_int), value :: year, month, day, hour, minute
        end function
        integer(c_int) function spd_model_step(model, nsteps, stream) bind(C, name="spd_model_step")
            import :: c_ptr, c_int
            type(c_ptr), value :: model, stream
            integer(c_int), value :: nsteps
        end function
        integer(c_int) function spd_model_check(model, time_level, error_codes, diag, stream) bind(C, name="spd_model_check")
            import :: c_ptr, c_int, c_int32_t
            type(c_ptr), value :: model, diag, stream   ! diag: c_null_ptr or c_loc of real(c_double) (kx, 3, nmembers)
            integer(c_int), value :: time_level
            integer(c_int32_t), intent(out) :: error_codes(*)
        end function
        integer(c_int) function spd_model_spectral2grid(model, first, count, stream) bind(C, name="spd_model_spectral2grid")
            import :: c_ptr, c_int
            type(c_ptr), value :: model, stream
            integer(c_int), value :: first, count
        end function
        integer(c_int) function spd_model_grid2spectral(model, first, count, stream) bind(C, name="spd_model_grid2spectral")
            import :: c_ptr, c_int
            type(c_ptr), value :: model, stream
            integer(c_int), value :: first, count
        end function
        integer(c_int) function spd_model_grid_filter(model, first, count, stream) bind(C, name="spd_model_grid_filter")
            import :: c_ptr, c_int
            type(c_ptr), value :: model, stream
            integer(c_int), value :: first, count
        end function
        ! time-mean statistics accumulated on the device inside spd_model_step calls (pyspeedy_amd.h: spd_model_stats_*).
        ! names: an array of c_ptr to NUL-terminated strings ("t_grid"//c_null_char, ...); kind: SPD_STATS_MEAN / _VARIANCE / _STD
        integer(c_int) function spd_model_stats_configure(model, names, n_names, every, with_variance) &
                bind(C, name="spd_model_stats_configure")
            import :: c_ptr, c_int
            type(c_ptr), value :: model
            type(c_ptr), intent(in) :: names(*)
            integer(c_int), value :: n_names, every, with_variance
        end function
        integer(c_int) function spd_model_stats_reset(model) bind(C, name="spd_model_stats_reset")
            import :: c_ptr, c_int
            type(c_ptr), value :: model
        end function
        integer(c_int) function spd_model_stats_samples(model) bind(C, name="spd_model_stats_samples")
            import :: c_ptr, c_int
            type(c_ptr), value :: model
        end function
        integer(c_int) function spd_model_stats_read(model, name, kind, first, count, dst_device, dst_bytes, stream) &
                bind(C, name="spd_model_stats_read")
            import :: c_ptr, c_int, c_char, c_size_t
            type(c_ptr), value :: model, dst_device, stream
            character(kind=c_char), intent(in) :: name(*)
            integer(c_int), value :: kind, first, count
            integer(c_size_t), value :: dst_bytes
        end function
        integer(c_int) function spd_model_stats_ensemble(model, name, kind, dst_device, dst_bytes, stream) &
                bind(C, name="spd_model_stats_ensemble")
            import :: c_ptr, c_int, c_char, c_size_t
            type(c_ptr), value :: model, dst_device, stream
            character(kind=c_char), intent(in) :: name(*)
            integer(c_int), value :: kind
            integer(c_size_t), value :: dst_bytes
        end function
        ! pressure-level fields and mean sea-level pressure (pyspeedy_amd.h: spd_model_plev_*).  levels_pa: Pa; names as for the
        ! statistics ("z_plev"//c_null_char, ...; n_names = 0: all six); refresh = 1: spd_model_spectral2grid first
        integer(c_int) function spd_model_plev_configure(model, levels_pa, n) bind(C, name="spd_model_plev_configure")
            import :: c_ptr, c_int, c_double
            type(c_ptr), value :: model
            real(c_double), intent(in) :: levels_pa(*)
            integer(c_int), value :: n
        end function
        integer(c_int) function spd_model_plev_levels(model, out, cap) bind(C, name="spd_model_plev_levels")
            import :: c_ptr, c_int, c_double
            type(c_ptr), value :: model
            real(c_double), intent(out) :: out(*)
            integer(c_int), value :: cap
        end function
        integer(c_int) function spd_model_plev_compute(model, names, n_names, first, count, refresh, stream) &
                bind(C, name="spd_model_plev_compute")
            import :: c_ptr, c_int
            type(c_ptr), value :: model, stream
            type(c_ptr), intent(in) :: names(*)
            integer(c_int), value :: n_names, first, count, refresh
        end function
        integer(c_int) function spd_model_plev_read(model, name, first, count, dst_device, dst_bytes, stream) &
                bind(C, name="spd_model_plev_read")
            import :: c_ptr, c_int, c_char, c_size_t
            type(c_ptr), value :: model, dst_device, stream
            character(kind=c_char), intent(in) :: name(*)
            integer(c_int), value :: first, count
            integer(c_size_t), value :: dst_bytes
        end function
        ! derived fields (pyspeedy_amd.h: spd_model_derive_*): vor_grid, div_grid, omega_grid, rh_grid, theta_grid (8 levels), tcwv,
        ! ivt_u, ivt_v, ke_col (one plane), omega_plev, vor_plev, div_plev, rh_plev, theta_plev (the levels of spd_model_plev_configure)
        integer(c_int) function spd_model_derive_compute(model, names, n_names, first, count, refresh, stream) &
                bind(C, name="spd_model_derive_compute")
            import :: c_ptr, c_int
            type(c_ptr), value :: model, stream
            type(c_ptr), intent(in) :: names(*)
            integer(c_int), value :: n_names, first, count, refresh
        end function
        integer(c_int) function spd_model_derive_read(model, name, first, count, dst_device, dst_bytes, stream) &
                bind(C, name="spd_model_derive_read")
            import :: c_ptr, c_int, c_char, c_size_t
            type(c_ptr), value :: model, dst_device, stream
            character(kind=c_char), intent(in) :: name(*)
            integer(c_int), value :: first, count
            integer(c_size_t), value :: dst_bytes
        end function
        ! the tape: time series of fields recorded on the device inside spd_model_step calls (pyspeedy_amd.h: spd_model_tape_*).
        ! names as for the statistics; dtype: SPD_TAPE_F32 (0) / SPD_TAPE_F64 (1); rows: (6, held) int32, oldest sample first:
        ! step counter after the sampled step, year, month, day, hour, minute; _read: (96, 48[, levels], nt, count) in the dtype
        integer(c_int) function spd_model_tape_configure(model, names, n_names, every, capacity, dtype) &
                bind(C, name="spd_model_tape_configure")
            import :: c_ptr, c_int
            type(c_ptr), value :: model
            type(c_ptr), intent(in) :: names(*)
            integer(c_int), value :: n_names, every, capacity, dtype
        end function
        integer(c_int) function spd_model_tape_reset(model) bind(C, name="spd_model_tape_reset")
            import :: c_ptr, c_int
            type(c_ptr), value :: model
        end function
        integer(c_int) function spd_model_tape_info(model, taken, held, capacity, every, dtype) bind(C, name="spd_model_tape_info")
            import :: c_ptr, c_int, c_long_long
            type(c_ptr), value :: model
            integer(c_long_long), intent(out) :: taken
            integer(c_int), intent(out) :: held, capacity, every, dtype
        end function
        integer(c_int) function spd_model_tape_times(model, rows, max_rows) bind(C, name="spd_model_tape_times")
            import :: c_ptr, c_int, c_int32_t
            type(c_ptr), value :: model
            integer(c_int32_t), intent(out) :: rows(6, *)
            integer(c_int), value :: max_rows
        end function
        integer(c_int) function spd_model_tape_read(model, name, first, count, t0, nt, dst_device, dst_bytes, stream) &
                bind(C, name="spd_model_tape_read")
            import :: c_ptr, c_int, c_char, c_size_t
            type(c_ptr), value :: model, dst_device, stream
            character(kind=c_char), intent(in) :: name(*)
            integer(c_int), value :: first, count, t0, nt
            integer(c_size_t), value :: dst_bytes
        end function
        ! the ensemble tape: mean and spread over all members of a model as a time series recorded on the device inside
        ! spd_model_step calls (pyspeedy_amd.h: spd_model_enstape_*).  names as for the statistics; rows as the tape's; kind:
        ! SPD_ENS_MEAN (0) / SPD_ENS_STD (1) / SPD_ENS_M2 (2); _read: (96, 48[, levels], nt) real(c_double)
        integer(c_int) function spd_model_enstape_configure(model, names, n_names, every, capacity) &
                bind(C, name="spd_model_enstape_configure")
            import :: c_ptr, c_int
            type(c_ptr), value :: model
            type(c_ptr), intent(in) :: names(*)
            integer(c_int), value :: n_names, every, capacity
        end function
        integer(c_int) function spd_model_enstape_reset(model) bind(C, name="spd_model_enstape_reset")
            import :: c_ptr, c_int
            type(c_ptr), value :: model
        end function
        integer(c_int) function spd_model_enstape_info(model, taken, held, capacity, every, members) &
                bind(C, name="spd_model_enstape_info")
            import :: c_ptr, c_int, c_long_long
            type(c_ptr), value :: model
            integer(c_long_long), intent(out) :: taken
            integer(c_int), intent(out) :: held, capacity, every, members
        end function
        integer(c_int) function spd_model_enstape_times(model, rows, max_rows) bind(C, name="spd_model_enstape_times")
            import :: c_ptr, c_int, c_int32_t
            type(c_ptr), value :: model
            integer(c_int32_t), intent(out) :: rows(6, *)
            integer(c_int), value :: max_rows
        end function
        integer(c_int) function spd_model_enstape_read(model, name, kind, t0, nt, dst_device, dst_bytes, stream) &
                bind(C, name="spd_model_enstape_read")
            import :: c_ptr, c_int, c_char, c_size_t
            type(c_ptr), value :: model, dst_device, stream
            character(kind=c_char), intent(in) :: name(*)
            integer(c_int), value :: kind, t0, nt
            integer(c_size_t), value :: dst_bytes
        end function
        ! the accumulation tape: window sums, means, minima and maxima of the column physics' 2-D outputs, accumulated on the device
        ! behind every step (pyspeedy_amd.h: spd_model_acctape_*).  An entry is names(k) with ops(k): SPD_ACC_SUM (0) / _MEAN (1) /
        ! _MIN (2) / _MAX (3); dtype as the tape's; rows(7, *): the tape's six and the number of steps in the window;
        ! _read: (96, 48[, 3], nt, count) in the ring's dtype
        integer(c_int) function spd_model_acctape_configure(model, names, ops, n_entries, every, capacity, dtype) &
                bind(C, name="spd_model_acctape_configure")
            import :: c_ptr, c_int
            type(c_ptr), value :: model
            type(c_ptr), intent(in) :: names(*)
            integer(c_int), intent(in) :: ops(*)
            integer(c_int), value :: n_entries, every, capacity, dtype
        end function
        integer(c_int) function spd_model_acctape_reset(model) bind(C, name="spd_model_acctape_reset")
            import :: c_ptr, c_int
            type(c_ptr), value :: model
        end function
        integer(c_int) function spd_model_acctape_info(model, taken, held, capacity, every, dtype) &
                bind(C, name="spd_model_acctape_info")
            import :: c_ptr, c_int, c_long_long
            type(c_ptr), value :: model
            integer(c_long_long), intent(out) :: taken
            integer(c_int), intent(out) :: held, capacity, every, dtype
        end function
        integer(c_int) function spd_model_acctape_times(model, rows, max_rows) bind(C, name="spd_model_acctape_times")
            import :: c_ptr, c_int, c_int32_t
            type(c_ptr), value :: model
            integer(c_int32_t), intent(out) :: rows(7, *)
            integer(c_int), value :: max_rows
        end function
        integer(c_int) function spd_model_acctape_read(model, name, op, first, count, t0, nt, dst_device, dst_bytes, stream) &
                bind(C, name="spd_model_acctape_read")
            import :: c_ptr, c_int, c_char, c_size_t
            type(c_ptr), value :: model, dst_device, stream
            character(kind=c_char), intent(in) :: name(*)
            integer(c_int), value :: op, first, count, t0, nt
            integer(c_size_t), value :: dst_bytes
        end function
        ! the window tape: window sums, means, minima, maxima and threshold counts of the state's grid-space fields, accumulated on
        ! the device behind the sampled steps; windows close every `every` steps, at midnight or at month ends (pyspeedy_amd.h:
        ! spd_model_wintape_*).  An entry is names(k) with ops(k): SPD_WIN_SUM (0) ... _COUNT_BELOW (5); thresholds: c_loc of a
        ! real(c_double) array of n_entries values, read for the count ops only (c_null_ptr without count ops); dtype as the tape's;
        ! rows(8, *): the tape's six, the samples and the steps in the window; _read: (96, 48[, levels], nt, count) in the ring's
        ! dtype.  spd_wintape_plan: the windows that close within nsteps steps from a date and a step counter (no model needed)
        integer(c_int) function spd_model_wintape_configure(model, names, ops, thresholds, n_entries, window, every, sample_every, &
                capacity, dtype) bind(C, name="spd_model_wintape_configure")
            import :: c_ptr, c_int
            type(c_ptr), value :: model, thresholds
            type(c_ptr), intent(in) :: names(*)
            integer(c_int), intent(in) :: ops(*)
            integer(c_int), value :: n_entries, window, every, sample_every, capacity, dtype
        end function
        integer(c_int) function spd_model_wintape_reset(model) bind(C, name="spd_model_wintape_reset")
            import :: c_ptr, c_int
            type(c_ptr), value :: model
        end function
        integer(c_int) function spd_model_wintape_info(model, taken, held, capacity, window, every, sample_every, dtype) &
                bind(C, name="spd_model_wintape_info")
            import :: c_ptr, c_int, c_long_long
            type(c_ptr), value :: model
            integer(c_long_long), intent(out) :: taken
            integer(c_int), intent(out) :: held, capacity, window, every, sample_every, dtype
        end function
        integer(c_int) function spd_model_wintape_times(model, rows, max_rows) bind(C, name="spd_model_wintape_times")
            import :: c_ptr, c_int, c_int32_t
            type(c_ptr), value :: model
            integer(c_int32_t), intent(out) :: rows(8, *)
            integer(c_int), value :: max_rows
        end function
        integer(c_int) function spd_model_wintape_read(model, name, op, first, count, t0, nt, dst_device, dst_bytes, stream) &
                bind(C, name="spd_model_wintape_read")
            import :: c_ptr, c_int, c_char, c_size_t
            type(c_ptr), value :: model, dst_device, stream
            character(kind=c_char), intent(in) :: name(*)
            integer(c_int), value :: op, first, count, t0, nt
            integer(c_size_t), value :: dst_bytes
        end function
        integer(c_int) function spd_wintape_plan(year, month, day, hour, minute, step0, nsteps, window, every, sample_every, rows, &
                max_rows) bind(C, name="spd_wintape_plan")
            import :: c_int, c_int32_t
            integer(c_int), value :: year, month, day, hour, minute, step0, nsteps, window, every, sample_every, max_rows
            integer(c_int32_t), intent(out) :: rows(8, *)
        end function
        ! the projection tape: weighted sums of single planes of the state's grid-space fields as scalar series, formed on the
        ! device behind the sampled steps (pyspeedy_amd.h: spd_model_projtape_*).  weights(96, 48, n_patterns); an entry is
        ! names(k) at the 0-based level levels(k) under the 0-based pattern patterns(k); rows(6, *): as the tape's; _read:
        ! real(c_double) (n_entries, nt, count)
        integer(c_int) function spd_model_projtape_configure(model, weights, n_patterns, names, levels, patterns, n_entries, every, &
                capacity) bind(C, name="spd_model_projtape_configure")
            import :: c_ptr, c_int, c_double
            type(c_ptr), value :: model
            real(c_double), intent(in) :: weights(*)
            type(c_ptr), intent(in) :: names(*)
            integer(c_int), intent(in) :: levels(*), patterns(*)
            integer(c_int), value :: n_patterns, n_entries, every, capacity
        end function
        integer(c_int) function spd_model_projtape_reset(model) bind(C, name="spd_model_projtape_reset")
            import :: c_ptr, c_int
            type(c_ptr), value :: model
        end function
        integer(c_int) function spd_model_projtape_info(model, taken, held, capacity, every, n_patterns, n_entries) &
                bind(C, name="spd_model_projtape_info")
            import :: c_ptr, c_int, c_long_long
            type(c_ptr), value :: model
            integer(c_long_long), intent(out) :: taken
            integer(c_int), intent(out) :: held, capacity, every, n_patterns, n_entries
        end function
        integer(c_int) function spd_model_projtape_times(model, rows, max_rows) bind(C, name="spd_model_projtape_times")
            import :: c_ptr, c_int, c_int32_t
            type(c_ptr), value :: model
            integer(c_int32_t), intent(out) :: rows(6, *)
            integer(c_int), value :: max_rows
        end function
        integer(c_int) function spd_model_projtape_read(model, first, count, t0, nt, dst_device, dst_bytes, stream) &
                bind(C, name="spd_model_projtape_read")
            import :: c_ptr, c_int, c_size_t
            type(c_ptr), value :: model, dst_device, stream
            integer(c_int), value :: first, count, t0, nt
            integer(c_size_t), value :: dst_bytes
        end function
        ! the track tape: the minimum or maximum of single planes of the state's grid-space fields over regions and where it lies,
        ! followed from sample to sample (pyspeedy_amd.h: spd_model_tracktape_*).  regions(96, 48, n_regions); an entry is names(k)
        ! at the 0-based level levels(k) over the 0-based region region_of(k), ops(k) SPD_TRACK_MIN / SPD_TRACK_MAX, radii(k) 0 ... 24;
        ! rows(6, *): as the tape's; _read: real(c_double) (4, n_entries, nt, count); _positions / _seed: (n_entries, count), 0-based
        ! points 96 j + i or -1; spd_track_point_host: plane(96, 48), mask(96, 48) of bytes, out4(4)
        integer(c_int) function spd_model_tracktape_configure(model, regions, n_regions, names, levels, region_of, ops, radii, &
                n_entries, every, capacity) bind(C, name="spd_model_tracktape_configure")
            import :: c_ptr, c_int, c_double
            type(c_ptr), value :: model
            real(c_double), intent(in) :: regions(*)
            type(c_ptr), intent(in) :: names(*)
            integer(c_int), intent(in) :: levels(*), region_of(*), ops(*), radii(*)
            integer(c_int), value :: n_regions, n_entries, every, capacity
        end function
        integer(c_int) function spd_model_tracktape_reset(model) bind(C, name="spd_model_tracktape_reset")
            import :: c_ptr, c_int
            type(c_ptr), value :: model
        end function
        integer(c_int) function spd_model_tracktape_info(model, taken, held, capacity, every, n_regions, n_entries) &
                bind(C, name="spd_model_tracktape_info")
            import :: c_ptr, c_int, c_long_long
            type(c_ptr), value :: model
            integer(c_long_long), intent(out) :: taken
            integer(c_int), intent(out) :: held, capacity, every, n_regions, n_entries
        end function
        integer(c_int) function spd_model_tracktape_times(model, rows, max_rows) bind(C, name="spd_model_tracktape_times")
            import :: c_ptr, c_int, c_int32_t
            type(c_ptr), value :: model
            integer(c_int32_t), intent(out) :: rows(6, *)
            integer(c_int), value :: max_rows
        end function
        integer(c_int) function spd_model_tracktape_read(model, first, count, t0, nt, dst_device, dst_bytes, stream) &
                bind(C, name="spd_model_tracktape_read")
            import :: c_ptr, c_int, c_size_t
            type(c_ptr), value :: model, dst_device, stream
            integer(c_int), value :: first, count, t0, nt
            integer(c_size_t), value :: dst_bytes
        end function
        integer(c_int) function spd_model_tracktape_positions(model, first, count, dst, max) &
                bind(C, name="spd_model_tracktape_positions")
            import :: c_ptr, c_int, c_int32_t
            type(c_ptr), value :: model
            integer(c_int), value :: first, count, max
            integer(c_int32_t), intent(out) :: dst(*)
        end function
        integer(c_int) function spd_model_tracktape_seed(model, first, count, src) bind(C, name="spd_model_tracktape_seed")
            import :: c_ptr, c_int, c_int32_t
            type(c_ptr), value :: model
            integer(c_int), value :: first, count
            integer(c_int32_t), intent(in) :: src(*)
        end function
        integer(c_int) function spd_track_point_host(plane, mask, prev, radius, op, out4) bind(C, name="spd_track_point_host")
            import :: c_int, c_double, c_signed_char
            real(c_double), intent(in) :: plane(*)
            integer(c_signed_char), intent(in) :: mask(*)
            integer(c_int), value :: prev, radius, op
            real(c_double), intent(out) :: out4(4)
        end function
        ! the filter tape: window means, covariances and last values of time-filtered planes of the state's grid-space fields
        ! (pyspeedy_amd.h: spd_model_filtape_*).  sections(5, sum of n_sections): b0, b1, b2, a1, a2 of each second-order section,
        ! filter after filter; an entry is names_a(k) at the 0-based level levels_a(k) through the 0-based filter filters(k) under
        ! ops(k) SPD_FIL_*, with names_b(k) (c_null_ptr: none) at levels_b(k) for a covariance of two fields; rows(8, *): as the
        ! window tape's with the counted samples; _read: (96, 48, nt, count) of one 0-based entry in the ring's dtype
        integer(c_int) function spd_model_filtape_configure(model, sections, n_sections, n_filters, names_a, levels_a, filters, ops, &
                names_b, levels_b, n_entries, window, every, sample_every, spinup, capacity, dtype) &
                bind(C, name="spd_model_filtape_configure")
            import :: c_ptr, c_int, c_double
            type(c_ptr), value :: model
            real(c_double), intent(in) :: sections(*)
            integer(c_int), intent(in) :: n_sections(*), levels_a(*), filters(*), ops(*), levels_b(*)
            type(c_ptr), intent(in) :: names_a(*), names_b(*)
            integer(c_int), value :: n_filters, n_entries, window, every, sample_every, spinup, capacity, dtype
        end function
        integer(c_int) function spd_model_filtape_off(model) bind(C, name="spd_model_filtape_off")
            import :: c_ptr, c_int
            type(c_ptr), value :: model
        end function
        integer(c_int) function spd_model_filtape_reset(model) bind(C, name="spd_model_filtape_reset")
            import :: c_ptr, c_int
            type(c_ptr), value :: model
        end function
        integer(c_int) function spd_model_filtape_info(model, taken, held, capacity, window, every, sample_every, spinup, dtype, &
                n_filters, n_planes, n_entries, filter_samples) bind(C, name="spd_model_filtape_info")
            import :: c_ptr, c_int, c_long_long
            type(c_ptr), value :: model
            integer(c_long_long), intent(out) :: taken, filter_samples
            integer(c_int), intent(out) :: held, capacity, window, every, sample_every, spinup, dtype, n_filters, n_planes, n_entries
        end function
        integer(c_int) function spd_model_filtape_times(model, rows, max_rows) bind(C, name="spd_model_filtape_times")
            import :: c_ptr, c_int, c_int32_t
            type(c_ptr), value :: model
            integer(c_int32_t), intent(out) :: rows(8, *)
            integer(c_int), value :: max_rows
        end function
        integer(c_int) function spd_model_filtape_read(model, entry, first, count, t0, nt, dst_device, dst_bytes, stream) &
                bind(C, name="spd_model_filtape_read")
            import :: c_ptr, c_int, c_size_t
            type(c_ptr), value :: model, dst_device, stream
            integer(c_int), value :: entry, first, count, t0, nt
            integer(c_size_t), value :: dst_bytes
        end function
        integer(c_int) function spd_filtape_check(sections, n_sections, n_filters, names_a, levels_a, filters, ops, names_b, levels_b, &
                n_entries, window, every, sample_every, spinup, capacity, dtype) bind(C, name="spd_filtape_check")
            import :: c_ptr, c_int, c_double
            real(c_double), intent(in) :: sections(*)
            integer(c_int), intent(in) :: n_sections(*), levels_a(*), filters(*), ops(*), levels_b(*)
            type(c_ptr), intent(in) :: names_a(*), names_b(*)
            integer(c_int), value :: n_filters, n_entries, window, every, sample_every, spinup, capacity, dtype
        end function
        integer(c_int) function spd_filtape_filter_host(sections, n_sections, x, n, y) bind(C, name="spd_filtape_filter_host")
            import :: c_int, c_double
            real(c_double), intent(in) :: sections(*), x(*)
            integer(c_int), value :: n_sections, n
            real(c_double), intent(out) :: y(*)
        end function
        ! nudging: relaxation of the spectral state toward target fields behind every step of spd_model_step (in_loop = 1) or once on
        ! the state as it stands (_apply) (pyspeedy_amd.h: spd_model_nudge_*).  names: any of vor, div, t, tr, ps; gains(32, 8,
        ! n_names) in [0, 1] by total wavenumber, level and name (ps reads its first row); member_mask: c_loc of an
        ! integer(c_int32_t) array of 0 / 1 per member, or c_null_ptr for all; a target is complex(c_double_complex) (31, 32, 8),
        ! (31, 32) for ps, passed by c_loc with its size in bytes; steps(n): strictly ascending absolute step stamps
        integer(c_int) function spd_model_nudge_configure(model, names, n_names, gains, member_mask, capacity, in_loop) &
                bind(C, name="spd_model_nudge_configure")
            import :: c_ptr, c_int, c_double
            type(c_ptr), value :: model, member_mask
            type(c_ptr), intent(in) :: names(*)
            real(c_double), intent(in) :: gains(32, 8, *)
            integer(c_int), value :: n_names, capacity, in_loop
        end function
        integer(c_int) function spd_model_nudge_set_times(model, steps, n) bind(C, name="spd_model_nudge_set_times")
            import :: c_ptr, c_int, c_int32_t
            type(c_ptr), value :: model
            integer(c_int32_t), intent(in) :: steps(*)
            integer(c_int), value :: n
        end function
        integer(c_int) function spd_model_nudge_set_target(model, slot, name, host, bytes) bind(C, name="spd_model_nudge_set_target")
            import :: c_ptr, c_int, c_char, c_size_t
            type(c_ptr), value :: model, host
            integer(c_int), value :: slot
            character(kind=c_char), intent(in) :: name(*)
            integer(c_size_t), value :: bytes
        end function
        integer(c_int) function spd_model_nudge_apply(model, first, count, stream) bind(C, name="spd_model_nudge_apply")
            import :: c_ptr, c_int
            type(c_ptr), value :: model, stream
            integer(c_int), value :: first, count
        end function
        integer(c_int) function spd_model_nudge_info(model, n_names, capacity, in_use, in_loop, applied) &
                bind(C, name="spd_model_nudge_info")
            import :: c_ptr, c_int, c_long_long
            type(c_ptr), value :: model
            integer(c_int), intent(out) :: n_names, capacity, in_use, in_loop
            integer(c_long_long), intent(out) :: applied
        end function
        ! breeding: the perturbation of a bred member against its control rescaled to `target` after every step that leaves the step
        ! counter at a multiple of `every` (in_loop = 1) or once on the state as it stands (_apply) (pyspeedy_amd.h:
        ! spd_model_breed_*).  control: c_loc of an integer(c_int32_t) array of one entry per member (0-based index of the control,
        ! -1: not bred), or c_null_ptr to switch breeding off; weights(8, 5) >= 0 by level and name (vor, div, t, tr, ps; ps reads
        ! its first entry); _read: what = 0 amplitude, 1 factor, (members, nt) fp64 in device memory; _rows: rows(6, *)
        integer(c_int) function spd_breed_check(control, members, weights, target, every, capacity, in_loop) &
                bind(C, name="spd_breed_check")
            import :: c_ptr, c_int, c_double
            type(c_ptr), value :: control
            real(c_double), intent(in) :: weights(8, 5)
            real(c_double), value :: target
            integer(c_int), value :: members, every, capacity, in_loop
        end function
        integer(c_int) function spd_model_breed_configure(model, control, weights, target, every, capacity, in_loop) &
                bind(C, name="spd_model_breed_configure")
            import :: c_ptr, c_int, c_double
            type(c_ptr), value :: model, control
            real(c_double), intent(in) :: weights(8, 5)
            real(c_double), value :: target
            integer(c_int), value :: every, capacity, in_loop
        end function
        integer(c_int) function spd_model_breed_apply(model, stream) bind(C, name="spd_model_breed_apply")
            import :: c_ptr, c_int
            type(c_ptr), value :: model, stream
        end function
        integer(c_int) function spd_model_breed_compute(model, dst_device, dst_bytes, stream) bind(C, name="spd_model_breed_compute")
            import :: c_ptr, c_int, c_size_t
            type(c_ptr), value :: model, dst_device, stream
            integer(c_size_t), value :: dst_bytes
        end function
        integer(c_int) function spd_model_breed_read(model, what, t0, nt, dst_device, dst_bytes, stream) &
                bind(C, name="spd_model_breed_read")
            import :: c_ptr, c_int, c_size_t
            type(c_ptr), value :: model, dst_device, stream
            integer(c_int), value :: what, t0, nt
            integer(c_size_t), value :: dst_bytes
        end function
        integer(c_int) function spd_model_breed_rows(model, rows, max_rows) bind(C, name="spd_model_breed_rows")
            import :: c_ptr, c_int, c_int32_t
            type(c_ptr), value :: model
            integer(c_int32_t), intent(out) :: rows(6, *)
            integer(c_int), value :: max_rows
        end function
        integer(c_int) function spd_model_breed_reset(model) bind(C, name="spd_model_breed_reset")
            import :: c_ptr, c_int
            type(c_ptr), value :: model
        end function
        integer(c_int) function spd_model_breed_info(model, bred, every, capacity, taken, in_loop, applied) &
                bind(C, name="spd_model_breed_info")
            import :: c_ptr, c_int, c_long_long
            type(c_ptr), value :: model
            integer(c_int), intent(out) :: bred, every, capacity, in_loop
            integer(c_long_long), intent(out) :: taken, applied
        end function
        ! orthonormalised breeding: the Gram-Schmidt cycle of the bred members that share a control (pyspeedy_amd.h:
        ! spd_model_breed_orthogonalize).  _gram: (members, members) fp64 in device memory; spd_breed_factor_host: gram and coef are
        ! row-major r x r (in Fortran: the transposes), rdiag(r)
        integer(c_int) function spd_model_breed_orthogonalize(model, on) bind(C, name="spd_model_breed_orthogonalize")
            import :: c_ptr, c_int
            type(c_ptr), value :: model
            integer(c_int), value :: on
        end function
        integer(c_int) function spd_model_breed_gram(model, dst_device, dst_bytes, stream) bind(C, name="spd_model_breed_gram")
            import :: c_ptr, c_int, c_size_t
            type(c_ptr), value :: model, dst_device, stream
            integer(c_size_t), value :: dst_bytes
        end function
        integer(c_int) function spd_breed_family_check(control, members) bind(C, name="spd_breed_family_check")
            import :: c_ptr, c_int
            type(c_ptr), value :: control
            integer(c_int), value :: members
        end function
        integer(c_int) function spd_breed_factor_host(gram, r, target, rdiag, coef, rank) bind(C, name="spd_breed_factor_host")
            import :: c_int, c_double
            real(c_double), intent(in) :: gram(*)
            integer(c_int), value :: r
            real(c_double), value :: target
            real(c_double), intent(out) :: rdiag(*), coef(*)
            integer(c_int), intent(out) :: rank
        end function
        integer(c_int) function spd_model_breed_ortho_info(model, on, families, largest) bind(C, name="spd_model_breed_ortho_info")
            import :: c_ptr, c_int
            type(c_ptr), value :: model
            integer(c_int), intent(out) :: on, families, largest
        end function
        ! assimilation: a serial ensemble square-root filter whose observations are projection-tape entries, inside the device loop
        ! (in_loop = 1) or once on the state as it stands (_apply), and the member-mixing transform for a caller's matrix
        ! (pyspeedy_amd.h: spd_model_assim_*).  weights(96, 48, n_patterns); entries as the projection tape's; mask: one
        ! integer(c_int32_t) per member (0 or 1), or c_null_ptr for spd_assim_check; yo and var (n_entries, n_rows); _read:
        ! real(c_double) (4, n_entries, nt) in device memory; _weights: (64, 64) (in Fortran: the transpose) and (r, n_entries);
        ! _transform: w is row-major r x r (in Fortran: the transpose), members 0-based; rows(6, *)
        integer(c_int) function spd_assim_check(weights, n_patterns, names, levels, patterns, n_entries, mask, members, every, &
                capacity, inflation, in_loop) bind(C, name="spd_assim_check")
            import :: c_ptr, c_int, c_double
            real(c_double), intent(in) :: weights(*)
            type(c_ptr), intent(in) :: names(*)
            integer(c_int), intent(in) :: levels(*), patterns(*)
            type(c_ptr), value :: mask
            real(c_double), value :: inflation
            integer(c_int), value :: n_patterns, n_entries, members, every, capacity, in_loop
        end function
        integer(c_int) function spd_model_assim_configure(model, weights, n_patterns, names, levels, patterns, n_entries, mask, &
                every, capacity, inflation, in_loop) bind(C, name="spd_model_assim_configure")
            import :: c_ptr, c_int, c_double
            type(c_ptr), value :: model, mask
            real(c_double), intent(in) :: weights(*)
            type(c_ptr), intent(in) :: names(*)
            integer(c_int), intent(in) :: levels(*), patterns(*)
            real(c_double), value :: inflation
            integer(c_int), value :: n_patterns, n_entries, every, capacity, in_loop
        end function
        integer(c_int) function spd_model_assim_off(model) bind(C, name="spd_model_assim_off")
            import :: c_ptr, c_int
            type(c_ptr), value :: model
        end function
        integer(c_int) function spd_model_assim_set_observations(model, steps, n_rows, yo, var, n_entries) &
                bind(C, name="spd_model_assim_set_observations")
            import :: c_ptr, c_int, c_int32_t, c_double
            type(c_ptr), value :: model
            integer(c_int32_t), intent(in) :: steps(*)
            real(c_double), intent(in) :: yo(*), var(*)
            integer(c_int), value :: n_rows, n_entries
        end function
        integer(c_int) function spd_model_assim_apply(model, stream) bind(C, name="spd_model_assim_apply")
            import :: c_ptr, c_int
            type(c_ptr), value :: model, stream
        end function
        integer(c_int) function spd_model_assim_compute(model, dst_device, dst_bytes, stream) bind(C, name="spd_model_assim_compute")
            import :: c_ptr, c_int, c_size_t
            type(c_ptr), value :: model, dst_device, stream
            integer(c_size_t), value :: dst_bytes
        end function
        integer(c_int) function spd_model_assim_transform(model, members, r, w, stream) bind(C, name="spd_model_assim_transform")
            import :: c_ptr, c_int, c_int32_t, c_double
            type(c_ptr), value :: model, stream
            integer(c_int32_t), intent(in) :: members(*)
            integer(c_int), value :: r
            real(c_double), intent(in) :: w(*)
        end function
        integer(c_int) function spd_model_assim_read(model, t0, nt, dst_device, dst_bytes, stream) bind(C, name="spd_model_assim_read")
            import :: c_ptr, c_int, c_size_t
            type(c_ptr), value :: model, dst_device, stream
            integer(c_int), value :: t0, nt
            integer(c_size_t), value :: dst_bytes
        end function
        integer(c_int) function spd_model_assim_weights(model, w_device, w_bytes, y_device, y_bytes, stream) &
                bind(C, name="spd_model_assim_weights")
            import :: c_ptr, c_int, c_size_t
            type(c_ptr), value :: model, w_device, y_device, stream
            integer(c_size_t), value :: w_bytes, y_bytes
        end function
        integer(c_int) function spd_model_assim_rows(model, rows, max_rows) bind(C, name="spd_model_assim_rows")
            import :: c_ptr, c_int, c_int32_t
            type(c_ptr), value :: model
            integer(c_int32_t), intent(out) :: rows(6, *)
            integer(c_int), value :: max_rows
        end function
        integer(c_int) function spd_model_assim_reset(model) bind(C, name="spd_model_assim_reset")
            import :: c_ptr, c_int
            type(c_ptr), value :: model
        end function
        integer(c_int) function spd_model_assim_info(model, r, n_entries, every, capacity, taken, skipped, in_loop, applied) &
                bind(C, name="spd_model_assim_info")
            import :: c_ptr, c_int, c_long_long
            type(c_ptr), value :: model
            integer(c_int), intent(out) :: r, n_entries, every, capacity, in_loop
            integer(c_long_long), intent(out) :: taken, skipped, applied
        end function
        integer(c_int) function spd_assim_weights_host(y, n_entries, r, yo, var, inflation, w_out, stats_out) &
                bind(C, name="spd_assim_weights_host")
            import :: c_int, c_double
            real(c_double), intent(in) :: y(*), yo(*), var(*)
            integer(c_int), value :: n_entries, r
            real(c_double), value :: inflation
            real(c_double), intent(out) :: w_out(*), stats_out(*)
        end function
        ! the verification tape: scores of a masked ensemble against a truth member of the same model, inside the device loop
        ! (in_loop = 1) or once on the state as it stands (_apply) (pyspeedy_amd.h: spd_model_verif_*).  weights(96, 48,
        ! n_patterns); entries as the projection tape's; mask: one integer(c_int32_t) per member (0 or 1), or c_null_ptr for
        ! spd_verif_check; truth 0-based; _read: real(c_double) (4, n_entries, 2, nt) in device memory; _hist: integer(c_int32_t)
        ! (66, n_entries, 2, nt) in device memory; rows(7, *); spd_verif_host: x(4608, r), y(4608), w(4608), out4(4), hist66(66)
        integer(c_int) function spd_verif_check(weights, n_patterns, names, levels, patterns, n_entries, mask, members, truth, every, &
                capacity, in_loop) bind(C, name="spd_verif_check")
            import :: c_ptr, c_int, c_double
            real(c_double), intent(in) :: weights(*)
            type(c_ptr), intent(in) :: names(*)
            integer(c_int), intent(in) :: levels(*), patterns(*)
            type(c_ptr), value :: mask
            integer(c_int), value :: n_patterns, n_entries, members, truth, every, capacity, in_loop
        end function
        integer(c_int) function spd_model_verif_configure(model, weights, n_patterns, names, levels, patterns, n_entries, mask, &
                truth, every, capacity, in_loop) bind(C, name="spd_model_verif_configure")
            import :: c_ptr, c_int, c_double
            type(c_ptr), value :: model, mask
            real(c_double), intent(in) :: weights(*)
            type(c_ptr), intent(in) :: names(*)
            integer(c_int), intent(in) :: levels(*), patterns(*)
            integer(c_int), value :: n_patterns, n_entries, truth, every, capacity, in_loop
        end function
        integer(c_int) function spd_model_verif_off(model) bind(C, name="spd_model_verif_off")
            import :: c_ptr, c_int
            type(c_ptr), value :: model
        end function
        integer(c_int) function spd_model_verif_reset(model) bind(C, name="spd_model_verif_reset")
            import :: c_ptr, c_int
            type(c_ptr), value :: model
        end function
        integer(c_int) function spd_model_verif_apply(model, stream) bind(C, name="spd_model_verif_apply")
            import :: c_ptr, c_int
            type(c_ptr), value :: model, stream
        end function
        integer(c_int) function spd_model_verif_compute(model, scores_device, scores_bytes, hist_device, hist_bytes, stream) &
                bind(C, name="spd_model_verif_compute")
            import :: c_ptr, c_int, c_size_t
            type(c_ptr), value :: model, scores_device, hist_device, stream
            integer(c_size_t), value :: scores_bytes, hist_bytes
        end function
        integer(c_int) function spd_model_verif_read(model, t0, nt, dst_device, dst_bytes, stream) bind(C, name="spd_model_verif_read")
            import :: c_ptr, c_int, c_size_t
            type(c_ptr), value :: model, dst_device, stream
            integer(c_int), value :: t0, nt
            integer(c_size_t), value :: dst_bytes
        end function
        integer(c_int) function spd_model_verif_hist(model, t0, nt, dst_device, dst_bytes, stream) bind(C, name="spd_model_verif_hist")
            import :: c_ptr, c_int, c_size_t
            type(c_ptr), value :: model, dst_device, stream
            integer(c_int), value :: t0, nt
            integer(c_size_t), value :: dst_bytes
        end function
        integer(c_int) function spd_model_verif_rows(model, rows, max_rows) bind(C, name="spd_model_verif_rows")
            import :: c_ptr, c_int, c_int32_t
            type(c_ptr), value :: model
            integer(c_int32_t), intent(out) :: rows(7, *)
            integer(c_int), value :: max_rows
        end function
        integer(c_int) function spd_model_verif_info(model, r, truth, n_entries, every, capacity, taken, in_loop, applied) &
                bind(C, name="spd_model_verif_info")
            import :: c_ptr, c_int, c_long_long
            type(c_ptr), value :: model
            integer(c_int), intent(out) :: r, truth, n_entries, every, capacity, in_loop
            integer(c_long_long), intent(out) :: taken, applied
        end function
        integer(c_int) function spd_verif_host(x, r, y, w, out4, hist66) bind(C, name="spd_verif_host")
            import :: c_int, c_int32_t, c_double
            real(c_double), intent(in) :: x(*), y(*), w(*)
            integer(c_int), value :: r
            real(c_double), intent(out) :: out4(4)
            integer(c_int32_t), intent(out) :: hist66(66)
        end function
        ! the quantile tape: order statistics over a masked ensemble at every grid point, inside the device loop (in_loop = 1) or
        ! once on the state as it stands (_apply) (pyspeedy_amd.h: spd_model_qtape_*).  An entry is names(k), levels(k) (0-based),
        ! ops(k): SPD_Q_MIN (0) ... SPD_Q_PROB_BELOW (4), params(k): q or a threshold; mask: one integer(c_int32_t) per member
        ! (0 or 1), or c_null_ptr for spd_qtape_check; entry 0-based; _read: real(c_double) (96, 48, nt) in device memory; _compute:
        ! (96, 48, n_entries) in device memory; rows(6, *); spd_qtape_host: x(4608, r) -> out(4608, n_entries)
        integer(c_int) function spd_qtape_check(names, levels, ops, params, n_entries, mask, members, every, capacity, in_loop) &
                bind(C, name="spd_qtape_check")
            import :: c_ptr, c_int, c_double
            type(c_ptr), intent(in) :: names(*)
            integer(c_int), intent(in) :: levels(*), ops(*)
            real(c_double), intent(in) :: params(*)
            type(c_ptr), value :: mask
            integer(c_int), value :: n_entries, members, every, capacity, in_loop
        end function
        integer(c_int) function spd_model_qtape_configure(model, names, levels, ops, params, n_entries, mask, every, capacity, &
                in_loop) bind(C, name="spd_model_qtape_configure")
            import :: c_ptr, c_int, c_double
            type(c_ptr), value :: model, mask
            type(c_ptr), intent(in) :: names(*)
            integer(c_int), intent(in) :: levels(*), ops(*)
            real(c_double), intent(in) :: params(*)
            integer(c_int), value :: n_entries, every, capacity, in_loop
        end function
        integer(c_int) function spd_model_qtape_off(model) bind(C, name="spd_model_qtape_off")
            import :: c_ptr, c_int
            type(c_ptr), value :: model
        end function
        integer(c_int) function spd_model_qtape_reset(model) bind(C, name="spd_model_qtape_reset")
            import :: c_ptr, c_int
            type(c_ptr), value :: model
        end function
        integer(c_int) function spd_model_qtape_apply(model, stream) bind(C, name="spd_model_qtape_apply")
            import :: c_ptr, c_int
            type(c_ptr), value :: model, stream
        end function
        integer(c_int) function spd_model_qtape_compute(model, dst_device, dst_bytes, stream) bind(C, name="spd_model_qtape_compute")
            import :: c_ptr, c_int, c_size_t
            type(c_ptr), value :: model, dst_device, stream
            integer(c_size_t), value :: dst_bytes
        end function
        integer(c_int) function spd_model_qtape_read(model, entry, t0, nt, dst_device, dst_bytes, stream) &
                bind(C, name="spd_model_qtape_read")
            import :: c_ptr, c_int, c_size_t
            type(c_ptr), value :: model, dst_device, stream
            integer(c_int), value :: entry, t0, nt
            integer(c_size_t), value :: dst_bytes
        end function
        integer(c_int) function spd_model_qtape_rows(model, rows, max_rows) bind(C, name="spd_model_qtape_rows")
            import :: c_ptr, c_int, c_int32_t
            type(c_ptr), value :: model
            integer(c_int32_t), intent(out) :: rows(6, *)
            integer(c_int), value :: max_rows
        end function
        integer(c_int) function spd_model_qtape_info(model, r, n_entries, every, capacity, taken, in_loop, applied) &
                bind(C, name="spd_model_qtape_info")
            import :: c_ptr, c_int, c_long_long
            type(c_ptr), value :: model
            integer(c_int), intent(out) :: r, n_entries, every, capacity, in_loop
            integer(c_long_long), intent(out) :: taken, applied
        end function
        integer(c_int) function spd_qtape_host(x, r, ops, params, n_entries, out) bind(C, name="spd_qtape_host")
            import :: c_int, c_double
            real(c_double), intent(in) :: x(*), params(*)
            integer(c_int), intent(in) :: ops(*)
            integer(c_int), value :: r, n_entries
            real(c_double), intent(out) :: out(*)
        end function
        ! spectra by total wavenumber and global means of the spectral state, recorded inside spd_model_step calls or computed on
        ! the state as it stands (pyspeedy_amd.h: spd_model_spectra_*).  fp64; rows as the tape's; _read: (32[, 8], nt, count) for
        ! a spectrum, ([8, ]nt, count) for a mean; _compute: (..., count) per name, one name after the other
        integer(c_int) function spd_model_spectra_configure(model, names, n_names, every, capacity) &
                bind(C, name="spd_model_spectra_configure")
            import :: c_ptr, c_int
            type(c_ptr), value :: model
            type(c_ptr), intent(in) :: names(*)
            integer(c_int), value :: n_names, every, capacity
        end function
        integer(c_int) function spd_model_spectra_reset(model) bind(C, name="spd_model_spectra_reset")
            import :: c_ptr, c_int
            type(c_ptr), value :: model
        end function
        integer(c_int) function spd_model_spectra_info(model, taken, held, capacity, every) bind(C, name="spd_model_spectra_info")
            import :: c_ptr, c_int, c_long_long
            type(c_ptr), value :: model
            integer(c_long_long), intent(out) :: taken
            integer(c_int), intent(out) :: held, capacity, every
        end function
        integer(c_int) function spd_model_spectra_times(model, rows, max_rows) bind(C, name="spd_model_spectra_times")
            import :: c_ptr, c_int, c_int32_t
            type(c_ptr), value :: model
            integer(c_int32_t), intent(out) :: rows(6, *)
            integer(c_int), value :: max_rows
        end function
        integer(c_int) function spd_model_spectra_read(model, name, first, count, t0, nt, dst_device, dst_bytes, stream) &
                bind(C, name="spd_model_spectra_read")
            import :: c_ptr, c_int, c_char, c_size_t
            type(c_ptr), value :: model, dst_device, stream
            character(kind=c_char), intent(in) :: name(*)
            integer(c_int), value :: first, count, t0, nt
            integer(c_size_t), value :: dst_bytes
        end function
        integer(c_int) function spd_model_spectra_compute(model, names, n_names, first, count, dst_device, dst_bytes, stream) &
                bind(C, name="spd_model_spectra_compute")
            import :: c_ptr, c_int, c_size_t
            type(c_ptr), value :: model, dst_device, stream
            type(c_ptr), intent(in) :: names(*)
            integer(c_int), value :: n_names, first, count
            integer(c_size_t), value :: dst_bytes
        end function
        integer(c_int) function spd_model_current_step(model) bind(C, name="spd_model_current_step")
            import :: c_ptr, c_int
            type(c_ptr), value :: model
        end function
        integer(c_int) function spd_model_set_flags(model, land_coupling, sst_anomaly_coupling, increase_co2) &
                bind(C, name="spd_model_set_flags")
            import :: c_ptr, c_int
            type(c_ptr), value :: model
            integer(c_int), value :: land_coupling, sst_anomaly_coupling, increase_co2
        end function
        ! cfg 5: fp32 /= 0 runs the arithmetic of the column physics in single precision (state and dynamics stay fp64)
        integer(c_int) function spd_model_set_physics_precision(model, fp32) bind(C, name="spd_model_set_physics_precision")
            import :: c_ptr, c_int
            type(c_ptr), value :: model
            integer(c_int), value :: fp32
        end function
        ! launch-plan switches by name ("diag_every_step", "spectral_early", "split_dyn"); name is
        ! a C string: pass "diag_every_step"//c_null_char
        integer(c_int) function spd_model_set_option(model, name, value) bind(C, name="spd_model_set_option")
            import :: c_ptr, c_int, c_char, c_int32_t
            type(c_ptr), value :: model
            character(kind=c_char), intent(in) :: name(*)
            integer(c_int32_t), value :: value
        end function
        integer(c_int) function spd_model_set_sppt(model, on, seed, first_member_id) bind(C, name="spd_model_set_sppt")
            import :: c_ptr, c_int, c_int64_t
            type(c_ptr), value :: model
            integer(c_int), value :: on
            integer(c_int64_t), value :: seed, first_member_id
        end function

        ! ---- outer boundary with the reference's own procedures (include/pyspeedy_amd_driver.h) -----------------------
        ! registry/templates/speedy_driver.f90.j2: modelstate_init :216, modelstate_init_sst_anom :225, modelstate_close :240,
        ! create_datetime :163, get_datetime :189, close_datetime :203, controlparams_init :131, controlparams_close :151,
        ! init :29, step :43, parallel_step :58, check :81, transform_* :94-125, get_<v> / set_<v> / get_<v>_shape :250-334
        integer(c_int) function spd_modelstate_init(state_cnt) bind(C, name="spd_modelstate_init")
            import :: c_int, c_int64_t
            integer(c_int64_t), intent(out) :: state_cnt
        end function
        integer(c_int) function spd_modelstate_init_sst_anom(state_cnt, n_months) bind(C, name="spd_modelstate_init_sst_anom")
            import :: c_int, c_int64_t, c_int32_t
            integer(c_int64_t), value :: state_cnt
            integer(c_int32_t), value :: n_months
        end function
        integer(c_int) function spd_modelstate_close(state_cnt) bind(C, name="spd_modelstate_close")
            import :: c_int, c_int64_t
            integer(c_int64_t), value :: state_cnt
        end function
        integer(c_int) function spd_create_datetime(year, month, day, hour, minute, datetime_cnt) &
                bind(C, name="spd_create_datetime")
            import :: c_int, c_int64_t, c_int32_t
            integer(c_int32_t), value :: year, month, day, hour, minute
            integer(c_int64_t), intent(out) :: datetime_cnt
        end function
        integer(c_int) function spd_get_datetime(datetime_cnt, year, month, day, hour, minute) bind(C, name="spd_get_datetime")
            import :: c_int, c_int64_t, c_int32_t
            integer(c_int64_t), value :: datetime_cnt
            integer(c_int32_t), intent(out) :: year, month, day, hour, minute
        end function
        integer(c_int) function spd_close_datetime(datetime_cnt) bind(C, name="spd_close_datetime")
            import :: c_int, c_int64_t
            integer(c_int64_t), value :: datetime_cnt
        end function
        integer(c_int) function spd_controlparams_init(control_cnt, start_datetime_cnt, end_datetime_cnt) &
                bind(C, name="spd_controlparams_init")
            import :: c_int, c_int64_t
            integer(c_int64_t), intent(out) :: control_cnt
            integer(c_int64_t), value :: start_datetime_cnt, end_datetime_cnt
        end function
        integer(c_int) function spd_controlparams_close(control_cnt) bind(C, name="spd_controlparams_close")
            import :: c_int, c_int64_t
            integer(c_int64_t), value :: control_cnt
        end function
        integer(c_int) function spd_init(state_cnt, control_cnt, error_code) bind(C, name="spd_init")
            import :: c_int, c_int64_t, c_int32_t
            integer(c_int64_t), value :: state_cnt, control_cnt
            integer(c_int32_t), intent(out) :: error_code
        end function
        integer(c_int) function spd_step(state_cnt, control_cnt, error_code) bind(C, name="spd_step")
            import :: c_int, c_int64_t, c_int32_t
            integer(c_int64_t), value :: state_cnt, control_cnt
            integer(c_int32_t), intent(out) :: error_code
        end function
        integer(c_int) function spd_parallel_step(state_cnts, control_cnts, error_codes, n_members) &
                bind(C, name="spd_parallel_step")
            import :: c_int, c_int64_t, c_int32_t
            integer(c_int64_t), intent(in) :: state_cnts(*), control_cnts(*)
            integer(c_int32_t), intent(out) :: error_codes(*)
            integer(c_int32_t), value :: n_members
        end function
        ! extension: the same step with its range check overlapped with the next step
        integer(c_int) function spd_parallel_step_begin(state_cnts, control_cnts, n_members, token) &
                bind(C, name="spd_parallel_step_begin")
            import :: c_int, c_int64_t, c_int32_t
            integer(c_int64_t), intent(in) :: state_cnts(*), control_cnts(*)
            integer(c_int32_t), value :: n_members
            integer(c_int64_t), intent(out) :: token
        end function
        integer(c_int) function spd_parallel_step_end(token, error_codes) bind(C, name="spd_parallel_step_end")
            import :: c_int, c_int64_t, c_int32_t
            integer(c_int64_t), value :: token
            integer(c_int32_t), intent(out) :: error_codes(*)
        end function
        ! extension: n_steps steps as ONE call, the range check of every step recorded on the device (the stretch of a time loop in
        ! which nothing looks at the state); steps_done: the steps a member completed before its first failing one
        integer(c_int) function spd_parallel_steps_begin(state_cnts, control_cnts, n_members, n_steps, token) &
                bind(C, name="spd_parallel_steps_begin")
            import :: c_int, c_int64_t, c_int32_t
            integer(c_int64_t), intent(in) :: state_cnts(*), control_cnts(*)
            integer(c_int32_t), value :: n_members, n_steps
            integer(c_int64_t), intent(out) :: token
        end function
        integer(c_int) function spd_parallel_steps_end(token, error_codes, steps_done) bind(C, name="spd_parallel_steps_end")
            import :: c_int, c_int64_t, c_int32_t
            integer(c_int64_t), value :: token
            integer(c_int32_t), intent(out) :: error_codes(*), steps_done(*)
        end function
        integer(c_int) function spd_check(state_cnt, error_code) bind(C, name="spd_check")
            import :: c_int, c_int64_t, c_int32_t
            integer(c_int64_t), value :: state_cnt
            integer(c_int32_t), intent(out) :: error_code
        end function
        integer(c_int) function spd_transform_spectral2grid(state_cnt) bind(C, name="spd_transform_spectral2grid")
            import :: c_int, c_int64_t
            integer(c_int64_t), value :: state_cnt
        end function
        integer(c_int) function spd_transform_grid2spectral(state_cnt) bind(C, name="spd_transform_grid2spectral")
            import :: c_int, c_int64_t
            integer(c_int64_t), value :: state_cnt
        end function
        integer(c_int) function spd_apply_grid_filter(state_cnt) bind(C, name="spd_apply_grid_filter")
            import :: c_int, c_int64_t
            integer(c_int64_t), value :: state_cnt
        end function
        integer(c_int) function spd_get(state_cnt, name, buf, bytes) bind(C, name="spd_get")
            import :: c_int, c_int64_t, c_char, c_size_t
            integer(c_int64_t), value :: state_cnt
            character(kind=c_char), intent(in) :: name(*)
            type(*) :: buf(*)
            integer(c_size_t), value :: bytes
        end function
        integer(c_int) function spd_set(state_cnt, name, buf, bytes) bind(C, name="spd_set")
            import :: c_int, c_int64_t, c_char, c_size_t
            integer(c_int64_t), value :: state_cnt
            character(kind=c_char), intent(in) :: name(*)
            type(*), intent(in) :: buf(*)
            integer(c_size_t), value :: bytes
        end function
        integer(c_int) function spd_get_shape(state_cnt, name, array_shape, ndim) bind(C, name="spd_get_shape")
            import :: c_int, c_int64_t, c_char, c_int32_t
            integer(c_int64_t), value :: state_cnt
            character(kind=c_char), intent(in) :: name(*)
            integer(c_int32_t), intent(out) :: array_shape(5), ndim
        end function
        integer(c_int) function spd_driver_model(state_cnt, model, member, members_in_model) bind(C, name="spd_driver_model")
            import :: c_int, c_int64_t, c_int32_t, c_ptr
            integer(c_int64_t), value :: state_cnt
            type(c_ptr), intent(out) :: model          ! spd_model_handle owned by the driver
            integer(c_int32_t), intent(out) :: member, members_in_model
        end function
        integer(c_int) function spd_modelstate_init_ensemble(state_cnts, n_members) bind(C, name="spd_modelstate_init_ensemble")
            import :: c_int, c_int64_t, c_int32_t
            integer(c_int64_t), intent(out) :: state_cnts(*)
            integer(c_int32_t), value :: n_members
        end function
        integer(c_int) function spd_modelstate_init_ensemble_on(state_cnts, n_members, n_devices) &
                bind(C, name="spd_modelstate_init_ensemble_on")
            import :: c_int, c_int64_t, c_int32_t
            integer(c_int64_t), intent(out) :: state_cnts(*)
            integer(c_int32_t), value :: n_members, n_devices   ! n_devices 0: the current device; k: blocks on devices 0 .. k-1
        end function
        integer(c_int) function spd_modelstate_init_ensemble_whole(state_cnts, n_members, n_devices) &
                bind(C, name="spd_modelstate_init_ensemble_whole")
            import :: c_int, c_int64_t, c_int32_t
            integer(c_int64_t), intent(out) :: state_cnts(*)
            integer(c_int32_t), value :: n_members, n_devices   ! ONE device model per device; n_devices < 0: the process-wide placement
        end function
        integer(c_int) function spd_driver_stats(state_cnt, models_alive, members_in_model) bind(C, name="spd_driver_stats")
            import :: c_int, c_int64_t, c_int32_t
            integer(c_int64_t), value :: state_cnt
            integer(c_int32_t), intent(out) :: models_alive, members_in_model
        end function
        ! ---- one process, several GPUs (extension; the reference's ensemble is one process, speedy_driver.f90.j2:58-79) ----
        integer(c_int) function spd_device_count(n_devices) bind(C, name="spd_device_count")
            import :: c_int, c_int32_t
            integer(c_int32_t), intent(out) :: n_devices
        end function
        integer(c_int) function spd_set_device_placement(n_devices) bind(C, name="spd_set_device_placement")
            import :: c_int, c_int32_t
            integer(c_int32_t), value :: n_devices   ! 0: current device; k: containers spread over devices 0 .. k-1
        end function
        integer(c_int) function spd_modelstate_init_on(state_cnt, device) bind(C, name="spd_modelstate_init_on")
            import :: c_int, c_int64_t, c_int32_t
            integer(c_int64_t), intent(out) :: state_cnt
            integer(c_int32_t), value :: device
        end function
        integer(c_int) function spd_modelstate_device(state_cnt, device) bind(C, name="spd_modelstate_device")
            import :: c_int, c_int64_t, c_int32_t
            integer(c_int64_t), value :: state_cnt
            integer(c_int32_t), intent(out) :: device
        end function
        integer(c_int) function spd_broadcast_boundary(state_cnts, n, root) bind(C, name="spd_broadcast_boundary")
            import :: c_int, c_int64_t, c_int32_t
            integer(c_int64_t), intent(in) :: state_cnts(*)
            integer(c_int32_t), value :: n, root     ! root: 0-based index into state_cnts
        end function
        integer(c_int) function spd_broadcast_boundary_stats(peer_copies, local_copies, collective_devices) &
                bind(C, name="spd_broadcast_boundary_stats")
            import :: c_int, c_int32_t
            integer(c_int32_t), intent(out) :: peer_copies, local_copies, collective_devices
        end function
        function spd_broadcast_boundary_note() bind(C, name="spd_broadcast_boundary_note") result(text)
            import :: c_ptr
            type(c_ptr) :: text   ! NUL-terminated, valid until this thread's next call
        end function
    end interface
end module pyspeedy_amd_c
