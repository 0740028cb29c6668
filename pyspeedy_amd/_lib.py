"""ctypes binding of the C ABI declared in include/pyspeedy_amd.h.

The HIP library is the product: if it is missing or cannot be loaded this module raises -- there is no
CPU fallback (the CPU oracle under oracle/ is test infrastructure and is never imported from here).
"""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
# PYSPEEDY_AMD_LIB: another build of the same library (A/B measurements of kernel variants in one session)
LIB_PATH = os.environ.get("PYSPEEDY_AMD_LIB") or os.path.join(_HERE, "libpyspeedy_amd.so")
CSRC = os.path.join(_HERE, "csrc")

IX, IL, IY, KX, MX, NX, TRUNC = 96, 48, 24, 8, 31, 32, 30
NSPEC, NFOUR, NGRID = MX * NX, 2 * MX * IL, IX * IL

SPD_OK, SPD_E_ARG, SPD_E_DEVICE, SPD_E_SIZE = 0, -1, -2, -3
SPD_STATS_MEAN, SPD_STATS_VARIANCE, SPD_STATS_STD = 0, 1, 2  # kinds of spd_model_stats_read / _ensemble
SPD_TAPE_F32, SPD_TAPE_F64 = 0, 1  # storage of spd_model_tape_configure
SPD_ENS_MEAN, SPD_ENS_STD, SPD_ENS_M2 = 0, 1, 2  # kinds of spd_model_enstape_read
SPD_ACC_SUM, SPD_ACC_MEAN, SPD_ACC_MIN, SPD_ACC_MAX = 0, 1, 2, 3  # ops of spd_model_acctape_configure / _read
SPD_WIN_SUM, SPD_WIN_MEAN, SPD_WIN_MIN, SPD_WIN_MAX, SPD_WIN_COUNT_ABOVE, SPD_WIN_COUNT_BELOW = 0, 1, 2, 3, 4, 5  # ops of spd_model_wintape_*
SPD_WINDOW_STEPS, SPD_WINDOW_DAY, SPD_WINDOW_MONTH = 0, 1, 2  # window kinds of spd_model_wintape_configure / spd_wintape_plan
SPD_Q_MIN, SPD_Q_MAX, SPD_Q_QUANTILE, SPD_Q_PROB_ABOVE, SPD_Q_PROB_BELOW = 0, 1, 2, 3, 4  # ops of spd_model_qtape_configure
SPD_TRACK_MIN, SPD_TRACK_MAX = 0, 1  # ops of spd_model_tracktape_configure
SPD_FIL_MEAN, SPD_FIL_COV, SPD_FIL_LAST = 0, 1, 2  # ops of spd_model_filtape_configure


class SpeedyHipError(RuntimeError):
    pass


def build(verbose=False):
    """Compile every HIP source for gfx950 into pyspeedy_amd/libpyspeedy_amd.so (hipcc cross-compiles)."""
    cmd = ["make", "-C", CSRC, "-j4"]
    if not verbose:
        cmd.insert(1, "-s")
    subprocess.run(cmd, check=True)
    if not os.path.isfile(LIB_PATH):
        raise SpeedyHipError("build did not produce " + LIB_PATH)


_PHYS_PTR_FIELDS = [
    "ug", "vg", "tg", "qg", "phig", "pslg", "utend", "vtend", "ttend", "qtend",
    "fmask_land", "phis0", "forog", "sst_am", "alb_land", "alb_sea", "snowc", "land_temp", "soil_avail_water",
    "flux_solar_in", "flux_ozone_upper", "flux_ozone_lower", "zenit_correction", "stratospheric_correction",
    "alb_surface",
    "precnv", "precls", "cbmf", "slrd", "slr", "olr",
    "slru", "ustr", "vstr", "shf", "evap", "hfluxn", "rad_st4a", "rad_flux",
    "tt_rsw", "rad_tau2", "rad_strat_corr", "tsr", "ssrd", "ssr", "qcloud_equiv",
    "iptop", "icltop", "ts", "tskin", "u0", "v0", "t0", "cloudc", "clstr",
]


class PhysicsArgs(C.Structure):
    """Mirror of spd_physics_args (include/pyspeedy_amd.h)."""
    _fields_ = [(n, C.c_void_p) for n in _PHYS_PTR_FIELDS] + [
        ("air_absortivity_co2", C.c_double), ("compute_shortwave", C.c_int32), ("fp32", C.c_int32),
        ("sppt_pattern", C.c_void_p)]


class ModelControl(C.Structure):
    """Mirror of spd_model_control (include/pyspeedy_amd.h)."""
    _fields_ = [(n, C.c_int32) for n in (
        "current_step", "year", "month", "day", "hour", "minute", "month_idx", "land_coupling_flag",
        "sst_anomaly_coupling_flag", "increase_co2", "sppt_on", "sppt_first", "physics_fp32", "reserved")] + [
        ("sppt_step", C.c_int64), ("sppt_first_member_id", C.c_int64), ("sppt_seed", C.c_uint64),
        ("air_absortivity_co2", C.c_double), ("ablco2_ref", C.c_double)]


class StreamProbeArgs(C.Structure):
    """Mirror of spd_stream_probe_args (include/pyspeedy_amd.h)."""
    _fields_ = [(n, C.c_int32) for n in (
        "reads", "writes", "lane_bytes", "in_flight", "nontemporal", "waves_per_simd", "rows_per_wave", "reps", "layout",
        "reserved")] + [
        ("total_bytes", C.c_uint64)]


# sections, n_sections, n_filters, names_a, levels_a, filters, ops, names_b, levels_b, n_entries, window, every, sample_every, spinup,
# capacity, dtype of spd_model_filtape_configure / spd_filtape_check
_FILTAPE_ARGS = ([C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_char_p)] + [C.POINTER(C.c_int)] * 3 +
                 [C.POINTER(C.c_char_p), C.POINTER(C.c_int)] + [C.c_int] * 7)

_SIGNATURES = {
    "spd_stream_probe": (C.c_int, [C.c_void_p, C.POINTER(StreamProbeArgs), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                   C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "spd_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int]),
    "spd_destroy": (C.c_int, [C.c_void_p]),
    "spd_device": (C.c_int, [C.c_void_p]),
    "spd_last_error": (C.c_char_p, []),
    "spd_version": (C.c_char_p, []),
    "spd_get_table_host": (C.c_long, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_size_t]),
    "spd_calendar_walk": (C.c_int, [C.c_int] * 6 + [C.c_void_p] * 5),
    "spd_daily_forcing_host": (C.c_int, [C.c_double, C.c_void_p]),
    "spd_spec2grid": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "spd_grid2spec": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "spd_legendre_inv": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "spd_legendre": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "spd_fourier_inv": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "spd_fourier": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "spd_vort2vel": (C.c_int, [C.c_void_p] + [C.c_void_p] * 4 + [C.c_int, C.c_void_p]),
    "spd_vel2vort": (C.c_int, [C.c_void_p] + [C.c_void_p] * 4 + [C.c_int, C.c_void_p]),
    "spd_grid_vel2vort": (C.c_int, [C.c_void_p] + [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_void_p]),
    "spd_gradient": (C.c_int, [C.c_void_p] + [C.c_void_p] * 3 + [C.c_int, C.c_void_p]),
    "spd_laplacian": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "spd_truncate": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "spd_grid_filter": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "spd_physics": (C.c_int, [C.c_void_p, C.POINTER(PhysicsArgs), C.c_int, C.c_void_p]),
    "spd_model_create": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    "spd_model_destroy": (C.c_int, [C.c_void_p]),
    "spd_model_members": (C.c_int, [C.c_void_p]),
    "spd_model_memory": (C.c_int, [C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "spd_model_var_bytes": (C.c_long, [C.c_void_p, C.c_char_p]),
    "spd_model_var_storage": (C.c_int, [C.c_void_p, C.c_char_p]),
    "spd_model_set": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int, C.c_void_p, C.c_size_t]),
    "spd_model_get": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int, C.c_void_p, C.c_size_t]),
    "spd_model_device_ptr": (C.c_void_p, [C.c_void_p, C.c_char_p]),
    "spd_model_invalidate": (C.c_int, [C.c_void_p]),
    "spd_model_checks_in_flight": (C.c_int, [C.c_void_p]),
    "spd_model_set_co2": (C.c_int, [C.c_void_p, C.c_double]),
    "spd_model_co2": (C.c_double, [C.c_void_p]),
    "spd_model_set_time_step": (C.c_int, [C.c_void_p, C.c_double]),
    "spd_model_step_dynamics": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_int, C.c_void_p]),
    "spd_model_check": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "spd_model_check_begin": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "spd_model_check_end": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "spd_model_check_defer": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "spd_model_check_settle": (C.c_int, [C.c_void_p, C.c_int]),
    "spd_model_check_counts": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "spd_model_init": (C.c_int, [C.c_void_p] + [C.c_int] * 5 + [C.c_void_p]),
    "spd_model_step": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "spd_model_current_step": (C.c_int, [C.c_void_p]),
    "spd_model_get_date": (C.c_int, [C.c_void_p, C.c_void_p]),
    "spd_model_mark_initialized": (C.c_int, [C.c_void_p] + [C.c_int] * 6),
    "spd_model_get_control": (C.c_int, [C.c_void_p, C.POINTER(ModelControl)]),
    "spd_model_set_control": (C.c_int, [C.c_void_p, C.POINTER(ModelControl)]),
    "spd_model_set_flags": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "spd_model_spectral2grid": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "spd_model_grid2spectral": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "spd_model_grid_filter": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "spd_model_export_pack": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "spd_model_init_sst_anom": (C.c_int, [C.c_void_p, C.c_int]),
    "spd_model_set_sppt": (C.c_int, [C.c_void_p, C.c_int, C.c_uint64, C.c_int64]),
    "spd_model_copy_member": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "spd_model_stats_configure": (C.c_int, [C.c_void_p, C.POINTER(C.c_char_p), C.c_int, C.c_int, C.c_int]),
    "spd_model_stats_reset": (C.c_int, [C.c_void_p]),
    "spd_model_stats_samples": (C.c_int, [C.c_void_p]),
    "spd_model_stats_read": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "spd_model_stats_ensemble": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "spd_model_tape_configure": (C.c_int, [C.c_void_p, C.POINTER(C.c_char_p), C.c_int, C.c_int, C.c_int, C.c_int]),
    "spd_model_tape_reset": (C.c_int, [C.c_void_p]),
    "spd_model_tape_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_longlong)] + [C.POINTER(C.c_int)] * 4),
    "spd_model_tape_times": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_int]),
    "spd_model_tape_read": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "spd_model_enstape_configure": (C.c_int, [C.c_void_p, C.POINTER(C.c_char_p), C.c_int, C.c_int, C.c_int]),
    "spd_model_enstape_reset": (C.c_int, [C.c_void_p]),
    "spd_model_enstape_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_longlong)] + [C.POINTER(C.c_int)] * 4),
    "spd_model_enstape_times": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_int]),
    "spd_model_enstape_read": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "spd_model_acctape_configure": (C.c_int, [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int, C.c_int]),
    "spd_model_acctape_reset": (C.c_int, [C.c_void_p]),
    "spd_model_acctape_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_longlong)] + [C.POINTER(C.c_int)] * 4),
    "spd_model_acctape_times": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_int]),
    "spd_model_acctape_read": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t,
                                         C.c_void_p]),
    "spd_model_wintape_configure": (C.c_int, [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_int), C.POINTER(C.c_double), C.c_int, C.c_int,
                                              C.c_int, C.c_int, C.c_int, C.c_int]),
    "spd_model_wintape_reset": (C.c_int, [C.c_void_p]),
    "spd_model_wintape_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_longlong)] + [C.POINTER(C.c_int)] * 6),
    "spd_model_wintape_times": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_int]),
    "spd_model_wintape_read": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t,
                                         C.c_void_p]),
    "spd_wintape_plan": (C.c_int, [C.c_int] * 10 + [C.POINTER(C.c_int32), C.c_int]),
    "spd_model_projtape_configure": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int),
                                               C.POINTER(C.c_int), C.c_int, C.c_int, C.c_int]),
    "spd_model_projtape_reset": (C.c_int, [C.c_void_p]),
    "spd_model_projtape_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_longlong)] + [C.POINTER(C.c_int)] * 5),
    "spd_model_projtape_times": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_int]),
    "spd_model_projtape_read": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "spd_model_tracktape_configure": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_char_p)] + [C.POINTER(C.c_int)] * 4 +
                                      [C.c_int, C.c_int, C.c_int]),
    "spd_model_tracktape_reset": (C.c_int, [C.c_void_p]),
    "spd_model_tracktape_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_longlong)] + [C.POINTER(C.c_int)] * 5),
    "spd_model_tracktape_times": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_int]),
    "spd_model_tracktape_read": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "spd_model_tracktape_positions": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_int]),
    "spd_model_tracktape_seed": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int32)]),
    "spd_track_point_host": (C.c_int, [C.POINTER(C.c_double), C.POINTER(C.c_ubyte), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]),
    "spd_model_filtape_configure": (C.c_int, [C.c_void_p] + _FILTAPE_ARGS),
    "spd_model_filtape_off": (C.c_int, [C.c_void_p]),
    "spd_model_filtape_reset": (C.c_int, [C.c_void_p]),
    "spd_model_filtape_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_longlong)] + [C.POINTER(C.c_int)] * 10 + [C.POINTER(C.c_longlong)]),
    "spd_model_filtape_times": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_int]),
    "spd_model_filtape_read": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "spd_filtape_check": (C.c_int, _FILTAPE_ARGS),
    "spd_filtape_filter_host": (C.c_int, [C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double)]),
    "spd_model_nudge_configure": (C.c_int, [C.c_void_p, C.POINTER(C.c_char_p), C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int32), C.c_int,
                                            C.c_int]),
    "spd_model_nudge_set_times": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_int]),
    "spd_model_nudge_set_target": (C.c_int, [C.c_void_p, C.c_int, C.c_char_p, C.c_void_p, C.c_size_t]),
    "spd_model_nudge_apply": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "spd_model_nudge_info": (C.c_int, [C.c_void_p] + [C.POINTER(C.c_int)] * 4 + [C.POINTER(C.c_longlong)]),
    "spd_breed_check": (C.c_int, [C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_double), C.c_double, C.c_int, C.c_int, C.c_int]),
    "spd_model_breed_configure": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.c_double, C.c_int, C.c_int, C.c_int]),
    "spd_model_breed_apply": (C.c_int, [C.c_void_p, C.c_void_p]),
    "spd_model_breed_compute": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "spd_model_breed_read": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "spd_model_breed_rows": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_int]),
    "spd_model_breed_reset": (C.c_int, [C.c_void_p]),
    "spd_model_breed_info": (C.c_int, [C.c_void_p] + [C.POINTER(C.c_int)] * 3 + [C.POINTER(C.c_longlong), C.POINTER(C.c_int), C.POINTER(C.c_longlong)]),
    "spd_model_breed_orthogonalize": (C.c_int, [C.c_void_p, C.c_int]),
    "spd_model_breed_gram": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "spd_breed_family_check": (C.c_int, [C.POINTER(C.c_int32), C.c_int]),
    "spd_breed_factor_host": (C.c_int, [C.POINTER(C.c_double), C.c_int, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    "spd_model_breed_ortho_info": (C.c_int, [C.c_void_p] + [C.POINTER(C.c_int)] * 3),
    "spd_assim_check": (C.c_int, [C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int,
                                  C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int, C.c_double, C.c_int]),
    "spd_model_assim_configure": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int),
                                            C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_double, C.c_int]),
    "spd_model_assim_off": (C.c_int, [C.c_void_p]),
    "spd_model_assim_set_observations": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                                   C.c_int]),
    "spd_model_assim_apply": (C.c_int, [C.c_void_p, C.c_void_p]),
    "spd_model_assim_compute": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "spd_model_assim_transform": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_double), C.c_void_p]),
    "spd_model_assim_read": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "spd_model_assim_weights": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]),
    "spd_model_assim_rows": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_int]),
    "spd_model_assim_reset": (C.c_int, [C.c_void_p]),
    "spd_model_assim_info": (C.c_int, [C.c_void_p] + [C.POINTER(C.c_int)] * 4 + [C.POINTER(C.c_longlong)] * 2 + [C.POINTER(C.c_int),
                                                                                                                  C.POINTER(C.c_longlong)]),
    "spd_assim_weights_host": (C.c_int, [C.POINTER(C.c_double), C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double,
                                         C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "spd_verif_check": (C.c_int, [C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int,
                                  C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "spd_model_verif_configure": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int),
                                            C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int, C.c_int]),
    "spd_model_verif_off": (C.c_int, [C.c_void_p]),
    "spd_model_verif_reset": (C.c_int, [C.c_void_p]),
    "spd_model_verif_apply": (C.c_int, [C.c_void_p, C.c_void_p]),
    "spd_model_verif_compute": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]),
    "spd_model_verif_read": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "spd_model_verif_hist": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "spd_model_verif_rows": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_int]),
    "spd_model_verif_info": (C.c_int, [C.c_void_p] + [C.POINTER(C.c_int)] * 5 + [C.POINTER(C.c_longlong), C.POINTER(C.c_int),
                                                                                 C.POINTER(C.c_longlong)]),
    "spd_verif_host": (C.c_int, [C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                 C.POINTER(C.c_int32)]),
    "spd_qtape_check": (C.c_int, [C.POINTER(C.c_char_p), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double), C.c_int,
                                  C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int, C.c_int]),
    "spd_model_qtape_configure": (C.c_int, [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double),
                                            C.c_int, C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int]),
    "spd_model_qtape_off": (C.c_int, [C.c_void_p]),
    "spd_model_qtape_reset": (C.c_int, [C.c_void_p]),
    "spd_model_qtape_apply": (C.c_int, [C.c_void_p, C.c_void_p]),
    "spd_model_qtape_compute": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "spd_model_qtape_read": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "spd_model_qtape_rows": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_int]),
    "spd_model_qtape_info": (C.c_int, [C.c_void_p] + [C.POINTER(C.c_int)] * 4 + [C.POINTER(C.c_longlong), C.POINTER(C.c_int),
                                                                                 C.POINTER(C.c_longlong)]),
    "spd_qtape_host": (C.c_int, [C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double)]),
    "spd_model_spectra_configure": (C.c_int, [C.c_void_p, C.POINTER(C.c_char_p), C.c_int, C.c_int, C.c_int]),
    "spd_model_spectra_reset": (C.c_int, [C.c_void_p]),
    "spd_model_spectra_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_longlong)] + [C.POINTER(C.c_int)] * 3),
    "spd_model_spectra_times": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_int]),
    "spd_model_spectra_read": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "spd_model_spectra_compute": (C.c_int, [C.c_void_p, C.POINTER(C.c_char_p), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "spd_model_plev_configure": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.c_int]),
    "spd_model_plev_levels": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.c_int]),
    "spd_model_plev_compute": (C.c_int, [C.c_void_p, C.POINTER(C.c_char_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "spd_model_plev_read": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "spd_model_derive_compute": (C.c_int, [C.c_void_p, C.POINTER(C.c_char_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "spd_model_derive_read": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    # outer boundary (include/pyspeedy_amd_driver.h): the procedures of speedy_driver.f90.j2
    "spd_modelstate_init": (C.c_int, [C.POINTER(C.c_int64)]),
    "spd_modelstate_init_ensemble": (C.c_int, [C.POINTER(C.c_int64), C.c_int32]),
    "spd_modelstate_init_sst_anom": (C.c_int, [C.c_int64, C.c_int32]),
    "spd_device_count": (C.c_int, [C.POINTER(C.c_int32)]),
    "spd_set_device_placement": (C.c_int, [C.c_int32]),
    "spd_modelstate_init_on": (C.c_int, [C.POINTER(C.c_int64), C.c_int32]),
    "spd_modelstate_device": (C.c_int, [C.c_int64, C.POINTER(C.c_int32)]),
    "spd_broadcast_boundary": (C.c_int, [C.POINTER(C.c_int64), C.c_int32, C.c_int32]),
    "spd_driver_trace": (C.c_int, [C.c_int32]),
    "spd_driver_trace_read": (C.c_int, [C.POINTER(C.c_int32), C.c_int32]),
    "spd_model_copy_vars": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.c_int, C.c_void_p]),
    "spd_model_copy_vars_enqueue": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.c_int, C.c_void_p]),
    "spd_model_broadcast_vars": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(C.c_char_p), C.c_int]),
    "spd_modelstate_init_ensemble_on": (C.c_int, [C.POINTER(C.c_int64), C.c_int32, C.c_int32]),
    "spd_broadcast_boundary_stats": (C.c_int, [C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "spd_broadcast_boundary_note": (C.c_char_p, []),
    "spd_modelstate_close": (C.c_int, [C.c_int64]),
    "spd_create_datetime": (C.c_int, [C.c_int32] * 5 + [C.POINTER(C.c_int64)]),
    "spd_get_datetime": (C.c_int, [C.c_int64] + [C.POINTER(C.c_int32)] * 5),
    "spd_close_datetime": (C.c_int, [C.c_int64]),
    "spd_controlparams_init": (C.c_int, [C.POINTER(C.c_int64), C.c_int64, C.c_int64]),
    "spd_controlparams_close": (C.c_int, [C.c_int64]),
    "spd_controlparams_get_model_datetime": (C.c_int, [C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "spd_init": (C.c_int, [C.c_int64, C.c_int64, C.POINTER(C.c_int32)]),
    "spd_init_ensemble": (C.c_int, [C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.c_int32]),
    "spd_step": (C.c_int, [C.c_int64, C.c_int64, C.POINTER(C.c_int32)]),
    "spd_parallel_step": (C.c_int, [C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.c_int32]),
    "spd_parallel_step_begin": (C.c_int, [C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int32, C.POINTER(C.c_int64)]),
    "spd_parallel_step_end": (C.c_int, [C.c_int64, C.POINTER(C.c_int32)]),
    "spd_modelstate_init_ensemble_whole": (C.c_int, [C.POINTER(C.c_int64), C.c_int32, C.c_int32]),
    "spd_parallel_steps_begin": (C.c_int, [C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int32, C.c_int32, C.POINTER(C.c_int64)]),
    "spd_parallel_steps_end": (C.c_int, [C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "spd_model_step_checked_begin": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "spd_model_step_checked_end": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "spd_driver_model": (C.c_int, [C.c_int64, C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "spd_check": (C.c_int, [C.c_int64, C.POINTER(C.c_int32)]),
    "spd_transform_spectral2grid": (C.c_int, [C.c_int64]),
    "spd_transform_grid2spectral": (C.c_int, [C.c_int64]),
    "spd_apply_grid_filter": (C.c_int, [C.c_int64]),
    "spd_get": (C.c_int, [C.c_int64, C.c_char_p, C.c_void_p, C.c_size_t]),
    "spd_set": (C.c_int, [C.c_int64, C.c_char_p, C.c_void_p, C.c_size_t]),
    "spd_get_shape": (C.c_int, [C.c_int64, C.c_char_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "spd_is_array": (C.c_int, [C.c_char_p, C.POINTER(C.c_int32)]),
    "spd_registry_entry": (C.c_int, [C.c_int32, C.c_char_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                     C.POINTER(C.c_int32)]),
    "spd_driver_stats": (C.c_int, [C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "spd_model_profile": (C.c_int, [C.c_void_p, C.c_int]),
    "spd_model_profile_read": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "spd_model_profile_read_kernels": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "spd_model_set_physics_precision": (C.c_int, [C.c_void_p, C.c_int]),
    "spd_model_get_config": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "spd_model_group_streams": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "spd_model_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int32]),
    "spd_model_get_option": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_int32)]),
}

EXPORTED_SYMBOLS = tuple(_SIGNATURES)

_lib = None


def lib():
    """Load the HIP library (once).  Raises SpeedyHipError if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.isfile(LIB_PATH):
            raise SpeedyHipError(
                "%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                "(or `make -C pyspeedy_amd/csrc`).  There is no CPU fallback." % LIB_PATH)
        # PyTorch ships its own HIP / ROCr runtime libraries.  They must be in the process BEFORE this library is loaded, so that
        # its libamdhip64 dependency binds to the copy torch initialises: with the opposite order the process holds two ROCr
        # runtimes, only the first of which can open the GPU ("no ROCm-capable device is detected" in the other).
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        try:
            handle = C.CDLL(LIB_PATH)
        except OSError as exc:
            raise SpeedyHipError("cannot load %s: %s" % (LIB_PATH, exc))
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype = res
            fn.argtypes = args
        _lib = handle
    return _lib


def check(rc, what):
    if rc != SPD_OK:
        msg = lib().spd_last_error()
        raise SpeedyHipError("%s failed (%d): %s" % (what, rc, msg.decode() if msg else "?"))


def wintape_plan(start, step0, nsteps, window, sample_every=1):
    """The windows the window tape (EnsembleModel.wintape_configure) closes within `nsteps` steps from the date `start` (a
    datetime or (year, month, day, hour, minute)) and the step counter `step0`: an int32 array [windows][8] of the step counter
    after the window, year, month, day, hour, minute of that state, the samples and the steps in the window.  `window` is a number
    of steps, "day" or "month".  The library's own schedule (spd_wintape_plan): no model and no device are needed."""
    import numpy as np
    kinds = {"day": SPD_WINDOW_DAY, "month": SPD_WINDOW_MONTH}
    if isinstance(window, str):
        if window not in kinds:
            raise ValueError("window must be a number of steps, 'day' or 'month', got %r" % (window,))
        kind, every = kinds[window], 0
    else:
        kind, every = SPD_WINDOW_STEPS, int(window)
    date = tuple(start) if isinstance(start, (tuple, list)) else (start.year, start.month, start.day, start.hour, start.minute)
    args = [int(v) for v in date] + [int(step0), int(nsteps), kind, every, int(sample_every)]
    n = lib().spd_wintape_plan(*args, None, 0)
    if n < 0:
        check(n, "spd_wintape_plan")
    rows = np.zeros((max(n, 1), 8), dtype=np.int32)
    n = lib().spd_wintape_plan(*args, rows.ctypes.data_as(C.POINTER(C.c_int32)), n)
    if n < 0:
        check(n, "spd_wintape_plan")
    return rows[:n]


def butterworth_sections(kind, order, periods, sample_interval):
    """Second-order sections of a digital Butterworth filter for EnsembleModel.filtape_configure: a float64 array [S][5] of
    (b0, b1, b2, a1, a2) with a0 = 1.  `kind` is "lowpass" (passes periods longer than `periods`), "highpass" (shorter) or
    "bandpass" (`periods` = the two edge periods, in either order); periods and `sample_interval` are in the same unit (hours,
    days, or samples with sample_interval = 1) and every period must be longer than two sample intervals.  `order` is the order N
    of the analog prototype, 1 ... 8 (1 ... 4 for a band-pass, which has 2 N poles): |H|^2 = 1 / (1 + W^(2 N)), one half at the
    edges.  Low- and high-pass have ceil(N / 2) sections, the band-pass N.  Bilinear transform with pre-warped edges, w = tan(pi *
    sample_interval / period); every section is scaled to gain 1 at zero frequency (low-pass), at the Nyquist frequency (high-pass)
    or at the band centre sqrt(w1 w2) (band-pass).  numpy only."""
    import numpy as np
    if kind not in ("lowpass", "highpass", "bandpass"):
        raise ValueError("kind must be 'lowpass', 'highpass' or 'bandpass', got %r" % (kind,))
    n = int(order)
    if n != order or n < 1 or n > (4 if kind == "bandpass" else 8):
        raise ValueError("order must be 1 ... %d for a %s, got %r" % (4 if kind == "bandpass" else 8, kind, order))
    edges = np.atleast_1d(np.asarray(periods, dtype=np.float64))
    if edges.shape != ((2,) if kind == "bandpass" else (1,)):
        raise ValueError("periods must be %s for a %s, got %r" % ("two periods" if kind == "bandpass" else "one period", kind, periods))
    dt = float(sample_interval)
    if not dt > 0.0 or not np.all(np.isfinite(edges)) or not np.all(edges > 2.0 * dt):
        raise ValueError("every period must be finite and longer than two sample intervals (%r), got %r" % (sample_interval, periods))
    if kind == "bandpass" and edges[0] == edges[1]:
        raise ValueError("the two periods of a bandpass must differ, got %r" % (periods,))
    warped = np.sort(np.tan(np.pi * dt / edges))  # analog edge frequencies under s = (z - 1) / (z + 1), ascending
    # the prototype's poles in the upper half plane, and the real one of an odd order
    proto = [np.exp(0.5j * np.pi * (2 * k + n + 1) / n) for k in range((n + 1) // 2)]
    if n % 2:
        proto[-1] = complex(-1.0, 0.0)  # (exactly, so that what follows from it is exactly real)

    def z_of(s_pole):
        return (1.0 + s_pole) / (1.0 - s_pole)

    def section(zeros, poles, at):
        """the section with these zeros and poles (a conjugate or real pair, or one real pole), of gain 1 at z = `at`"""
        b = np.real(np.poly(zeros))
        a = np.real(np.poly(poles))
        b = np.concatenate([b, np.zeros(3 - b.size)])
        a = np.concatenate([a, np.zeros(3 - a.size)])
        powers = np.array([1.0, 1.0 / at, 1.0 / (at * at)])
        b = b * (abs(np.dot(a, powers)) / abs(np.dot(b, powers)))
        return [b[0], b[1], b[2], a[1], a[2]]

    out = []
    if kind in ("lowpass", "highpass"):
        low = kind == "lowpass"
        zero, at = (-1.0, 1.0) if low else (1.0, -1.0)
        for q in proto:
            s_pole = warped[0] * q if low else warped[0] / q
            if abs(q.imag) < 1e-12:
                out.append(section([zero], [z_of(s_pole.real)], at))
            else:
                zp = z_of(s_pole)
                out.append(section([zero, zero], [zp, np.conj(zp)], at))
    else:
        band, centre2 = warped[1] - warped[0], warped[0] * warped[1]
        at = z_of(1j * np.sqrt(centre2))
        for q in proto:  # s^2 - q B s + w0^2 = 0: two poles per prototype pole
            root = np.sqrt(complex((q * band) ** 2 - 4.0 * centre2))
            s_plus, s_minus = 0.5 * (q * band + root), 0.5 * (q * band - root)
            if abs(q.imag) < 1e-12:
                if abs(s_plus.imag) > 0.0:  # a conjugate pair
                    zp = z_of(s_plus)
                    out.append(section([1.0, -1.0], [zp, np.conj(zp)], at))
                else:
                    out.append(section([1.0, -1.0], [z_of(s_plus.real), z_of(s_minus.real)], at))
            else:
                for s_pole in (s_plus, s_minus):
                    zp = z_of(s_pole)
                    out.append(section([1.0, -1.0], [zp, np.conj(zp)], at))
    return np.ascontiguousarray(out, dtype=np.float64)


def nudge_gains(tau_hours, levels=None, l_max=31, taper=0):
    """A gain table for EnsembleModel.nudge_configure from a relaxation time scale: an array (levels, 32) of
    g = (2400 / (3600 tau)) * w(l), the fraction of the distance to the target that one 40-minute step removes, by level and total
    wavenumber l.  w = 1 for l <= l_max - taper, a linear ramp (l_max + 1 - l) / (taper + 1) from there to 0 at l_max + 1, and 0
    beyond; the table ends at l = 31, the largest wavenumber that is nudged.  `tau_hours`: one value or one per level.  `levels`:
    None for the 8 model levels, a number of rows (1 for ps), or the 0-based indices of the levels to nudge (8 rows, the others
    zero).  Raises ValueError if a gain exceeds 1 (tau shorter than a step) or tau is not positive."""
    import numpy as np
    rows, chosen = 8, None
    if levels is not None:
        if np.ndim(levels) == 0:
            rows = int(levels)
        else:
            chosen = [int(k) for k in levels]
    tau = np.broadcast_to(np.asarray(tau_hours, dtype=np.float64), (rows,))
    if not np.all(tau > 0):
        raise ValueError("tau_hours must be positive")
    taper = int(taper)
    if taper < 0:
        raise ValueError("taper must not be negative")
    l = np.arange(32)
    w = np.clip((int(l_max) + 1 - l) / (taper + 1.0), 0.0, 1.0)
    g = (2400.0 / (3600.0 * tau))[:, None] * w[None, :]
    if chosen is not None:
        keep = np.zeros(rows, dtype=bool)
        keep[chosen] = True
        g[~keep] = 0.0
    if np.any(g > 1.0):
        raise ValueError("a gain exceeds 1: tau_hours must be at least one 40-minute step (2/3 h)")
    return g


BREED_NAMES = ("vor", "div", "t", "tr", "ps")
# sigma thicknesses of the eight levels (half levels 0, 0.05, 0.14, 0.26, 0.42, 0.60, 0.77, 0.90, 1 as the model holds them: fp32
# literals, differenced in fp64)
_HALF_LEVELS = (0.000, 0.050, 0.140, 0.260, 0.420, 0.600, 0.770, 0.900, 1.000)


def breed_weights(kind="kinetic_energy", levels=None):
    """The weights of a breeding norm for EnsembleModel.breed_configure: a dict name -> array (8,) over vor, div, t, tr, ps (ps
    reads entry 0).  With E the quadratic forms of the definition (the kinetic energy of the difference wind per level for vor and
    div, the area mean square for t, tr and ps) and dhs[k] the sigma thickness of level k, A^2 = sum weights * E is
      "kinetic_energy"  dhs[k] on vor and div: the column kinetic energy per unit mass [m^2 s^-2]
      "total_energy"    adds (cp / Tr) dhs[k] on t and R Tr on ps (ln ps): the dry total-energy norm with the reference temperature
                        Tr = 270 K, cp = 1004 J kg^-1 K^-1 and R = (2 / 7) cp, the model's own constants
      "t_rms"           dhs[k] on t: the column mean square of the temperature difference [K^2]
    `levels`: None for all eight, or the 0-based indices of the levels that take part (the others get weight zero; ps stays)."""
    import numpy as np
    half = np.asarray(_HALF_LEVELS, dtype=np.float32).astype(np.float64)
    dhs = half[1:] - half[:-1]
    if levels is not None:
        keep = np.zeros(8, dtype=bool)
        keep[[int(k) for k in levels]] = True
        dhs = np.where(keep, dhs, 0.0)
    cp, tref = 1004.0, 270.0
    rgas = float(np.float32(2.0) / np.float32(7.0)) * cp
    out = {n: np.zeros(8) for n in BREED_NAMES}
    if kind == "kinetic_energy":
        out["vor"], out["div"] = dhs.copy(), dhs.copy()
    elif kind == "total_energy":
        out["vor"], out["div"] = dhs.copy(), dhs.copy()
        out["t"] = (cp / tref) * dhs
        out["ps"][0] = rgas * tref
    elif kind == "t_rms":
        out["t"] = dhs.copy()
    else:
        raise ValueError("unknown kind of breeding weights '%s' (kinetic_energy, total_energy, t_rms)" % (kind,))
    return out


class ProjectionWeights:
    """Weight maps [48][96] for EnsembleModel.projtape_configure, in the layout of one level of a tape sample: row j = 0 is the
    southernmost Gaussian latitude, column i lies at 3.75 i degrees east.  `lat` and `lon` are the export's coordinates in degrees
    (float32 values, as a Dataset carries them); `area` is the quadrature weight of a grid point, summing to 1 over the sphere: the
    library's Gaussian weight of its row (table "wt", which sums to 1 over a hemisphere) over two hemispheres and the 96 points
    of the row.  Host only: no device is needed."""

    def __init__(self, spectral=None):
        import numpy as np
        handle = None if spectral is None else spectral.handle

        def table(name):
            n = lib().spd_get_table_host(handle, name.encode(), None, 0)
            if n < 0:
                check(int(n), "spd_get_table_host(%s)" % name)
            out = np.empty(int(n), dtype=np.float64)
            lib().spd_get_table_host(handle, name.encode(), out.ctypes.data_as(C.c_void_p), out.size)
            return out

        radang, wt = table("radang"), table("wt")
        # the export's coordinates (the outer boundary's "lon" and "lat": 3.75 i and radang * 90 / asin(1), in single precision)
        self.lon = (np.float32(3.75) * np.arange(IX, dtype=np.float32)).astype(np.float64)
        self.lat = (radang.astype(np.float32) * np.float32(90.0) / np.arcsin(np.float32(1.0))).astype(np.float64)
        rows = np.concatenate([wt, wt[::-1]])  # (wt: the 24 rows of a hemisphere from the pole; radang runs south to north)
        self.area = np.repeat(rows[:, None], IX, axis=1) / (2 * IX)

    def _normalised(self, mask, what):
        import math

        import numpy as np
        w = np.where(mask, self.area, 0.0)
        total = math.fsum(w.ravel())
        if not total > 0.0:
            raise ValueError("%s holds no grid point" % what)
        return w / total

    def box(self, lon0, lon1, lat0, lat1):
        """The quadrature weights of the grid points with lat0 <= lat <= lat1 and longitude from lon0 eastward to lon1 (both ends
        included; lon0 > lon1 after reduction to [0, 360) crosses the date line of the grid, lon1 - lon0 >= 360 is every
        longitude), normalised to sum 1: the area mean over the box.  Raises ValueError for a box without a grid point."""
        import numpy as np
        if lon1 - lon0 >= 360.0:
            in_lon = np.ones(IX, dtype=bool)
        else:
            a, b = lon0 % 360.0, lon1 % 360.0
            in_lon = (self.lon >= a) & (self.lon <= b) if a <= b else (self.lon >= a) | (self.lon <= b)
        in_lat = (self.lat >= lat0) & (self.lat <= lat1)
        return self._normalised(in_lat[:, None] & in_lon[None, :], "the box lon %g ... %g, lat %g ... %g" % (lon0, lon1, lat0, lat1))

    def band(self, lat0, lat1):
        """The zonal band lat0 <= lat <= lat1: box(0, 360, lat0, lat1)."""
        return self.box(0.0, 360.0, lat0, lat1)

    def global_mean(self):
        """The quadrature weights of the whole sphere, normalised to sum 1: box(0, 360, -90, 90)."""
        return self.box(0.0, 360.0, -90.0, 90.0)

    def point(self, lon, lat):
        """The four bilinear weights of the station (lon, lat) in degrees: periodic in longitude, linear in latitude between the
        two Gaussian rows around it and clamped to the outermost rows beyond them."""
        import numpy as np
        x = (lon % 360.0) / 3.75
        i0 = int(np.floor(x))
        fx = x - i0
        i0, i1 = i0 % IX, (i0 + 1) % IX
        if lat <= self.lat[0]:
            j0, fy = 0, 0.0
        elif lat >= self.lat[-1]:
            j0, fy = IL - 2, 1.0
        else:
            j0 = int(np.searchsorted(self.lat, lat, side="right")) - 1
            fy = (lat - self.lat[j0]) / (self.lat[j0 + 1] - self.lat[j0])
        w = np.zeros((IL, IX))
        w[j0, i0] += (1.0 - fx) * (1.0 - fy)
        w[j0, i1] += fx * (1.0 - fy)
        w[j0 + 1, i0] += (1.0 - fx) * fy
        w[j0 + 1, i1] += fx * fy
        return w


def projection_weights(spectral=None):
    """The builder of weight maps for EnsembleModel.projtape_configure (ProjectionWeights: global_mean, box, band, point), from
    the library's own tables -- those of `spectral` (a ModSpectral), or the library's device-less copy of the same tables."""
    return ProjectionWeights(spectral)
