"""Ensemble model object: the device-resident state of M members and the model time step (`step` of
speedy.f90/time_stepping.f90:38-147 for all members at once).

Host arrays use the reference's shapes and Fortran order (what the f2py getters of speedy_driver.f90.j2:250-334
return); on the device every variable is member-major with that same order inside a member, so get/set are plain copies.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import check
from .registry import REGISTRY

# reference shapes of the device-resident registry variables (registry.py); sst_anom follows the model's allocation
SHAPES = {n: (v.dtype, v.shape) for n, v in REGISTRY.items() if v.where == "device"}
SHAPES["sst_anom"] = (np.float64, (96, 48, 3))  # right after creation: n_months = 1

DELT = 86400.0 / 36  # params.f90:33

# kernel ids of spd_model_profile_read_kernels (SPD_K_* of include/pyspeedy_amd.h)
KERNEL_NAMES = ("geopotential", "spec2grid", "column_sw", "column", "grid2spec", "spectral_step", "coupler", "forcing",
                "sppt", "dyn_grid", "physics_sw", "physics")

# boundary-condition file variable -> registry variable (pyspeedy/speedy.py:279-296)
BC_MAP = (("orog", "orog"), ("fmask_orig", "lsm"), ("alb0", "alb"), ("veg_high", "vegh"), ("veg_low", "vegl"),
          ("stl12", "stl"), ("snowd12", "snowd"), ("soil_wc_l1", "swl1"), ("soil_wc_l2", "swl2"), ("soil_wc_l3", "swl3"),
          ("sst12", "sst"), ("sea_ice_frac12", "icec"))


# ---- what the *_configure methods and the ring readers of EnsembleModel share ----
def _c_array(ctype, values):
    """a ctypes array of `values` (of one element where there are none: the library is never handed a null list)"""
    values = list(values)
    return (ctype * max(len(values), 1))(*values)


def _c_names(names):
    return _c_array(C.c_char_p, [n.encode() for n in names])


def _pattern_rows(entries):
    """the (name, level, pattern) entries of the projection tape, the assimilation and the verification tape"""
    rows = []
    for entry in entries:
        if len(entry) != 3:
            raise ValueError("an entry is (name, level, pattern), got %r" % (entry,))
        rows.append((str(entry[0]), int(entry[1]), int(entry[2])))
    return rows


def _weight_maps(weights, checked=True):
    w = np.ascontiguousarray(weights, dtype=np.float64)
    if checked and (w.ndim != 3 or w.shape[1:] != (48, 96)):
        raise ValueError("weights must be [P][48][96], got shape %r" % (w.shape,))
    return w


def _held_span(info, t0, nt):
    """(t0, nt) of a ring reader: nt = None is every held sample from t0 on"""
    t0 = int(t0)
    return t0, info["held"] - t0 if nt is None else int(nt)


class EnsembleModel:
    def __init__(self, spectral, nmembers):
        self.sp = spectral
        self.nmembers = int(nmembers)
        self._lib = _lib.lib()
        self._m = C.c_void_p()
        self.n_months = 1  # sst_anom holds n_months + 2 planes
        self._shapes = dict(SHAPES)  # per model: set_sppt adds the two SPPT arrays
        self._owned = True
        with torch.cuda.device(spectral.device):
            check(self._lib.spd_model_create(spectral.handle, self.nmembers, C.byref(self._m)), "spd_model_create")

    @classmethod
    def borrowed(cls, handle, nmembers, device, n_months=1):
        """A view of a device model that something else owns (the C driver's containers, speedy_driver.device_model): the
        same methods, nothing is created and nothing destroyed."""
        import types
        self = cls.__new__(cls)
        self.sp = types.SimpleNamespace(device=device)
        self.nmembers, self.n_months = int(nmembers), int(n_months)
        self._lib, self._m, self._owned = _lib.lib(), handle, False
        self._shapes = dict(SHAPES)
        return self

    def close(self):
        if getattr(self, "_m", None) is not None and self._m:
            if self._owned:
                self._lib.spd_model_destroy(self._m)
            self._m = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- registry access (speedy_driver.f90.j2:250-334) --------------------------------------------------
    def variables(self):
        """Names of the registry arrays of this model (the reference's + tcorh / qcorh [+ the SPPT arrays when SPPT is on])."""
        return tuple(self._shapes)

    def shape(self, name):
        dtype, shape = self._shapes[name]
        return (dtype, (96, 48, self.n_months + 2)) if name == "sst_anom" else (dtype, shape)

    def set(self, name, value, member=-1):
        """Copy a host array (reference shape) into one member, or into every member when member == -1."""
        dtype, shape = self.shape(name)
        a = np.asarray(value, dtype=dtype)
        if a.shape != shape:
            raise ValueError("Array shape missmatch: %s expects %s, got %s" % (name, shape, a.shape))  # speedy.py:153
        flat = np.ascontiguousarray(a.ravel(order="F"))
        check(self._lib.spd_model_set(self._m, name.encode(), int(member), flat.ctypes.data_as(C.c_void_p), flat.nbytes),
              "spd_model_set(%s)" % name)

    def get(self, name, member=0):
        dtype, shape = self.shape(name)
        flat = np.empty(int(np.prod(shape)), dtype=dtype)
        check(self._lib.spd_model_get(self._m, name.encode(), int(member), flat.ctypes.data_as(C.c_void_p), flat.nbytes),
              "spd_model_get(%s)" % name)
        return flat.reshape(shape, order="F")

    # work arrays of the step that are registered with the C model without being registry variables of the reference: the
    # grid-point inputs of the column physics (physics.f90:89-101) as the last step left them
    WORK_ARRAYS = {"u_grid_phys": (96, 48, 8), "v_grid_phys": (96, 48, 8), "t_grid_phys": (96, 48, 8), "q_grid_phys": (96, 48, 8),
                   "phi_grid_phys": (96, 48, 8), "pslg_phys": (96, 48)}

    def device_view(self, name):
        """Zero-copy torch view [nmembers, *reversed reference shape] of a registry variable in HBM (C order == the
        reference's Fortran order inside a member).  For on-device post-processing such as ensemble statistics.

        The view stays valid for the life of the model (spd_model_device_ptr, include/pyspeedy_amd.h): after every later
        step it shows the variable as that step left it.  Taking the view drops what the model had derived from the state;
        WRITING through a view taken earlier must be followed by `invalidate()` before the next step.  A view of "phi"
        pins the geopotential to one buffer (small ensembles lose the 1-3 % of the look-ahead geopotential)."""
        dtype, shape = (np.float64, self.WORK_ARRAYS[name]) if name in self.WORK_ARRAYS else self.shape(name)
        ptr = self._lib.spd_model_device_ptr(self._m, name.encode())
        if not ptr:
            raise KeyError(name)
        if self._lib.spd_model_var_storage(self._m, name.encode()) == 4:
            # cfg 5 (set_physics_precision(True)): what only the column physics reads back is STORED as float32; the view shows the
            # array as it is in memory (a view taken before the precision was switched shows bytes that no longer mean anything)
            dtype = np.float32

        class _Blob:  # CUDA array interface v2 (understood by torch.as_tensor on ROCm builds as well)
            __cuda_array_interface__ = {"shape": (self.nmembers,) + tuple(reversed(shape)),
                                        "typestr": np.dtype(dtype).str, "data": (int(ptr), False), "version": 2}
        return torch.as_tensor(_Blob(), device=self.sp.device)

    def invalidate(self):
        """The state was written through a device view taken earlier: drop what the model derived from it (look-ahead
        geopotential, the day's interpolated climatologies)."""
        check(self._lib.spd_model_invalidate(self._m), "spd_model_invalidate")

    def set_sppt(self, on=True, seed=0, first_member_id=0):
        """Switch the deterministic SPPT scheme (csrc/sppt.hip) on or off; `first_member_id` = global id of member 0 of
        this shard, so that an ensemble gives the same noise however it is split over GPUs."""
        check(self._lib.spd_model_set_sppt(self._m, int(bool(on)), int(seed), int(first_member_id)), "spd_model_set_sppt")
        if on:
            self._shapes.setdefault("sppt_spec", (np.complex128, (31, 32, 8)))
            self._shapes.setdefault("sppt_pattern", (np.float64, (96, 48, 8)))

    @property
    def co2(self):
        return float(self._lib.spd_model_co2(self._m))

    def set_co2(self, value):
        check(self._lib.spd_model_set_co2(self._m, float(value)), "spd_model_set_co2")

    # ---- lifecycle (pyspeedy/speedy.py:217-301, 375-405) ----------------------------------------------------
    def set_bc(self, bc, start_date=(1982, 1, 1, 0, 0), member=-1):
        """Load the 12 boundary fields (mapping like example_bc.nc, dims (lon, lat[, month])) and run the reference's
        `init`: land/sea preprocessing, rest atmosphere, coupler, forcing, first_step.  Zero SST anomaly unless
        `sst_anom` was set before."""
        for state_name, bc_name in BC_MAP:
            self.set(state_name, np.asarray(bc[bc_name], dtype=np.float64), member)
        self.init(start_date)

    def init(self, start_date=(1982, 1, 1, 0, 0)):
        """The reference's `init` (initialize_state) for every member, from the boundary fields stored with set()."""
        check(self._lib.spd_model_init(self._m, *[int(v) for v in start_date], self._stream()), "spd_model_init")

    def init_sst_anom(self, n_months):
        """modelstate_init_sst_anom: (re)allocate sst_anom with n_months + 2 zero-filled planes per member."""
        check(self._lib.spd_model_init_sst_anom(self._m, int(n_months)), "spd_model_init_sst_anom")
        self.n_months = int(n_months)

    def mark_initialized(self, current_step, date):
        """Declare a state loaded through set() / copy_member_from() as initialised at `date` = (y, m, d, h, mi)."""
        check(self._lib.spd_model_mark_initialized(self._m, int(current_step), *[int(v) for v in date]),
              "spd_model_mark_initialized")
        self.set_time_step(2 * DELT)

    # ---- checkpoint / resume: the registry arrays plus the host-side control block are the whole state of a run -------
    def control(self):
        """spd_model_control: step counter, date, month index, coupling / CO2 flags, CO2 reference, SPPT generator position."""
        c = _lib.ModelControl()
        check(self._lib.spd_model_get_control(self._m, C.byref(c)), "spd_model_get_control")
        return c

    def state_dict(self, member=0):
        """Everything needed to continue a member's run elsewhere, bit for bit (numpy arrays in the reference's shapes plus
        the control block as `__control__/<field>` scalars)."""
        out = {n: self.get(n, member) for n in self._shapes if n != "sppt_pattern"}  # (the pattern is recomputed every step)
        c = self.control()
        for name, _ in c._fields_:
            out["__control__/" + name] = np.asarray(getattr(c, name))
        return out

    def load_state_dict(self, state, member=-1):
        """Inverse of state_dict (member = -1: every member gets the same state); marks the model initialised and resets
        nothing: month index, CO2 reference, flags and the SPPT position continue where the checkpoint left them."""
        c = _lib.ModelControl()
        for name, _ in c._fields_:
            setattr(c, name, state["__control__/" + name].item())
        if state["sst_anom"].shape[2] != self.n_months + 2:
            self.init_sst_anom(state["sst_anom"].shape[2] - 2)
        if c.sppt_on:
            self.set_sppt(True, c.sppt_seed, c.sppt_first_member_id)
        for n in self._shapes:
            if n in state:
                self.set(n, state[n], member)
        check(self._lib.spd_model_set_control(self._m, C.byref(c)), "spd_model_set_control")
        self.set_time_step(2 * DELT)

    def copy_member_from(self, src, src_member, dst_member):
        """Device-to-device copy of every registry variable of one member of `src` into one of this model's members."""
        check(self._lib.spd_model_copy_member(self._m, int(dst_member), src._m, int(src_member), self._stream()),
              "spd_model_copy_member")

    def sync(self):
        torch.cuda.current_stream().synchronize()

    @staticmethod
    def _stream():
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    # ---- grid-space views of the prognostic variables (prognostics.f90:125-219) -------------------------
    def _range(self, first, count):
        return int(first), int(self.nmembers - first if count is None else count)

    def spectral2grid(self, first=0, count=None):
        check(self._lib.spd_model_spectral2grid(self._m, *self._range(first, count), self._stream()), "spd_model_spectral2grid")

    def grid2spectral(self, first=0, count=None):
        check(self._lib.spd_model_grid2spectral(self._m, *self._range(first, count), self._stream()), "spd_model_grid2spectral")

    def grid_filter(self, first=0, count=None):
        check(self._lib.spd_model_grid_filter(self._m, *self._range(first, count), self._stream()), "spd_model_grid_filter")

    def run(self, nsteps):
        """`nsteps` model steps (40 simulated minutes each) for every member; asynchronous."""
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        check(self._lib.spd_model_step(self._m, int(nsteps), stream), "spd_model_step")

    def run_checked(self, nsteps):
        """`nsteps` steps as ONE device call with the range check of EVERY step recorded by the device
        (spd_model_step_checked_begin / _end); waits for it.  -> (first_failed, accepted): per member the first step of the call
        (0-based) whose check failed, -1 for none, and [members, 7] the model's step counter, date (y, m, d, h, min) and month index
        after the member's last accepted step."""
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        check(self._lib.spd_model_step_checked_begin(self._m, int(nsteps), stream), "spd_model_step_checked_begin")
        failed = np.zeros(self.nmembers, dtype=np.int32)
        accepted = np.zeros((self.nmembers, 7), dtype=np.int32)
        check(self._lib.spd_model_step_checked_end(self._m, failed.ctypes.data_as(C.POINTER(C.c_int32)),
                                                   accepted.ctypes.data_as(C.POINTER(C.c_int32))), "spd_model_step_checked_end")
        return failed, accepted

    @property
    def current_step(self):
        return int(self._lib.spd_model_current_step(self._m))

    @property
    def current_date(self):
        buf = (C.c_int * 5)()
        check(self._lib.spd_model_get_date(self._m, buf), "spd_model_get_date")
        return tuple(buf)

    def set_physics_precision(self, fp32):
        """BASELINE cfg 5: run the arithmetic of the column physics in single precision AND keep what only the column physics
        reads back -- its grid-point inputs at the physics' time level, the radiation state persisted between shortwave steps
        (tt_rsw, rad_tau2, rad_strat_corr), the diagnostics-only outputs (rad_st4a, rad_flux, precnv, precls, cbmf, slrd, slr,
        olr, slru, ustr, vstr) -- in memory as float32.  State, dynamics and tendencies stay fp64; get / set of the narrowed
        variables still speak float64 (converted on the way); device_view shows them as float32.  Switching converts the
        arrays in place."""
        check(self._lib.spd_model_set_physics_precision(self._m, int(bool(fp32))), "spd_model_set_physics_precision")

    def memory(self):
        """Device memory of the model in bytes: (reserved, in use) -- spd_model_memory."""
        reserved, used = C.c_size_t(0), C.c_size_t(0)
        check(self._lib.spd_model_memory(self._m, C.byref(reserved), C.byref(used)), "spd_model_memory")
        return reserved.value, used.value

    def config(self):
        """How the step is configured: dict(inv_per_member, diag_every_step, chunks, split_dyn, ...) -- spd_model_get_config.
        The land / sea-ice coupling always rides in spectral_step_kernel: its key is always True.  forward_table: "products" when
        the step's grid -> spectral launch forms the flux and kinetic-energy products itself (the fused column kernel, which does
        not store them), "plain" when it reads them from memory (split_dyn: the stand-alone dynamics kernel stores them).
        tau_recompute: 0 / 1 / 2, whether multi-step calls recompute the longwave transmissivities between shortwave steps
        instead of re-loading rad_tau2 -- never / from 20 members up / whatever the size."""
        cfg = (C.c_int32 * 8)()
        check(self._lib.spd_model_get_config(self._m, cfg), "spd_model_get_config")
        created, apart = C.c_int32(0), C.c_int32(1)
        check(self._lib.spd_model_group_streams(self._m, C.byref(created), C.byref(apart)), "spd_model_group_streams")
        block = C.c_int32(0)
        check(self._lib.spd_model_get_option(self._m, b"block_members", C.byref(block)), "spd_model_get_option")
        # (a library from before the product table -- PYSPEEDY_AMD_LIB, tools/build_variant.sh -- does not know the name: plain)
        staged = C.c_int32(0)
        rc = self._lib.spd_model_get_option(self._m, b"staged_products", C.byref(staged))
        if rc != _lib.SPD_E_ARG:
            check(rc, "spd_model_get_option")
        # (... nor, from before the compact record of the longwave transmissivities, this one: every step uses rad_tau2)
        tau = C.c_int32(0)
        rc = self._lib.spd_model_get_option(self._m, b"tau_recompute", C.byref(tau))
        if rc != _lib.SPD_E_ARG:
            check(rc, "spd_model_get_option")
        streams, M = cfg[2], self.nmembers
        # (as spd_model_step forms them: rounds of `chunks` x `block_members` members from 4 x block_members members up; not while
        # profiling or with separate dynamics / physics launches, which step everybody as one group)
        rounds = 1
        if block.value > 0 and M >= 4 * block.value and not cfg[3]:
            rounds = (M + max(streams, 1) * block.value - 1) // (max(streams, 1) * block.value)
        return dict(inv_per_member=cfg[0], diag_every_step=bool(cfg[1]), chunks=cfg[2], split_dyn=bool(cfg[3]),
                    fold_geo=bool(cfg[4]), coupler_in_spectral=bool(cfg[5]), physics_fp32=bool(cfg[6]),
                    physics_storage32=bool(cfg[7]), group_streams=created.value, group_streams_apart=bool(apart.value),
                    block_members=block.value, rounds=rounds, forward_table="products" if staged.value else "plain",
                    tau_recompute=tau.value)

    def set_option(self, name, value):
        """A launch-plan switch of the live model by name (spd_model_set_option: diag_every_step, spectral_early, split_dyn,
        member_groups, block_members, physics_storage32, tau_recompute); none of them changes the state a step leaves behind.
        ValueError for an unknown name."""
        rc = self._lib.spd_model_set_option(self._m, name.encode(), int(value))
        if rc == _lib.SPD_E_ARG:
            raise ValueError("unknown option or value out of range: %s = %r" % (name, value))
        check(rc, "spd_model_set_option")

    def get_option(self, name):
        """The value of a switch of set_option, or of a read-only figure (spd_model_get_option): quiet_rim_members is the number
        of members whose coefficients beyond the truncation's halo the last multi-step call found to be all-zero bits and left
        alone, -1 when that call did not look (a call of one step, or an ensemble of up to 8 members).  ValueError for an
        unknown name."""
        value = C.c_int32(0)
        rc = self._lib.spd_model_get_option(self._m, name.encode(), C.byref(value))
        if rc == _lib.SPD_E_ARG:
            raise ValueError("unknown option: %s" % name)
        check(rc, "spd_model_get_option")
        return value.value

    def profile(self, level=1):
        """HIP-event brackets on the launch stream: 0 off, 1 the spectral->grid launch of every step, 2 every kernel."""
        check(self._lib.spd_model_profile(self._m, int(level)), "spd_model_profile")

    def profile_read_kernels(self):
        """{kernel id (KERNEL_NAMES): (mean ms, min ms, brackets, units per bracket)} since profile(2)."""
        n = len(KERNEL_NAMES)
        mean, mn = np.zeros(n), np.zeros(n)
        cnt, units = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
        check(self._lib.spd_model_profile_read_kernels(self._m, mean.ctypes.data_as(C.c_void_p), mn.ctypes.data_as(C.c_void_p),
                                                       cnt.ctypes.data_as(C.c_void_p), units.ctypes.data_as(C.c_void_p)),
              "spd_model_profile_read_kernels")
        return {KERNEL_NAMES[k]: (float(mean[k]), float(mn[k]), int(cnt[k]), int(units[k])) for k in range(n) if cnt[k]}

    def profile_read(self):
        """(mean launch time in ms, number of launches, fields per launch) of the spectral->grid kernel since profile(True)."""
        ms, n, f = C.c_double(), C.c_int(), C.c_int()
        check(self._lib.spd_model_profile_read(self._m, C.byref(ms), C.byref(n), C.byref(f)), "spd_model_profile_read")
        return ms.value, n.value, f.value

    # ---- time-mean statistics accumulated on the device (spd_model_stats_*, include/pyspeedy_amd.h) ---------------------
    STATS_VARIABLES = ("u_grid", "v_grid", "t_grid", "q_grid", "phi_grid", "ps_grid", "precnv", "precls",
                       "u_plev", "v_plev", "t_plev", "q_plev", "z_plev", "mslp")  # (the last six: after plev_configure)
    # (every recorder that takes these names takes the fourteen DERIVED_VARIABLES as well)

    def stats_configure(self, variables, every, variance=True):
        """Sample `variables` (any of STATS_VARIABLES) after every step that leaves current_step at a multiple of `every`, inside
        run() / run_checked() calls of any length; per member and grid point the mean and, with `variance`, the unbiased time
        variance.  Starts a new averaging period; an empty list switches sampling off.  Synchronises the device."""
        names = [str(v) for v in variables]
        arr = _c_names(names)
        check(self._lib.spd_model_stats_configure(self._m, arr, len(names), int(every), int(bool(variance))),
              "spd_model_stats_configure")

    def stats_reset(self):
        """Start a new averaging period (e.g. at a month boundary a call was made to end at)."""
        check(self._lib.spd_model_stats_reset(self._m), "spd_model_stats_reset")

    @property
    def stats_samples(self):
        n = self._lib.spd_model_stats_samples(self._m)
        if n < 0:
            check(n, "spd_model_stats_samples")
        return int(n)

    def _stats_shape(self, name):
        if name in self.PLEV_VARIABLES[:5] or name in self.DERIVED_VARIABLES[9:]:
            return (len(self.plev_levels), 48, 96)
        levels = 8 if name in ("u_grid", "v_grid", "t_grid", "q_grid", "phi_grid") + self.DERIVED_VARIABLES[:5] else 1
        return (levels, 48, 96) if levels > 1 else (48, 96)

    def _stats_read(self, name, kind, first, count):
        first, count = self._range(first, count)
        out = torch.empty((count,) + self._stats_shape(name), dtype=torch.float64, device=self.sp.device)
        with torch.cuda.device(self.sp.device):
            check(self._lib.spd_model_stats_read(self._m, name.encode(), kind, first, count, C.c_void_p(out.data_ptr()),
                                                 out.numel() * 8, self._stream()), "spd_model_stats_read(%s)" % name)
        return out

    def stats_mean(self, name, first=0, count=None):
        """Time mean of members [first, first + count): float64 tensor on the model's device, laid out as device_view(name)."""
        return self._stats_read(name, _lib.SPD_STATS_MEAN, first, count)

    def stats_var(self, name, first=0, count=None):
        """Unbiased time variance (ddof 1) of members [first, first + count), laid out as stats_mean."""
        return self._stats_read(name, _lib.SPD_STATS_VARIANCE, first, count)

    def stats_ensemble(self, name):
        """(mean, std) over the members of their time means, per point (std: ddof 1); float64 tensors [levels,] 48, 96."""
        out = []
        for kind in (_lib.SPD_STATS_MEAN, _lib.SPD_STATS_STD):
            t = torch.empty(self._stats_shape(name), dtype=torch.float64, device=self.sp.device)
            with torch.cuda.device(self.sp.device):
                check(self._lib.spd_model_stats_ensemble(self._m, name.encode(), kind, C.c_void_p(t.data_ptr()), t.numel() * 8,
                                                         self._stream()), "spd_model_stats_ensemble(%s)" % name)
            out.append(t)
        return tuple(out)

    # ---- the tape: time series of fields recorded on the device (spd_model_tape_*, include/pyspeedy_amd.h) ---------------
    TAPE_DTYPES = {"float32": (_lib.SPD_TAPE_F32, torch.float32), "float64": (_lib.SPD_TAPE_F64, torch.float64)}

    def tape_configure(self, variables, every, capacity, dtype="float32"):
        """Record `variables` (any of STATS_VARIABLES) after every step that leaves current_step at a multiple of `every`, inside
        run() / run_checked() calls of any length, into a ring in device memory that keeps the last `capacity` samples of every
        member; dtype "float32" (the default: what the export writes) or "float64".  Empties the tape; an empty list switches it
        off and frees it.  Synchronises the device."""
        key = str(dtype).replace("torch.", "")
        if key not in self.TAPE_DTYPES:
            raise ValueError("dtype must be 'float32' or 'float64', got %r" % (dtype,))
        names = [str(v) for v in variables]
        arr = _c_names(names)
        with torch.cuda.device(self.sp.device):
            check(self._lib.spd_model_tape_configure(self._m, arr, len(names), int(every), int(capacity), self.TAPE_DTYPES[key][0]),
                  "spd_model_tape_configure")

    def tape_reset(self):
        """Empty the tape (no device work); the next sample is the first."""
        check(self._lib.spd_model_tape_reset(self._m), "spd_model_tape_reset")

    @property
    def tape_info(self):
        """dict(taken, held, capacity, every, dtype): samples since the last reset, samples the ring holds (min(taken, capacity)),
        and the configuration."""
        taken, held, capacity, every, dtype = C.c_longlong(0), C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
        check(self._lib.spd_model_tape_info(self._m, C.byref(taken), C.byref(held), C.byref(capacity), C.byref(every), C.byref(dtype)),
              "spd_model_tape_info")
        name = [k for k, v in self.TAPE_DTYPES.items() if v[0] == dtype.value][0]
        return dict(taken=int(taken.value), held=held.value, capacity=capacity.value, every=every.value, dtype=name)

    # ---- shared by the recorders that take a member mask, and by those that remember their entries ----
    def _member_mask(self, members):
        mask = np.ascontiguousarray(np.asarray(members).astype(np.int32))
        if mask.shape != (self.nmembers,):
            raise ValueError("members must have one entry per member (%d), got shape %s" % (self.nmembers, mask.shape))
        return mask

    def _configure_refused(self, symbol, rc, gone, attr):
        """a _configure call returned non-zero: the remembered entries go if the refusal came behind the point where the earlier
        configuration went (`gone()`), and the library's text is raised"""
        text = (self._lib.spd_last_error() or b"?").decode()
        if gone():
            setattr(self, attr, ())
        raise _lib.SpeedyHipError("%s failed (%d): %s" % (symbol, rc, text))

    # ---- the rows a ring keeps beside its slots (csrc/ring.hpp): step and date of each held sample, window or event, oldest first ----
    def _ring_rows(self, symbol, held, width):
        rows = np.zeros((max(held, 1), width), dtype=np.int32)
        n = getattr(self._lib, symbol)(self._m, rows.ctypes.data_as(C.POINTER(C.c_int32)), held)
        if n < 0:
            check(n, symbol)
        return rows[:n]

    @staticmethod
    def _row_steps(rows):
        return rows[:, 0].astype(np.int64)

    @staticmethod
    def _row_times(rows):
        from datetime import datetime
        return [datetime(*(int(v) for v in row[1:6])) for row in rows]

    def _tape_rows(self):
        return self._ring_rows("spd_model_tape_times", self.tape_info["held"], 6)

    def tape_steps(self):
        """The model's step counter after each held sample's step, oldest first (numpy int array)."""
        return self._row_steps(self._tape_rows())

    def tape_times(self):
        """The date of each held sample's state, oldest first (a list of datetime)."""
        return self._row_times(self._tape_rows())

    def tape(self, name, first=0, count=None, t0=0, nt=None):
        """Members [first, first + count) and samples [t0, t0 + nt) of the held ones (oldest first) of one variable: a tensor
        [count][nt][levels][48][96] ([count][nt][48][96] for one-level names) on the model's device in the tape's dtype."""
        first, count = self._range(first, count)
        info = self.tape_info
        t0, nt = _held_span(info, t0, nt)
        dtype = self.TAPE_DTYPES[info["dtype"]][1]
        out = torch.empty((count, max(nt, 0)) + self._stats_shape(name), dtype=dtype, device=self.sp.device)
        with torch.cuda.device(self.sp.device):
            check(self._lib.spd_model_tape_read(self._m, name.encode(), first, count, t0, nt, C.c_void_p(out.data_ptr()),
                                                out.numel() * out.element_size(), self._stream()), "spd_model_tape_read(%s)" % name)
        return out

    # ---- the ensemble tape: series of the mean and spread over the members (spd_model_enstape_*, include/pyspeedy_amd.h) ---
    def enstape_configure(self, variables, every, capacity):
        """Record the ensemble mean and spread of `variables` (any of STATS_VARIABLES) after every step that leaves current_step
        at a multiple of `every`, inside run() / run_checked() calls of any length, into a ring in device memory that keeps the last
        `capacity` samples: per grid point the mean over all members of this model and the sum of squared deviations from it,
        float64 -- two planes per sample and member group, whatever the number of members.  Empties the ring; an empty list
        switches it off and frees it.  Synchronises the device."""
        names = [str(v) for v in variables]
        arr = _c_names(names)
        with torch.cuda.device(self.sp.device):
            check(self._lib.spd_model_enstape_configure(self._m, arr, len(names), int(every), int(capacity)),
                  "spd_model_enstape_configure")

    def enstape_reset(self):
        """Empty the ensemble tape (no device work); the next sample is the first."""
        check(self._lib.spd_model_enstape_reset(self._m), "spd_model_enstape_reset")

    @property
    def enstape_info(self):
        """dict(taken, held, capacity, every, members): samples since the last reset, samples the ring holds (min(taken,
        capacity)), the configuration, and the number of members a sample reduces over."""
        taken, held, capacity, every, members = C.c_longlong(0), C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
        check(self._lib.spd_model_enstape_info(self._m, C.byref(taken), C.byref(held), C.byref(capacity), C.byref(every),
                                               C.byref(members)), "spd_model_enstape_info")
        return dict(taken=int(taken.value), held=held.value, capacity=capacity.value, every=every.value, members=members.value)

    def _enstape_rows(self):
        return self._ring_rows("spd_model_enstape_times", self.enstape_info["held"], 6)

    def enstape_steps(self):
        """The model's step counter after each held sample's step, oldest first (numpy int array)."""
        return self._row_steps(self._enstape_rows())

    def enstape_times(self):
        """The date of each held sample's state, oldest first (a list of datetime)."""
        return self._row_times(self._enstape_rows())

    def _enstape_read(self, name, kind, t0, nt):
        t0, nt = _held_span(self.enstape_info, t0, nt)
        out = torch.empty((max(nt, 0),) + self._stats_shape(name), dtype=torch.float64, device=self.sp.device)
        with torch.cuda.device(self.sp.device):
            check(self._lib.spd_model_enstape_read(self._m, name.encode(), kind, t0, nt, C.c_void_p(out.data_ptr()), out.numel() * 8,
                                                   self._stream()), "spd_model_enstape_read(%s)" % name)
        return out

    def enstape(self, name, t0=0, nt=None):
        """(mean, std) over the members for the samples [t0, t0 + nt) of the held ones (oldest first) of one variable: float64
        tensors [nt][levels][48][96] ([nt][48][96] for one-level names) on the model's device; std is the unbiased standard
        deviation (ddof 1; NaN for a model of one member)."""
        return (self._enstape_read(name, _lib.SPD_ENS_MEAN, t0, nt), self._enstape_read(name, _lib.SPD_ENS_STD, t0, nt))

    def enstape_moments(self, name, t0=0, nt=None):
        """(members, mean, m2) of the same samples: m2 is the sum over the members of the squared deviations from the mean.  What
        pyspeedy_amd.ensemble.merge_moments combines across several models or ranks."""
        return (self.enstape_info["members"], self._enstape_read(name, _lib.SPD_ENS_MEAN, t0, nt),
                self._enstape_read(name, _lib.SPD_ENS_M2, t0, nt))

    # ---- the accumulation tape: window sums, means and extremes of the physics fluxes (spd_model_acctape_*, pyspeedy_amd.h) ---
    ACCTAPE_NAMES = ("precnv", "precls", "cbmf", "olr", "tsr", "ssr", "ssrd", "slr", "slrd", "ustr", "vstr", "shf", "evap", "slru")
    ACCTAPE_THREE_PLANES = ("ustr", "vstr", "shf", "evap", "slru")  # land, sea, weighted by the land fraction
    ACCTAPE_OPS = {"sum": _lib.SPD_ACC_SUM, "mean": _lib.SPD_ACC_MEAN, "min": _lib.SPD_ACC_MIN, "max": _lib.SPD_ACC_MAX}

    def _acctape_op(self, op):
        if op not in self.ACCTAPE_OPS:
            raise ValueError("op must be one of 'sum', 'mean', 'min', 'max', got %r" % (op,))
        return self.ACCTAPE_OPS[op]

    def acctape_configure(self, entries, every, capacity, dtype="float32"):
        """Accumulate over windows of steps, inside run() / run_checked() calls of any length: `entries` is a list of (name, op)
        pairs, name any of ACCTAPE_NAMES (the column physics' 2-D outputs, in the registry's unit), op "sum", "mean", "min" or
        "max".  Every step adds to the open window; a window closes after every step that leaves current_step at a multiple of
        `every` into a ring in device memory that keeps the last `capacity` windows of every member; dtype "float32" (the default)
        or "float64".  The first window starts at the current step and may be shorter (acctape_counts()).  Empties the ring; an
        empty list switches the recorder off and frees it.  Synchronises the device."""
        key = str(dtype).replace("torch.", "")
        if key not in self.TAPE_DTYPES:
            raise ValueError("dtype must be 'float32' or 'float64', got %r" % (dtype,))
        pairs = [(str(n), self._acctape_op(op)) for n, op in entries]
        names, ops = _c_names(n for n, _ in pairs), _c_array(C.c_int, (op for _, op in pairs))
        with torch.cuda.device(self.sp.device):
            check(self._lib.spd_model_acctape_configure(self._m, names, ops, len(pairs), int(every), int(capacity),
                                                        self.TAPE_DTYPES[key][0]), "spd_model_acctape_configure")

    def acctape_reset(self):
        """Empty the ring and start a new window at the current step (no device work)."""
        check(self._lib.spd_model_acctape_reset(self._m), "spd_model_acctape_reset")

    @property
    def acctape_info(self):
        """dict(taken, held, capacity, every, dtype): windows closed since the last reset, windows the ring holds (min(taken,
        capacity)), and the configuration."""
        taken, held, capacity, every, dtype = C.c_longlong(0), C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
        check(self._lib.spd_model_acctape_info(self._m, C.byref(taken), C.byref(held), C.byref(capacity), C.byref(every),
                                               C.byref(dtype)), "spd_model_acctape_info")
        name = [k for k, v in self.TAPE_DTYPES.items() if v[0] == dtype.value][0]
        return dict(taken=int(taken.value), held=held.value, capacity=capacity.value, every=every.value, dtype=name)

    def _acctape_rows(self):
        return self._ring_rows("spd_model_acctape_times", self.acctape_info["held"], 7)

    def acctape_steps(self):
        """The model's step counter after the last step of each held window, oldest first (numpy int array)."""
        return self._row_steps(self._acctape_rows())

    def acctape_times(self):
        """The date of the state after each held window's last step, oldest first (a list of datetime)."""
        return self._row_times(self._acctape_rows())

    def acctape_counts(self):
        """The number of steps in each held window, oldest first (numpy int array)."""
        return self._acctape_rows()[:, 6].astype(np.int64)

    def acctape(self, name, op, first=0, count=None, t0=0, nt=None):
        """Members [first, first + count) and windows [t0, t0 + nt) of the held ones (oldest first) of one entry: a tensor
        [count][nt][48][96] ([count][nt][3][48][96] for the names of ACCTAPE_THREE_PLANES) on the model's device in the ring's
        dtype."""
        first, count = self._range(first, count)
        info = self.acctape_info
        t0, nt = _held_span(info, t0, nt)
        dtype = self.TAPE_DTYPES[info["dtype"]][1]
        inner = (3, 48, 96) if name in self.ACCTAPE_THREE_PLANES else (48, 96)
        out = torch.empty((count, max(nt, 0)) + inner, dtype=dtype, device=self.sp.device)
        with torch.cuda.device(self.sp.device):
            check(self._lib.spd_model_acctape_read(self._m, name.encode(), self._acctape_op(op), first, count, t0, nt,
                                                   C.c_void_p(out.data_ptr()), out.numel() * out.element_size(), self._stream()),
                  "spd_model_acctape_read(%s, %s)" % (name, op))
        return out

    # ---- the window tape: window means, extremes and threshold counts of the state's fields (spd_model_wintape_*) ----------
    WINTAPE_NAMES = STATS_VARIABLES + ("wspd_grid", "wspd_plev")  # (the wind speeds: sqrt(u * u + v * v), this recorder only)
    WINTAPE_OPS = {"sum": _lib.SPD_WIN_SUM, "mean": _lib.SPD_WIN_MEAN, "min": _lib.SPD_WIN_MIN, "max": _lib.SPD_WIN_MAX,
                   "count_above": _lib.SPD_WIN_COUNT_ABOVE, "count_below": _lib.SPD_WIN_COUNT_BELOW}
    WINTAPE_WINDOWS = {"day": _lib.SPD_WINDOW_DAY, "month": _lib.SPD_WINDOW_MONTH}

    wintape_plan = staticmethod(_lib.wintape_plan)  # (the windows ahead, from the library's own schedule: no device needed)

    def _wintape_op(self, op):
        if op not in self.WINTAPE_OPS:
            raise ValueError("op must be one of 'sum', 'mean', 'min', 'max', 'count_above', 'count_below', got %r" % (op,))
        return self.WINTAPE_OPS[op]

    def wintape_configure(self, entries, window, capacity, sample_every=1, dtype="float32"):
        """Accumulate the state's fields over windows, inside run() / run_checked() calls of any length.  `entries` is a list of
        (name, op) or (name, op, threshold): name any of WINTAPE_NAMES (the tape's fourteen, the pressure-level ones after
        plev_configure with its levels in hPa, and the wind speeds wspd_grid / wspd_plev), op "sum", "mean", "min", "max",
        "count_above" (samples with x > threshold) or "count_below" (x < threshold); a threshold is in the unit tape() returns the
        name in (t_grid in K, winds in m/s, ps_grid and mslp in Pa).  A sample is taken after every step that leaves current_step
        at a multiple of `sample_every` and is what a float64 tape holds.  `window` is a number of steps (a window closes after
        every step that leaves current_step at a multiple of it), "day" (at 00:00) or "month" (at 00:00 on day 1 of the model's
        calendar); the ring in device memory keeps the last `capacity` windows of every member; dtype "float32" (the default) or
        "float64".  The first window starts at the current step and may be short (wintape_counts()); a window without a sample
        holds 0 for sums and counts and NaN otherwise.  Empties the ring; an empty list switches the recorder off and frees it.
        Synchronises the device."""
        key = str(dtype).replace("torch.", "")
        if key not in self.TAPE_DTYPES:
            raise ValueError("dtype must be 'float32' or 'float64', got %r" % (dtype,))
        if isinstance(window, str):
            if window not in self.WINTAPE_WINDOWS:
                raise ValueError("window must be a number of steps, 'day' or 'month', got %r" % (window,))
            kind, every = self.WINTAPE_WINDOWS[window], 0
        else:
            kind, every = _lib.SPD_WINDOW_STEPS, int(window)
        rows = []
        for entry in entries:
            if len(entry) not in (2, 3):
                raise ValueError("an entry is (name, op) or (name, op, threshold), got %r" % (entry,))
            op = self._wintape_op(entry[1])
            counts = op in (_lib.SPD_WIN_COUNT_ABOVE, _lib.SPD_WIN_COUNT_BELOW)
            if counts and len(entry) != 3:
                raise ValueError("op %r needs a threshold: (name, op, threshold)" % (entry[1],))
            rows.append((str(entry[0]), op, float(entry[2]) if counts else 0.0))
        names, ops = _c_names(r[0] for r in rows), _c_array(C.c_int, (r[1] for r in rows))
        thresholds = _c_array(C.c_double, (r[2] for r in rows))
        with torch.cuda.device(self.sp.device):
            check(self._lib.spd_model_wintape_configure(self._m, names, ops, thresholds, len(rows), kind, every, int(sample_every),
                                                        int(capacity), self.TAPE_DTYPES[key][0]), "spd_model_wintape_configure")

    def wintape_reset(self):
        """Empty the ring and start a new window at the current step (no device work)."""
        check(self._lib.spd_model_wintape_reset(self._m), "spd_model_wintape_reset")

    @property
    def wintape_info(self):
        """dict(taken, held, capacity, window, sample_every, dtype): windows closed since the last reset, windows the ring holds
        (min(taken, capacity)), and the configuration (window: the number of steps, "day" or "month")."""
        taken, held, capacity, kind, every, sample_every, dtype = (C.c_longlong(0), C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0),
                                                                   C.c_int(0), C.c_int(0))
        check(self._lib.spd_model_wintape_info(self._m, C.byref(taken), C.byref(held), C.byref(capacity), C.byref(kind), C.byref(every),
                                               C.byref(sample_every), C.byref(dtype)), "spd_model_wintape_info")
        name = [k for k, v in self.TAPE_DTYPES.items() if v[0] == dtype.value][0]
        window = every.value if kind.value == _lib.SPD_WINDOW_STEPS else [k for k, v in self.WINTAPE_WINDOWS.items() if v == kind.value][0]
        return dict(taken=int(taken.value), held=held.value, capacity=capacity.value, window=window, sample_every=sample_every.value,
                    dtype=name)

    def _wintape_rows(self):
        return self._ring_rows("spd_model_wintape_times", self.wintape_info["held"], 8)

    def wintape_steps(self):
        """The model's step counter after the last step of each held window, oldest first (numpy int array)."""
        return self._row_steps(self._wintape_rows())

    def wintape_times(self):
        """The date of the state after each held window's last step, oldest first (a list of datetime)."""
        return self._row_times(self._wintape_rows())

    def wintape_counts(self):
        """(samples, steps) in each held window, oldest first (two numpy int arrays)."""
        rows = self._wintape_rows()
        return rows[:, 6].astype(np.int64), rows[:, 7].astype(np.int64)

    def wintape(self, name, op, first=0, count=None, t0=0, nt=None):
        """Members [first, first + count) and windows [t0, t0 + nt) of the held ones (oldest first) of one entry: a tensor
        [count][nt][levels][48][96] ([count][nt][48][96] for one-level names) on the model's device in the ring's dtype."""
        first, count = self._range(first, count)
        info = self.wintape_info
        t0, nt = _held_span(info, t0, nt)
        dtype = self.TAPE_DTYPES[info["dtype"]][1]
        shape = self._stats_shape({"wspd_grid": "u_grid", "wspd_plev": "u_plev"}.get(name, name))
        out = torch.empty((count, max(nt, 0)) + shape, dtype=dtype, device=self.sp.device)
        with torch.cuda.device(self.sp.device):
            check(self._lib.spd_model_wintape_read(self._m, name.encode(), self._wintape_op(op), first, count, t0, nt,
                                                   C.c_void_p(out.data_ptr()), out.numel() * out.element_size(), self._stream()),
                  "spd_model_wintape_read(%s, %s)" % (name, op))
        return out

    # ---- the projection tape: weighted sums of fields as scalar series (spd_model_projtape_*, include/pyspeedy_amd.h) --------
    def projtape_configure(self, weights, entries, every, capacity):
        """Record scalar series taken from grid-space fields inside run() / run_checked() calls of any length.  `weights` is
        array-like [P][48][96] (1 <= P <= 64, finite), weight maps in the layout of one level of a tape sample
        (pyspeedy_amd.projection_weights builds global means, boxes, bands and station stencils); `entries` is a list of
        (name, level, pattern): name any of STATS_VARIABLES (the pressure-level ones after plev_configure), level a 0-based level
        of that name, pattern an index into `weights`.  After every step that leaves current_step at a multiple of `every`, each
        entry's sum over the 4608 points of weight times the value a float64 tape holds is formed on the device in a fixed,
        documented order and kept for every member in a ring of the last `capacity` samples.  Empties the
        ring; an empty list switches the recorder off and frees it.  Synchronises the device."""
        rows = _pattern_rows(entries)
        w = _weight_maps(weights, checked=bool(rows))
        names, levels = _c_names(r[0] for r in rows), _c_array(C.c_int, (r[1] for r in rows))
        patterns = _c_array(C.c_int, (r[2] for r in rows))
        with torch.cuda.device(self.sp.device):
            rc = self._lib.spd_model_projtape_configure(self._m, w.ctypes.data_as(C.POINTER(C.c_double)), w.shape[0] if rows else 0, names,
                                                        levels, patterns, len(rows), int(every), int(capacity))
        if rc != 0:
            off = lambda: self._lib.spd_model_projtape_info(self._m, None, None, None, None, None, None) != 0  # noqa: E731
            self._configure_refused("spd_model_projtape_configure", rc, off, "_projtape_entries")
        self._projtape_entries = tuple(rows)

    def projtape_reset(self):
        """Empty the projection tape (no device work); the next sample is the first."""
        check(self._lib.spd_model_projtape_reset(self._m), "spd_model_projtape_reset")

    @property
    def projtape_info(self):
        """dict(taken, held, capacity, every, patterns, entries): samples since the last reset, samples the ring holds (min(taken,
        capacity)), and the configuration."""
        taken, held, capacity, every, patterns, entries = C.c_longlong(0), C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
        check(self._lib.spd_model_projtape_info(self._m, C.byref(taken), C.byref(held), C.byref(capacity), C.byref(every),
                                                C.byref(patterns), C.byref(entries)), "spd_model_projtape_info")
        return dict(taken=int(taken.value), held=held.value, capacity=capacity.value, every=every.value, patterns=patterns.value,
                    entries=entries.value)

    @property
    def projtape_entries(self):
        """The configured entries, a tuple of (name, level, pattern) in the order of the last axis of projtape() (empty: off)."""
        return getattr(self, "_projtape_entries", ())

    def _projtape_rows(self):
        return self._ring_rows("spd_model_projtape_times", self.projtape_info["held"], 6)

    def projtape_steps(self):
        """The model's step counter after each held sample's step, oldest first (numpy int array)."""
        return self._row_steps(self._projtape_rows())

    def projtape_times(self):
        """The date of each held sample's state, oldest first (a list of datetime)."""
        return self._row_times(self._projtape_rows())

    def projtape(self, first=0, count=None, t0=0, nt=None):
        """Members [first, first + count) and samples [t0, t0 + nt) of the held ones (oldest first) of every entry: a float64
        tensor [count][nt][E] on the model's device, E in the order of projtape_entries."""
        first, count = self._range(first, count)
        info = self.projtape_info
        t0, nt = _held_span(info, t0, nt)
        out = torch.empty((count, max(nt, 0), info["entries"]), dtype=torch.float64, device=self.sp.device)
        with torch.cuda.device(self.sp.device):
            check(self._lib.spd_model_projtape_read(self._m, first, count, t0, nt, C.c_void_p(out.data_ptr()), out.numel() * 8,
                                                    self._stream()), "spd_model_projtape_read")
        return out

    # ---- the track tape: extremes of fields over regions and their positions (spd_model_tracktape_*, include/pyspeedy_amd.h) --
    TRACK_OPS = {"min": _lib.SPD_TRACK_MIN, "max": _lib.SPD_TRACK_MAX}

    def tracktape_configure(self, regions, entries, every, capacity):
        """Record the minimum or maximum of grid-space fields over regions, and where it lies, inside run() / run_checked() calls
        of any length.  `regions` is array-like [R][48][96] (1 <= R <= 64, finite): the projection tape's weight maps
        (pyspeedy_amd.projection_weights), a point belongs to a region where its weight is not zero; `entries` is a list of
        (name, level, region, op, radius): name and level as projtape_configure takes them, region an index into `regions`, op
        "min" or "max" (or SPD_TRACK_MIN / SPD_TRACK_MAX), radius 0 ... 24 grid points.  After every step that leaves
        current_step at a multiple of `every`, each entry's extreme over its region of the plane a float64 tape holds is found on
        the device for every member and kept as (value, p, di, dj) in a ring of the last `capacity` samples: p = 96 j + i the
        winner's point (the lowest among equal values; -1 and NaN where every value of the region is NaN), di and dj sub-grid
        offsets in [-0.5, 0.5] from the parabola through its neighbours.  An entry with radius > 0 follows its
        feature: once it holds a position (its last winner, or a seed: tracktape_seed), it looks only at the points of the region
        within `radius` rows and columns of it.  Empties the ring and un-seeds; an empty list switches the recorder off and frees
        it.  Synchronises the device."""
        rows = []
        for entry in entries:
            if len(entry) != 5:
                raise ValueError("an entry is (name, level, region, op, radius), got %r" % (entry,))
            op = entry[3]
            if isinstance(op, str):
                if op not in self.TRACK_OPS:
                    raise ValueError("op must be one of %s, got %r" % (", ".join(self.TRACK_OPS), op))
                op = self.TRACK_OPS[op]
            rows.append((str(entry[0]), int(entry[1]), int(entry[2]), int(op), int(entry[4])))
        w = _weight_maps(regions, checked=bool(rows))
        names = _c_names(r[0] for r in rows)
        levels, region_of, ops, radii = (_c_array(C.c_int, (r[k] for r in rows)) for k in (1, 2, 3, 4))
        with torch.cuda.device(self.sp.device):
            rc = self._lib.spd_model_tracktape_configure(self._m, w.ctypes.data_as(C.POINTER(C.c_double)), w.shape[0] if rows else 0, names,
                                                         levels, region_of, ops, radii, len(rows), int(every), int(capacity))
        if rc != 0:
            off = lambda: self._lib.spd_model_tracktape_info(self._m, None, None, None, None, None, None) != 0  # noqa: E731
            self._configure_refused("spd_model_tracktape_configure", rc, off, "_tracktape_entries")
        self._tracktape_entries = tuple(rows)

    def tracktape_off(self):
        """Switch the track tape off and free it (no-op when it is off)."""
        self.tracktape_configure([], [], 0, 0)

    def tracktape_reset(self):
        """Empty the track tape and un-seed it: the next sample is the first, and every entry looks at its whole region."""
        with torch.cuda.device(self.sp.device):
            check(self._lib.spd_model_tracktape_reset(self._m), "spd_model_tracktape_reset")

    @property
    def tracktape_info(self):
        """dict(taken, held, capacity, every, regions, entries): samples since the last reset, samples the ring holds (min(taken,
        capacity)), and the configuration."""
        taken, held, capacity, every, regions, entries = C.c_longlong(0), C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
        check(self._lib.spd_model_tracktape_info(self._m, C.byref(taken), C.byref(held), C.byref(capacity), C.byref(every),
                                                 C.byref(regions), C.byref(entries)), "spd_model_tracktape_info")
        return dict(taken=int(taken.value), held=held.value, capacity=capacity.value, every=every.value, regions=regions.value,
                    entries=entries.value)

    @property
    def tracktape_entries(self):
        """The configured entries, a tuple of (name, level, region, op, radius) with op as SPD_TRACK_MIN / SPD_TRACK_MAX, in the
        order of tracktape()'s entry axis (empty: off)."""
        return getattr(self, "_tracktape_entries", ())

    def _tracktape_rows(self):
        return self._ring_rows("spd_model_tracktape_times", self.tracktape_info["held"], 6)

    def tracktape_steps(self):
        """The model's step counter after each held sample's step, oldest first (numpy int array)."""
        return self._row_steps(self._tracktape_rows())

    def tracktape_times(self):
        """The date of each held sample's state, oldest first (a list of datetime)."""
        return self._row_times(self._tracktape_rows())

    def tracktape(self, first=0, count=None, t0=0, nt=None):
        """Members [first, first + count) and samples [t0, t0 + nt) of the held ones (oldest first) of every entry: a float64
        tensor [count][nt][E][4] on the model's device, E in the order of tracktape_entries, the last axis (value, p, di, dj)."""
        first, count = self._range(first, count)
        info = self.tracktape_info
        t0, nt = _held_span(info, t0, nt)
        out = torch.empty((count, max(nt, 0), info["entries"], 4), dtype=torch.float64, device=self.sp.device)
        with torch.cuda.device(self.sp.device):
            check(self._lib.spd_model_tracktape_read(self._m, first, count, t0, nt, C.c_void_p(out.data_ptr()), out.numel() * 8,
                                                     self._stream()), "spd_model_tracktape_read")
        return out

    def tracktape_positions(self, first=0, count=None):
        """The follow-state of members [first, first + count): a numpy int32 array [count][E] of points p = 96 j + i, -1 where an
        entry follows nothing.  Synchronises the device."""
        first, count = self._range(first, count)
        out = np.full((count, self.tracktape_info["entries"]), -1, dtype=np.int32)
        with torch.cuda.device(self.sp.device):
            n = self._lib.spd_model_tracktape_positions(self._m, first, count, out.ctypes.data_as(C.POINTER(C.c_int32)), out.size)
        if n < 0:
            check(n, "spd_model_tracktape_positions")
        return out

    def tracktape_seed(self, positions, first=0):
        """Set the follow-state of the members from `first` on: `positions` is array-like [count][E] of points p = 96 j + i inside
        each entry's region, or -1 (follow nothing until the next sample).  Seeding picks WHICH low an entry with radius > 0
        follows.  Synchronises the device."""
        src = np.ascontiguousarray(positions, dtype=np.int32)
        if src.ndim != 2 or src.shape[1] != self.tracktape_info["entries"]:
            raise ValueError("positions must be [count][%d], got shape %r" % (self.tracktape_info["entries"], src.shape))
        with torch.cuda.device(self.sp.device):
            check(self._lib.spd_model_tracktape_seed(self._m, int(first), src.shape[0], src.ctypes.data_as(C.POINTER(C.c_int32))),
                  "spd_model_tracktape_seed")

    @staticmethod
    def tracktape_lonlat(track):
        """(lon, lat) in degrees of tracktape()'s output (a tensor or array [..., 4]): lon = 3.75 (i + di) mod 360, lat linear
        between the winner's row of ProjectionWeights.lat and the neighbouring row in the direction of dj, by |dj|.  NaN where
        nothing was found (p = -1)."""
        track = track.cpu().numpy() if torch.is_tensor(track) else np.asarray(track, dtype=np.float64)
        lats = _lib.projection_weights().lat
        p, di, dj = track[..., 1], track[..., 2], track[..., 3]
        found = p >= 0
        at = np.where(found, p, 0).astype(np.int64)
        j, i = at // 96, at % 96
        lon = np.mod(3.75 * (i + di), 360.0)
        toward = np.clip(j + np.where(dj < 0, -1, 1), 0, 47)
        lat = lats[j] + np.abs(dj) * (lats[toward] - lats[j])
        return np.where(found, lon, np.nan), np.where(found, lat, np.nan)

    # ---- the filter tape: window means and covariances of time-filtered fields (spd_model_filtape_*, include/pyspeedy_amd.h) --
    FILTAPE_OPS = {"mean": _lib.SPD_FIL_MEAN, "cov": _lib.SPD_FIL_COV, "last": _lib.SPD_FIL_LAST}

    def _filtape_level(self, name, level):
        """the 0-based level of an entry: a name on the target levels of plev_configure gives its level in hPa"""
        if name in self.PLEV_VARIABLES[:5] or name in self.DERIVED_VARIABLES[9:]:
            levels = self.plev_levels
            if float(level) not in levels:
                raise ValueError("%r is not among the configured pressure levels %r (hPa) of %s" % (level, levels, name))
            return levels.index(float(level))
        return int(level)

    def filtape_configure(self, filters, entries, window, capacity, sample_every=1, spinup=0, dtype="float32"):
        """Record window means, covariances and last values of time-filtered fields inside run() / run_checked() calls of any
        length: the band-passed variance of z_plev at 500 hPa (the storm track), eddy fluxes such as v'T' at 850 hPa, the variance
        of a low-passed field.  `filters` is a list of 1 ... 8 cascades, each array-like [S][5] (1 <= S <= 4) of second-order
        sections (b0, b1, b2, a1, a2) as pyspeedy_amd.butterworth_sections returns them, with the sampling interval `sample_every`
        steps of 40 minutes.  `entries` is a list (at most 64) of (name, level, filter, op) or (name, level, filter, "cov", name_b,
        level_b): name any of STATS_VARIABLES or DERIVED_VARIABLES, level a 0-based level of the name -- for a name on the target
        levels of plev_configure the level itself in hPa --, filter an index into `filters`, op "mean" (the window mean of the
        filtered field), "cov" (the window mean of the product of two filtered fields, the variance of one when no second field is
        named; a moment about zero: subtract the product of two "mean" entries where the filter passes the mean) or "last" (the
        filtered field at the window's last counted sample).  A sample is taken after every step that leaves current_step at a
        multiple of `sample_every` and is what a float64 tape holds; the first `spinup` samples run the filters and are counted
        in no window.  `window` is a number of steps, "day" or "month" as wintape_configure takes it (wintape_plan tells the
        windows ahead); the ring in device memory keeps the last `capacity` windows of every member; dtype "float32" (the
        default) or "float64".  A window without a counted sample holds NaN.  The arithmetic is fixed.  Empties
        the ring and restarts the filters.  Synchronises the device."""
        key = str(dtype).replace("torch.", "")
        if key not in self.TAPE_DTYPES:
            raise ValueError("dtype must be 'float32' or 'float64', got %r" % (dtype,))
        if isinstance(window, str):
            if window not in self.WINTAPE_WINDOWS:
                raise ValueError("window must be a number of steps, 'day' or 'month', got %r" % (window,))
            kind, every = self.WINTAPE_WINDOWS[window], 0
        else:
            kind, every = _lib.SPD_WINDOW_STEPS, int(window)
        cascades = [np.ascontiguousarray(f, dtype=np.float64) for f in filters]
        for f in cascades:
            if f.ndim != 2 or f.shape[1] != 5:
                raise ValueError("a filter is [S][5] (b0, b1, b2, a1, a2 per section), got shape %r" % (f.shape,))
        rows = []
        for entry in entries:
            if len(entry) not in (4, 6):
                raise ValueError("an entry is (name, level, filter, op) or (name, level, filter, op, name_b, level_b), got %r" % (entry,))
            op = entry[3]
            if isinstance(op, str):
                if op not in self.FILTAPE_OPS:
                    raise ValueError("op must be one of 'mean', 'cov', 'last', got %r" % (op,))
                op = self.FILTAPE_OPS[op]
            second = (str(entry[4]), self._filtape_level(str(entry[4]), entry[5])) if len(entry) == 6 else ("", 0)
            rows.append((str(entry[0]), self._filtape_level(str(entry[0]), entry[1]), int(entry[2]), int(op)) + second)
        flat = np.concatenate(cascades) if cascades else np.zeros((1, 5))
        counts = _c_array(C.c_int, (f.shape[0] for f in cascades))
        names_a, names_b = _c_names(r[0] for r in rows), _c_names(r[4] for r in rows)
        levels_a, which, ops, levels_b = (_c_array(C.c_int, (r[k] for r in rows)) for k in (1, 2, 3, 5))
        with torch.cuda.device(self.sp.device):
            rc = self._lib.spd_model_filtape_configure(self._m, flat.ctypes.data_as(C.POINTER(C.c_double)), counts, len(cascades), names_a,
                                                       levels_a, which, ops, names_b, levels_b, len(rows), kind, every, int(sample_every),
                                                       int(spinup), int(capacity), self.TAPE_DTYPES[key][0])
        if rc != 0:
            off = lambda: self._lib.spd_model_filtape_info(self._m, *([None] * 12)) != 0  # noqa: E731
            self._configure_refused("spd_model_filtape_configure", rc, off, "_filtape_entries")
        self._filtape_entries = tuple(rows)

    def filtape_off(self):
        """Switch the filter tape off and free it."""
        with torch.cuda.device(self.sp.device):
            check(self._lib.spd_model_filtape_off(self._m), "spd_model_filtape_off")
        self._filtape_entries = ()

    def filtape_reset(self):
        """Empty the ring, start a new window at the current step and restart the filters: the next sample starts every section
        in the steady state of its value (no device work)."""
        check(self._lib.spd_model_filtape_reset(self._m), "spd_model_filtape_reset")

    @property
    def filtape_info(self):
        """dict(taken, held, capacity, window, sample_every, spinup, dtype, filters, planes, entries, filter_samples): windows
        closed since the last reset, windows the ring holds (min(taken, capacity)), the configuration (window: the number of steps,
        "day" or "month"; planes: distinct filtered (name, level, filter) planes) and the filter samples taken since the filters
        last started."""
        taken, k = C.c_longlong(0), C.c_longlong(0)
        v = [C.c_int(0) for _ in range(10)]
        check(self._lib.spd_model_filtape_info(self._m, C.byref(taken), *[C.byref(x) for x in v], C.byref(k)), "spd_model_filtape_info")
        held, capacity, kind, every, sample_every, spinup, dtype, filters, planes, entries = (x.value for x in v)
        name = [key for key, val in self.TAPE_DTYPES.items() if val[0] == dtype][0]
        window = every if kind == _lib.SPD_WINDOW_STEPS else [key for key, val in self.WINTAPE_WINDOWS.items() if val == kind][0]
        return dict(taken=int(taken.value), held=held, capacity=capacity, window=window, sample_every=sample_every, spinup=spinup,
                    dtype=name, filters=filters, planes=planes, entries=entries, filter_samples=int(k.value))

    @property
    def filtape_entries(self):
        """The configured entries, a tuple of (name, level, filter, op, name_b, level_b) with 0-based levels, op as SPD_FIL_* and
        name_b "" where there is none, in the order filtape() numbers them (empty: off)."""
        return getattr(self, "_filtape_entries", ())

    def _filtape_rows(self):
        return self._ring_rows("spd_model_filtape_times", self.filtape_info["held"], 8)

    def filtape_steps(self):
        """The model's step counter after the last step of each held window, oldest first (numpy int array)."""
        return self._row_steps(self._filtape_rows())

    def filtape_times(self):
        """The date of the state after each held window's last step, oldest first (a list of datetime)."""
        return self._row_times(self._filtape_rows())

    def filtape_counts(self):
        """(counted samples, steps) in each held window, oldest first (two numpy int arrays)."""
        rows = self._filtape_rows()
        return rows[:, 6].astype(np.int64), rows[:, 7].astype(np.int64)

    def filtape(self, entry, first=0, count=None, t0=0, nt=None):
        """Members [first, first + count) and windows [t0, t0 + nt) of the held ones (oldest first) of entry number `entry` of
        filtape_entries: a tensor [count][nt][48][96] on the model's device in the ring's dtype."""
        first, count = self._range(first, count)
        info = self.filtape_info
        t0, nt = _held_span(info, t0, nt)
        out = torch.empty((count, max(nt, 0), 48, 96), dtype=self.TAPE_DTYPES[info["dtype"]][1], device=self.sp.device)
        with torch.cuda.device(self.sp.device):
            check(self._lib.spd_model_filtape_read(self._m, int(entry), first, count, t0, nt, C.c_void_p(out.data_ptr()),
                                                   out.numel() * out.element_size(), self._stream()), "spd_model_filtape_read(%d)" % int(entry))
        return out

    # ---- nudging: relaxation of the spectral state toward target fields (spd_model_nudge_*, include/pyspeedy_amd.h) ---------
    NUDGE_NAMES = ("vor", "div", "t", "tr", "ps")

    def nudge_configure(self, gains, members=None, capacity=2, in_loop=True):
        """Relax the spectral state toward target fields: after every step of run() / run_checked() (`in_loop`) or only when
        nudge_apply() is called.  `gains` maps a name of NUDGE_NAMES to an array (levels, 32) of gains in [0, 1] by level and
        total wavenumber ((32,) or (1, 32) for ps; pyspeedy_amd.nudge_gains builds one from a time scale): X' = X + g (T - X) on
        both time levels for m + n <= 31, every operation rounded on its own.  `members`: a mask of 0 / 1 (or bools) per member,
        None for all.  `capacity` target slots, zero-filled and shared by all members, are allocated; nudge_targets fills and
        stamps them.  An empty dict switches nudging off.  While in-loop nudging with a gain that is not zero is configured the
        geopotential look-ahead of small ensembles is off (config()["fold_geo"]).  Synchronises the device."""
        names = [str(n) for n in gains]
        table = np.zeros((max(len(names), 1), 8, 32))
        for k, n in enumerate(names):
            g = np.asarray(gains[n], dtype=np.float64)
            rows = 1 if n == "ps" else 8
            if n == "ps" and g.shape == (32,):
                g = g.reshape(1, 32)
            if n in self.NUDGE_NAMES and g.shape != (rows, 32):
                raise ValueError("gains of %s must have the shape (%d, 32), got %s" % (n, rows, g.shape))
            table[k, :g.shape[0]] = g
        mask = None if members is None else self._member_mask(members)
        arr = _c_names(names)
        with torch.cuda.device(self.sp.device):
            check(self._lib.spd_model_nudge_configure(self._m, arr, len(names), table.ctypes.data_as(C.POINTER(C.c_double)),
                                                      None if mask is None else mask.ctypes.data_as(C.POINTER(C.c_int32)),
                                                      int(capacity), int(bool(in_loop))), "spd_model_nudge_configure")

    def nudge_off(self):
        """Switch nudging off and free its slots."""
        self.nudge_configure({})

    def _nudge_step(self, when):
        """absolute step counter of a datetime, from the model's current date and step at 40 minutes per step"""
        from datetime import datetime, timedelta
        if not isinstance(when, datetime):
            return int(when)
        delta = when - datetime(*self.current_date)
        steps, rest = divmod(delta, timedelta(minutes=40))
        if rest:
            raise ValueError("%s is not a whole number of 40-minute steps from the model's date" % (when,))
        return self.current_step + int(steps)

    def nudge_targets(self, times, fields):
        """Fill the first len(times) target slots and declare them in use.  `times`: strictly ascending absolute step counters or
        datetimes (converted with the model's current date and step, 40 minutes per step).  `fields` maps every configured name
        to a complex array (n, 31, 32, 8) ((n, 31, 32) for ps) in the state's stored units, as get() returns a time level.
        Between two stamps the target is interpolated linearly; before the first and after the last it is held."""
        stamps = np.asarray([self._nudge_step(t) for t in times], dtype=np.int32)
        for name, value in fields.items():
            shape = (len(stamps), 31, 32) + (() if name == "ps" else (8,))
            a = np.asarray(value, dtype=np.complex128)
            if a.shape != shape:
                raise ValueError("Array shape missmatch: targets of %s expect %s, got %s" % (name, shape, a.shape))
            for slot in range(len(stamps)):
                flat = np.ascontiguousarray(a[slot].ravel(order="F"))
                check(self._lib.spd_model_nudge_set_target(self._m, slot, str(name).encode(), flat.ctypes.data_as(C.c_void_p),
                                                           flat.nbytes), "spd_model_nudge_set_target(%s)" % name)
        check(self._lib.spd_model_nudge_set_times(self._m, stamps.ctypes.data_as(C.POINTER(C.c_int32)), len(stamps)),
              "spd_model_nudge_set_times")

    def nudge_apply(self, first=0, count=None):
        """The nudging launch once, on the state as it stands, at the current step counter, for members [first, first + count)
        (of which the masked ones move); asynchronous on the current stream."""
        check(self._lib.spd_model_nudge_apply(self._m, *self._range(first, count), self._stream()), "spd_model_nudge_apply")

    def nudge_info(self):
        """dict(names, capacity, in_use, in_loop, applied): the number of configured names (0: off), the slots allocated and in use,
        the mode, and the steps nudged since nudge_configure."""
        n, capacity, in_use, in_loop, applied = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0), C.c_longlong(0)
        check(self._lib.spd_model_nudge_info(self._m, C.byref(n), C.byref(capacity), C.byref(in_use), C.byref(in_loop),
                                             C.byref(applied)), "spd_model_nudge_info")
        return dict(names=n.value, capacity=capacity.value, in_use=in_use.value, in_loop=bool(in_loop.value), applied=int(applied.value))

    # ---- breeding: member perturbations rescaled against their control runs (spd_model_breed_*, include/pyspeedy_amd.h) ------
    BREED_NAMES = ("vor", "div", "t", "tr", "ps")

    def breed_configure(self, control, target, every, weights="kinetic_energy", capacity=64, in_loop=True, orthogonalize=False):
        """Breed perturbations: after every step that leaves current_step at a multiple of `every`, inside run() / run_checked()
        calls of any length (`in_loop`) or only when breed_apply() is called, every bred member p is pulled back to the distance
        `target` from its control c: X_p' = X_c + s (X_p - X_c), s = target / A, on both time levels of vor, div, t, tr, ps for
        m + n <= 31, every operation rounded on its own.  `control`: one entry per member, the index of its control run or -1 for
        a member that is not bred (a control must itself have -1).  `weights`: a kind of pyspeedy_amd.breed_weights, or a dict
        name of BREED_NAMES -> (8,) weights >= 0 of the quadratic forms that make A^2 (names left out weigh nothing; ps reads
        entry 0).  Every rescale writes the amplitudes before it and the factors to a ring of `capacity` events (breed()).  Land and
        sea temperatures are not rescaled.  `orthogonalize`: breed_orthogonalize() behind the configuration.  Synchronises the
        device."""
        from ._lib import breed_weights
        ctl = np.ascontiguousarray(np.asarray(control).astype(np.int32))
        if ctl.shape != (self.nmembers,):
            raise ValueError("control must have one entry per member (%d), got shape %s" % (self.nmembers, ctl.shape))
        table = self._breed_table(breed_weights(weights) if isinstance(weights, str) else weights)
        with torch.cuda.device(self.sp.device):
            check(self._lib.spd_model_breed_configure(self._m, ctl.ctypes.data_as(C.POINTER(C.c_int32)),
                                                      table.ctypes.data_as(C.POINTER(C.c_double)), float(target), int(every),
                                                      int(capacity), int(bool(in_loop))), "spd_model_breed_configure")
        if orthogonalize:
            self.breed_orthogonalize(True)

    def breed_orthogonalize(self, on=True):
        """Orthonormalised breeding on or off: with it on, every rescale (in-loop and breed_apply()) is the Gram-Schmidt cycle of
        each family -- the bred members p_1 < ... < p_r (r <= 64) that share a control.  With G the Gram matrix of their
        differences in the configured norm, G = R^T R and C = target R^-1 (upper triangular), member p_j becomes
        X_c + sum_{i <= j} C_ij (X_(p_i) - X_c) on both time levels: the perturbations leave orthonormal at `target`.  The ring
        holds amplitude = R_jj (what grew orthogonally to the earlier members) and factor = target / R_jj, so breed_growth() gives
        the local Lyapunov exponents, member by member in descending order.  A family breaks at a member whose perturbation has
        nothing left (or is not finite): that member and the later ones are left alone.  breed_off() and breed_configure() switch
        it off.  Synchronises the device."""
        with torch.cuda.device(self.sp.device):
            check(self._lib.spd_model_breed_orthogonalize(self._m, int(bool(on))), "spd_model_breed_orthogonalize")

    def breed_gram(self):
        """The Gram matrix of the perturbations on the state as it stands, in the configured norm: a float64 tensor
        [members][members] on the model's device; entry (a, b) is the inner product of the two members' differences against their
        control if both are bred with the same control, else 0.0.  Its diagonal is breed_amplitude() squared.  Writes neither the
        state nor the ring; works with orthogonalisation on or off."""
        out = torch.empty((self.nmembers, self.nmembers), dtype=torch.float64, device=self.sp.device)
        with torch.cuda.device(self.sp.device):
            check(self._lib.spd_model_breed_gram(self._m, C.c_void_p(out.data_ptr()), out.numel() * 8, self._stream()),
                  "spd_model_breed_gram")
        return out

    @classmethod
    def _breed_table(cls, weights):
        """dict name -> (8,) (a scalar or (1,) for ps) as the library's [5][8] table"""
        table = np.zeros((5, 8))
        for n, w in weights.items():
            if n not in cls.BREED_NAMES:
                raise ValueError("unknown variable '%s' in the breeding weights %s" % (n, cls.BREED_NAMES))
            w = np.atleast_1d(np.asarray(w, dtype=np.float64))
            rows = (1, 8) if n == "ps" else (8,)
            if w.ndim != 1 or w.shape[0] not in rows:
                raise ValueError("weights of %s must have the shape (8,), got %s" % (n, w.shape))
            table[cls.BREED_NAMES.index(n), :w.shape[0]] = w
        return table

    def breed_off(self):
        """Switch breeding off and free its ring."""
        with torch.cuda.device(self.sp.device):
            check(self._lib.spd_model_breed_configure(self._m, None, None, 0.0, 0, 0, 0), "spd_model_breed_configure")

    def breed_apply(self):
        """Rescale every bred member once, on the state as it stands; asynchronous on the current stream; writes a ring slot."""
        check(self._lib.spd_model_breed_apply(self._m, self._stream()), "spd_model_breed_apply")

    def breed_amplitude(self):
        """The amplitude A of every member's perturbation on the state as it stands (0.0 for members that are not bred): a float64
        tensor [members] on the model's device.  Writes neither the state nor the ring."""
        out = torch.empty(self.nmembers, dtype=torch.float64, device=self.sp.device)
        with torch.cuda.device(self.sp.device):
            check(self._lib.spd_model_breed_compute(self._m, C.c_void_p(out.data_ptr()), out.numel() * 8, self._stream()),
                  "spd_model_breed_compute")
        return out

    def breed_info(self):
        """dict(bred, every, capacity, taken, held, in_loop, applied): bred members (all zero: off), the configuration, events
        since breed_configure / breed_reset and events the ring holds, the mode, and the rescales launched since breed_configure.
        While orthogonalisation is on the dict also has orthogonalize (True), families and largest_family; a model with plain
        breeding reports exactly what it always did."""
        on, families, largest = C.c_int(0), C.c_int(0), C.c_int(0)
        check(self._lib.spd_model_breed_ortho_info(self._m, C.byref(on), C.byref(families), C.byref(largest)), "spd_model_breed_ortho_info")
        bred, every, capacity, in_loop = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
        taken, applied = C.c_longlong(0), C.c_longlong(0)
        check(self._lib.spd_model_breed_info(self._m, C.byref(bred), C.byref(every), C.byref(capacity), C.byref(taken), C.byref(in_loop),
                                             C.byref(applied)), "spd_model_breed_info")
        info = dict(bred=bred.value, every=every.value, capacity=capacity.value, taken=int(taken.value),
                    held=int(min(taken.value, capacity.value)), in_loop=bool(in_loop.value), applied=int(applied.value))
        if on.value:
            info.update(orthogonalize=True, families=families.value, largest_family=largest.value)
        return info

    def breed_reset(self):
        """Empty the ring of breeding events (no device work)."""
        check(self._lib.spd_model_breed_reset(self._m), "spd_model_breed_reset")

    def breed(self, t0=0, nt=None):
        """The events [t0, t0 + nt) of the held ones, oldest first: dict(amplitude, factor) of float64 tensors [nt][members] on
        the model's device -- the A before each rescale (0.0 for members that are not bred) and the s (1.0 for those)."""
        t0, nt = _held_span(self.breed_info(), t0, nt)
        out = {}
        with torch.cuda.device(self.sp.device):
            for what, name in enumerate(("amplitude", "factor")):
                buf = torch.empty((max(nt, 0), self.nmembers), dtype=torch.float64, device=self.sp.device)
                check(self._lib.spd_model_breed_read(self._m, what, t0, nt, C.c_void_p(buf.data_ptr()), buf.numel() * 8, self._stream()),
                      "spd_model_breed_read(%s)" % name)
                out[name] = buf
        return out

    def _breed_rows(self):
        return self._ring_rows("spd_model_breed_rows", self.breed_info()["held"], 6)

    def breed_steps(self):
        """The model's step counter at each held event, oldest first (numpy int array)."""
        return self._row_steps(self._breed_rows())

    def breed_times(self):
        """The date of each held event's state, oldest first (a list of datetime)."""
        return self._row_times(self._breed_rows())

    def breed_growth(self):
        """Growth rates [1/s] of the held events: a float64 numpy array [events][members] of ln(A_k / A'_(k-1)) / dt, with
        A'_(k-1) = s_(k-1) A_(k-1) the amplitude the event before left behind (the target, unless that member was left alone) and
        dt the time between the two events (2400 s per step).  NaN for the first held event and for members that are not bred."""
        got = self.breed()
        a, s = got["amplitude"].cpu().numpy(), got["factor"].cpu().numpy()
        steps = self.breed_steps()
        out = np.full(a.shape, np.nan)
        if len(steps) > 1:
            dt = 2400.0 * np.diff(steps)[:, None]
            with np.errstate(divide="ignore", invalid="ignore"):
                out[1:] = np.log(a[1:] / (a[:-1] * s[:-1])) / dt
        return out

    def breed_exponents(self, skip=1):
        """The time mean of breed_growth() over the held events but the first `skip`, per member, in 1/day: with orthogonalisation
        on, the leading Lyapunov exponents of the control's trajectory (the first member of a family carries the largest).  Host
        arithmetic; events without a growth rate (NaN) are left out, a member without any gives NaN."""
        g = self.breed_growth()[max(int(skip), 0):]
        ok = np.isfinite(g)
        n = ok.sum(axis=0)
        with np.errstate(divide="ignore", invalid="ignore"):
            return 86400.0 * np.where(ok, g, 0.0).sum(axis=0) / np.where(n > 0, n, np.nan)

    # ---- assimilation: a serial ensemble square-root filter in the device loop (spd_model_assim_*, include/pyspeedy_amd.h) ----
    def assim_configure(self, weights, entries, members, every, capacity=64, inflation=1.0, in_loop=True):
        """Assimilate observations: after every step that leaves current_step at a multiple of `every` AND for which
        assim_observations() holds a row, inside run() / run_checked() calls of any length (`in_loop`) or only when assim_apply()
        is called, the members with mask 1 are corrected by a serial ensemble square-root filter.  `weights`
        [P][48][96] and `entries` (name, level, pattern) are the projection tape's (pyspeedy_amd.projection_weights; precnv and
        precls are refused; at most 64 entries): each entry is one scalar observation operator.  `members`: a mask of 0 / 1 (or
        bools) per member with 2 ... 64 ones; a member with 0 -- a nature run -- is never touched.  `inflation` >= 1 multiplies
        the prior perturbations.  Every executed event writes the prior mean, prior variance, innovation and a used flag of each
        entry to a ring of `capacity` events (assim()).  Land and sea temperatures are not updated.  Synchronises the device."""
        rows = _pattern_rows(entries)
        w = _weight_maps(weights)
        mask = self._member_mask(members)
        names, levels = _c_names(r[0] for r in rows), _c_array(C.c_int, (r[1] for r in rows))
        patterns = _c_array(C.c_int, (r[2] for r in rows))
        with torch.cuda.device(self.sp.device):
            check(self._lib.spd_model_assim_configure(self._m, w.ctypes.data_as(C.POINTER(C.c_double)), w.shape[0], names, levels, patterns,
                                                      len(rows), mask.ctypes.data_as(C.POINTER(C.c_int32)), int(every), int(capacity),
                                                      float(inflation), int(bool(in_loop))), "spd_model_assim_configure")

    def assim_off(self):
        """Switch assimilation off and free everything it holds."""
        with torch.cuda.device(self.sp.device):
            check(self._lib.spd_model_assim_off(self._m), "spd_model_assim_off")

    def assim_observations(self, steps, values, variances):
        """Replace the observation table: `steps` strictly ascending absolute step counters (or datetimes, converted with the
        model's current date and step), `values` [T][E] (NaN: missing) and `variances` [T][E] (finite, > 0; a scalar or [E] is
        broadcast) in the order of the configured entries.  An event runs only at a step that a row is stamped with."""
        stamps = np.ascontiguousarray([self._nudge_step(t) for t in steps], dtype=np.int32)
        entries = self.assim_info()["entries"]
        yo = np.ascontiguousarray(np.asarray(values, dtype=np.float64))
        if yo.shape != (len(stamps), entries):
            raise ValueError("values must be [%d][%d] (rows, configured entries), got shape %r" % (len(stamps), entries, yo.shape))
        var = np.ascontiguousarray(np.broadcast_to(np.asarray(variances, dtype=np.float64), yo.shape))
        as_double = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
        check(self._lib.spd_model_assim_set_observations(self._m, stamps.ctypes.data_as(C.POINTER(C.c_int32)), len(stamps), as_double(yo),
                                                         as_double(var), max(entries, 1)), "spd_model_assim_set_observations")

    def assim_apply(self):
        """The analysis once, on the state as it stands, with the row stamped with current_step (refused if there is none);
        asynchronous on the current stream; writes a ring slot."""
        check(self._lib.spd_model_assim_apply(self._m, self._stream()), "spd_model_assim_apply")

    def assim_compute(self):
        """The observation-space ensemble of the state as it stands: a float64 tensor [E][r] on the model's device, entry e of
        masked member a_i -- bit for bit what the projection tape records for that entry.  Writes neither the state nor the ring."""
        info = self.assim_info()
        out = torch.empty((info["entries"], info["members"]), dtype=torch.float64, device=self.sp.device)
        with torch.cuda.device(self.sp.device):
            check(self._lib.spd_model_assim_compute(self._m, C.c_void_p(out.data_ptr()), out.numel() * 8, self._stream()),
                  "spd_model_assim_compute")
        return out

    def assim_transform(self, members, W):
        """Mix members with a matrix of the caller's: member members[j] becomes sum_i W[i][j] X_(members[i]) on both time levels of
        vor, div, t, tr, ps for m + n <= 31, the sum in ascending i, every operation rounded on its own (the transform of the
        analysis; for a host-side ETKF or a resampling step).  `members`: up to 64 distinct member indices; `W`: finite
        [r][r].  Works with or without assim_configure().  Waits for the current stream once, then launches on it."""
        idx = np.ascontiguousarray(np.asarray(members).astype(np.int32))
        w = np.ascontiguousarray(W, dtype=np.float64)
        if idx.ndim != 1 or w.shape != (len(idx), len(idx)):
            raise ValueError("W must be [r][r] for r = len(members) = %d, got shape %r" % (len(idx), w.shape))
        with torch.cuda.device(self.sp.device):
            check(self._lib.spd_model_assim_transform(self._m, idx.ctypes.data_as(C.POINTER(C.c_int32)), len(idx),
                                                      w.ctypes.data_as(C.POINTER(C.c_double)), self._stream()), "spd_model_assim_transform")

    def assim_info(self):
        """dict(members, entries, every, capacity, taken, held, skipped, in_loop, applied): masked members r (all zero: off), the
        configuration, events executed since assim_configure / assim_reset and events the ring holds, in-loop events that found
        no row of observations, the mode, and the events executed since assim_configure."""
        r, entries, every, capacity, in_loop = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
        taken, skipped, applied = C.c_longlong(0), C.c_longlong(0), C.c_longlong(0)
        check(self._lib.spd_model_assim_info(self._m, C.byref(r), C.byref(entries), C.byref(every), C.byref(capacity), C.byref(taken),
                                             C.byref(skipped), C.byref(in_loop), C.byref(applied)), "spd_model_assim_info")
        return dict(members=r.value, entries=entries.value, every=every.value, capacity=capacity.value, taken=int(taken.value),
                    held=int(min(taken.value, capacity.value)), skipped=int(skipped.value), in_loop=bool(in_loop.value),
                    applied=int(applied.value))

    def assim_reset(self):
        """Empty the ring of assimilation events and the count of skipped ones (no device work)."""
        check(self._lib.spd_model_assim_reset(self._m), "spd_model_assim_reset")

    def assim(self, t0=0, nt=None):
        """The events [t0, t0 + nt) of the held ones, oldest first: dict(mean, variance, innovation, used) of float64 tensors
        [nt][E] on the model's device -- the prior ensemble mean and sample variance of each entry as the serial filter met it,
        the innovation yo - mean (0.0 for a missing observation) and 1.0 / 0.0 for an entry that was / was not used."""
        info = self.assim_info()
        t0, nt = _held_span(info, t0, nt)
        buf = torch.empty((max(nt, 0), info["entries"], 4), dtype=torch.float64, device=self.sp.device)
        with torch.cuda.device(self.sp.device):
            check(self._lib.spd_model_assim_read(self._m, t0, nt, C.c_void_p(buf.data_ptr()), buf.numel() * 8, self._stream()),
                  "spd_model_assim_read")
        return dict(mean=buf[:, :, 0], variance=buf[:, :, 1], innovation=buf[:, :, 2], used=buf[:, :, 3])

    def assim_weights(self):
        """The last executed event's mixing matrix and observation-space prior: dict(W, Y) of float64 tensors [r][r] and [E][r]
        on the model's device."""
        info = self.assim_info()
        w = torch.empty((64, 64), dtype=torch.float64, device=self.sp.device)
        y = torch.empty((info["entries"], info["members"]), dtype=torch.float64, device=self.sp.device)
        with torch.cuda.device(self.sp.device):
            check(self._lib.spd_model_assim_weights(self._m, C.c_void_p(w.data_ptr()), w.numel() * 8, C.c_void_p(y.data_ptr()), y.numel() * 8,
                                                    self._stream()), "spd_model_assim_weights")
        return dict(W=w[:info["members"], :info["members"]].contiguous(), Y=y)

    def _assim_rows(self):
        return self._ring_rows("spd_model_assim_rows", self.assim_info()["held"], 6)

    def assim_steps(self):
        """The model's step counter at each held event, oldest first (numpy int array)."""
        return self._row_steps(self._assim_rows())

    def assim_times(self):
        """The date of each held event's state, oldest first (a list of datetime)."""
        return self._row_times(self._assim_rows())

    # ---- the verification tape: scores of an ensemble against a truth member (spd_model_verif_*, include/pyspeedy_amd.h) -------
    def verif_configure(self, weights, entries, members, truth, every, capacity=64, in_loop=True):
        """Score the members with mask 1 in `members` (2 ... 64 of them) against the member `truth` (mask 0: a nature run in the
        same model) after every step that leaves current_step at a multiple of `every`, inside run() / run_checked() calls of any
        length (`in_loop`) or only when verif_apply() is called.  `weights` [P][48][96] and `entries` (name, level, pattern) are
        the projection tape's (pyspeedy_amd.projection_weights; up to 256 entries, precnv and precls included): per entry the
        weighted sums of the ensemble mean's error, its square, the ensemble variance and the CRPS, and the rank histogram over
        the points whose weight is not zero, each in a fixed, documented order, go to a ring of `capacity`
        events -- before and, where an in-loop analysis was applied at the same step, after it.  Writes nothing into the model.
        Synchronises the device."""
        rows = _pattern_rows(entries)
        w = _weight_maps(weights)
        mask = self._member_mask(members)
        names, levels = _c_names(r[0] for r in rows), _c_array(C.c_int, (r[1] for r in rows))
        patterns = _c_array(C.c_int, (r[2] for r in rows))
        with torch.cuda.device(self.sp.device):
            rc = self._lib.spd_model_verif_configure(self._m, w.ctypes.data_as(C.POINTER(C.c_double)), w.shape[0], names, levels, patterns,
                                                     len(rows), mask.ctypes.data_as(C.POINTER(C.c_int32)), int(truth), int(every),
                                                     int(capacity), int(bool(in_loop)))
        if rc != 0:
            self._configure_refused("spd_model_verif_configure", rc, lambda: self.verif_info()["members"] == 0, "_verif_entries")
        self._verif_entries = tuple(rows)

    def verif_off(self):
        """Switch the verification tape off and free everything it holds."""
        with torch.cuda.device(self.sp.device):
            check(self._lib.spd_model_verif_off(self._m), "spd_model_verif_off")
        self._verif_entries = ()

    def verif_reset(self):
        """Empty the ring of verification events (no device work)."""
        check(self._lib.spd_model_verif_reset(self._m), "spd_model_verif_reset")

    def verif_apply(self):
        """One event on the state as it stands: a ring slot whose first half holds the scores (the second reads NaN / -1);
        asynchronous on the current stream.  run(k); verif_apply() is what the in-loop mode does at a scheduled step."""
        check(self._lib.spd_model_verif_apply(self._m, self._stream()), "spd_model_verif_apply")

    def verif_compute(self):
        """The scores of the state as it stands, without touching the ring: dict(bias, mse, variance, crps) of float64 tensors
        [E] and hist, an int32 tensor [E][r + 2] (ranks 0 ... r, then the ties), on the model's device."""
        info = self.verif_info()
        scores = torch.empty((info["entries"], 4), dtype=torch.float64, device=self.sp.device)
        hist = torch.empty((info["entries"], 66), dtype=torch.int32, device=self.sp.device)
        with torch.cuda.device(self.sp.device):
            check(self._lib.spd_model_verif_compute(self._m, C.c_void_p(scores.data_ptr()), scores.numel() * 8, C.c_void_p(hist.data_ptr()),
                                                    hist.numel() * 4, self._stream()), "spd_model_verif_compute")
        return dict(bias=scores[:, 0], mse=scores[:, 1], variance=scores[:, 2], crps=scores[:, 3], hist=hist[:, :info["members"] + 2])

    def verif_info(self):
        """dict(members, truth, entries, every, capacity, taken, held, in_loop, applied): masked members r (0: off), the truth
        member (-1: off), the configuration, events recorded since verif_configure / verif_reset and events the ring holds, the
        mode, and the events recorded since verif_configure."""
        r, truth, entries, every, capacity, in_loop = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
        taken, applied = C.c_longlong(0), C.c_longlong(0)
        check(self._lib.spd_model_verif_info(self._m, C.byref(r), C.byref(truth), C.byref(entries), C.byref(every), C.byref(capacity),
                                             C.byref(taken), C.byref(in_loop), C.byref(applied)), "spd_model_verif_info")
        return dict(members=r.value, truth=truth.value, entries=entries.value, every=every.value, capacity=capacity.value,
                    taken=int(taken.value), held=int(min(taken.value, capacity.value)), in_loop=bool(in_loop.value),
                    applied=int(applied.value))

    @property
    def verif_entries(self):
        """The configured entries, a tuple of (name, level, pattern) in the order of the last axis of verif() (empty: off)."""
        return getattr(self, "_verif_entries", ())

    def _verif_rows(self):
        return self._ring_rows("spd_model_verif_rows", self.verif_info()["held"], 7)

    def verif_steps(self):
        """The model's step counter at each held event, oldest first (numpy int array)."""
        return self._row_steps(self._verif_rows())

    def verif_times(self):
        """The date of each held event's state, oldest first (a list of datetime)."""
        return self._row_times(self._verif_rows())

    def verif(self, t0=0, nt=None):
        """The events [t0, t0 + nt) of the held ones, oldest first: dict(bias, mse, variance, crps, rmse, spread) of float64
        tensors [nt][2][E] on the model's device -- axis 1 is the phase: 0 the state as the event found it (the background), 1 the
        state an in-loop analysis left at the same step (NaN where there was none) -- with rmse = sqrt(mse), spread =
        sqrt(variance), and analysis, an int32 tensor [nt]: 1 where phase 1 is filled."""
        info = self.verif_info()
        t0, nt = _held_span(info, t0, nt)
        buf = torch.empty((max(nt, 0), 2, info["entries"], 4), dtype=torch.float64, device=self.sp.device)
        with torch.cuda.device(self.sp.device):
            check(self._lib.spd_model_verif_read(self._m, t0, nt, C.c_void_p(buf.data_ptr()), buf.numel() * 8, self._stream()),
                  "spd_model_verif_read")
        rows = self._verif_rows()[t0:t0 + max(nt, 0)]
        analysis = torch.as_tensor(np.ascontiguousarray(rows[:, 6]), dtype=torch.int32).to(self.sp.device)
        return dict(bias=buf[..., 0], mse=buf[..., 1], variance=buf[..., 2], crps=buf[..., 3], rmse=torch.sqrt(buf[..., 1]),
                    spread=torch.sqrt(buf[..., 2]), analysis=analysis)

    def verif_hist(self, t0=0, nt=None):
        """The rank histograms of the same events: an int32 tensor [nt][2][E][r + 2] on the model's device -- per entry the number
        of points with a non-zero weight whose truth lies above exactly k members, k = 0 ... r, without equalling any, then the
        number of points where it equals one (ties); -1 in a phase that was not filled."""
        info = self.verif_info()
        t0, nt = _held_span(info, t0, nt)
        buf = torch.empty((max(nt, 0), 2, info["entries"], 66), dtype=torch.int32, device=self.sp.device)
        with torch.cuda.device(self.sp.device):
            check(self._lib.spd_model_verif_hist(self._m, t0, nt, C.c_void_p(buf.data_ptr()), buf.numel() * 4, self._stream()),
                  "spd_model_verif_hist")
        return buf[..., :info["members"] + 2]

    # ---- the quantile tape: the distribution over the members at every grid point (spd_model_qtape_*, include/pyspeedy_amd.h) --
    QTAPE_OPS = {"min": _lib.SPD_Q_MIN, "max": _lib.SPD_Q_MAX, "quantile": _lib.SPD_Q_QUANTILE, "prob_above": _lib.SPD_Q_PROB_ABOVE,
                 "prob_below": _lib.SPD_Q_PROB_BELOW}

    def qtape_configure(self, entries, members, every, capacity=64, in_loop=True):
        """Record order statistics over the members with mask 1 in `members` (2 ... 64 of them) at every grid point, after every
        step that leaves current_step at a multiple of `every`, inside run() / run_checked() calls of any length (`in_loop`) or
        only when qtape_apply() is called.  `entries` is a list (at most 64) of (name, level, op) or (name, level, op, param): name
        any of STATS_VARIABLES (the pressure-level ones after plev_configure with its levels in hPa; precnv and precls included),
        level a 0-based level of that name, op "min", "max", "quantile" (param: q within 0 ... 1), "prob_above" or "prob_below"
        (param: a threshold in the unit tape() returns the name in -- t_grid in K, ps_grid and mslp in Pa; the share of the
        members strictly above / below it).  Each value is formed from what a float64 tape holds, exactly as numpy's stable sort
        and the documented interpolation give it, and goes to a ring of `capacity` events in device memory.
        Writes nothing into the model.  Synchronises the device."""
        rows = []
        for entry in entries:
            if len(entry) not in (3, 4):
                raise ValueError("an entry is (name, level, op) or (name, level, op, param), got %r" % (entry,))
            if entry[2] not in self.QTAPE_OPS:
                raise ValueError("op must be one of 'min', 'max', 'quantile', 'prob_above', 'prob_below', got %r" % (entry[2],))
            if entry[2] not in ("min", "max") and len(entry) != 4:
                raise ValueError("op %r needs a parameter: (name, level, op, param)" % (entry[2],))
            rows.append((str(entry[0]), int(entry[1]), entry[2], float(entry[3]) if len(entry) == 4 else 0.0))
        mask = self._member_mask(members)
        names, levels = _c_names(r[0] for r in rows), _c_array(C.c_int, (r[1] for r in rows))
        ops, params = _c_array(C.c_int, (self.QTAPE_OPS[r[2]] for r in rows)), _c_array(C.c_double, (r[3] for r in rows))
        with torch.cuda.device(self.sp.device):
            rc = self._lib.spd_model_qtape_configure(self._m, names, levels, ops, params, len(rows), mask.ctypes.data_as(C.POINTER(C.c_int32)),
                                                     int(every), int(capacity), int(bool(in_loop)))
        if rc != 0:
            self._configure_refused("spd_model_qtape_configure", rc, lambda: self.qtape_info()["members"] == 0, "_qtape_entries")
        self._qtape_entries = tuple(rows)

    def qtape_off(self):
        """Switch the quantile tape off and free everything it holds."""
        with torch.cuda.device(self.sp.device):
            check(self._lib.spd_model_qtape_off(self._m), "spd_model_qtape_off")
        self._qtape_entries = ()

    def qtape_reset(self):
        """Empty the ring of quantile-tape events (no device work)."""
        check(self._lib.spd_model_qtape_reset(self._m), "spd_model_qtape_reset")

    def qtape_apply(self):
        """One event on the state as it stands: a ring slot with every entry's plane; asynchronous on the current stream.
        run(k); qtape_apply() is what the in-loop mode does at a scheduled step."""
        check(self._lib.spd_model_qtape_apply(self._m, self._stream()), "spd_model_qtape_apply")

    def qtape_compute(self):
        """Every entry's plane of the state as it stands, without touching the ring: a float64 tensor [E][48][96] on the model's
        device."""
        out = torch.empty((self.qtape_info()["entries"], 48, 96), dtype=torch.float64, device=self.sp.device)
        with torch.cuda.device(self.sp.device):
            check(self._lib.spd_model_qtape_compute(self._m, C.c_void_p(out.data_ptr()), out.numel() * 8, self._stream()),
                  "spd_model_qtape_compute")
        return out

    def qtape_info(self):
        """dict(members, entries, every, capacity, taken, held, in_loop, applied): masked members r (0: off), the configuration,
        events recorded since qtape_configure / qtape_reset and events the ring holds, the mode, and the events recorded since
        qtape_configure."""
        r, entries, every, capacity, in_loop = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
        taken, applied = C.c_longlong(0), C.c_longlong(0)
        check(self._lib.spd_model_qtape_info(self._m, C.byref(r), C.byref(entries), C.byref(every), C.byref(capacity), C.byref(taken),
                                             C.byref(in_loop), C.byref(applied)), "spd_model_qtape_info")
        return dict(members=r.value, entries=entries.value, every=every.value, capacity=capacity.value, taken=int(taken.value),
                    held=int(min(taken.value, capacity.value)), in_loop=bool(in_loop.value), applied=int(applied.value))

    @property
    def qtape_entries(self):
        """The configured entries, a tuple of (name, level, op, param) in the order qtape() counts them in (empty: off)."""
        return getattr(self, "_qtape_entries", ())

    def _qtape_rows(self):
        return self._ring_rows("spd_model_qtape_rows", self.qtape_info()["held"], 6)

    def qtape_steps(self):
        """The model's step counter at each held event, oldest first (numpy int array)."""
        return self._row_steps(self._qtape_rows())

    def qtape_times(self):
        """The date of each held event's state, oldest first (a list of datetime)."""
        return self._row_times(self._qtape_rows())

    def qtape(self, entry, t0=0, nt=None):
        """The events [t0, t0 + nt) of the held ones, oldest first, of the entry with index `entry` in qtape_entries: a float64
        tensor [nt][48][96] on the model's device."""
        info = self.qtape_info()
        t0, nt = _held_span(info, t0, nt)
        out = torch.empty((max(nt, 0), 48, 96), dtype=torch.float64, device=self.sp.device)
        with torch.cuda.device(self.sp.device):
            check(self._lib.spd_model_qtape_read(self._m, int(entry), t0, nt, C.c_void_p(out.data_ptr()), out.numel() * 8, self._stream()),
                  "spd_model_qtape_read")
        return out

    # ---- spectra by total wavenumber and global means of the spectral state (spd_model_spectra_*, include/pyspeedy_amd.h) -
    SPECTRA_NAMES = ("ke_rot_spectrum", "ke_div_spectrum", "t_spectrum", "q_spectrum", "lnps_spectrum", "t_mean", "q_mean",
                     "lnps_mean")
    # host arithmetic on what was read: name -> the stored names it needs
    SPECTRA_DERIVED = {"ke_spectrum": ("ke_rot_spectrum", "ke_div_spectrum"), "ke_mean": ("ke_rot_spectrum", "ke_div_spectrum"),
                       "ke_column": ("ke_rot_spectrum", "ke_div_spectrum")}
    _SPECTRA_SHAPES = {"ke_rot_spectrum": (8, 32), "ke_div_spectrum": (8, 32), "t_spectrum": (8, 32), "q_spectrum": (8, 32),
                       "lnps_spectrum": (32,), "t_mean": (8,), "q_mean": (8,), "lnps_mean": (1,)}

    def spectra_configure(self, variables, every, capacity):
        """Record `variables` (any of SPECTRA_NAMES, or of SPECTRA_DERIVED: the stored names they need are recorded) after every
        step that leaves current_step at a multiple of `every`, inside run() / run_checked() calls of any length, into a ring in
        device memory that keeps the last `capacity` samples of every member (float64).  Sums over the spectral coefficients: no
        transform, one small launch per sample.  Empties the ring; an empty list switches the spectra off.  Synchronises the device."""
        names = []
        for v in variables:
            for n in self.SPECTRA_DERIVED.get(str(v), (str(v),)):
                if n not in names:
                    names.append(n)
        arr = _c_names(names)
        with torch.cuda.device(self.sp.device):
            check(self._lib.spd_model_spectra_configure(self._m, arr, len(names), int(every), int(capacity)),
                  "spd_model_spectra_configure")

    def spectra_reset(self):
        """Empty the ring of spectra (no device work); the next sample is the first."""
        check(self._lib.spd_model_spectra_reset(self._m), "spd_model_spectra_reset")

    def spectra_info(self):
        """dict(taken, held, capacity, every): samples since the last reset, samples the ring holds (min(taken, capacity)), and
        the configuration."""
        taken, held, capacity, every = C.c_longlong(0), C.c_int(0), C.c_int(0), C.c_int(0)
        check(self._lib.spd_model_spectra_info(self._m, C.byref(taken), C.byref(held), C.byref(capacity), C.byref(every)),
              "spd_model_spectra_info")
        return dict(taken=int(taken.value), held=held.value, capacity=capacity.value, every=every.value)

    def _spectra_rows(self):
        return self._ring_rows("spd_model_spectra_times", self.spectra_info()["held"], 6)

    def spectra_steps(self):
        """The model's step counter after each held sample's step, oldest first (numpy int array)."""
        return self._row_steps(self._spectra_rows())

    def spectra_times(self):
        """The date of each held sample's state, oldest first (a list of datetime)."""
        return self._row_times(self._spectra_rows())

    def _spectra_derive(self, name, rot, div):
        """ke_spectrum = rot + div [..., 8, 32]; ke_mean = its sum over l [..., 8]; ke_column = sum over the levels of dhs[k] *
        ke_mean[k] [...] (the sigma-thickness weights: NOT weighted by the surface pressure)."""
        ke = rot + div
        if name == "ke_spectrum":
            return ke
        mean = ke.sum(dim=-1)
        if name == "ke_mean":
            return mean
        dhs = torch.as_tensor(self.sp.table("dhs"), dtype=torch.float64, device=ke.device)
        return (mean * dhs).sum(dim=-1)

    def spectra(self, name, first=0, count=None, t0=0, nt=None):
        """Members [first, first + count) and samples [t0, t0 + nt) of the held ones (oldest first) of one name: a float64 tensor
        [count][nt][8][32] (ke_rot_spectrum, ke_div_spectrum, t_spectrum, q_spectrum, ke_spectrum), [count][nt][32]
        (lnps_spectrum), [count][nt][8] (t_mean, q_mean, ke_mean), [count][nt][1] (lnps_mean) or [count][nt] (ke_column) on the
        model's device.  Bin l of a spectrum is total wavenumber l."""
        name = str(name)
        if name in self.SPECTRA_DERIVED:
            return self._spectra_derive(name, *(self.spectra(n, first, count, t0, nt) for n in self.SPECTRA_DERIVED[name]))
        first, count = self._range(first, count)
        t0, nt = _held_span(self.spectra_info(), t0, nt)
        shape = self._SPECTRA_SHAPES.get(name, (1,))  # (an unknown name: the library says which ones it knows)
        out = torch.empty((count, max(nt, 0)) + shape, dtype=torch.float64, device=self.sp.device)
        with torch.cuda.device(self.sp.device):
            check(self._lib.spd_model_spectra_read(self._m, name.encode(), first, count, t0, nt, C.c_void_p(out.data_ptr()),
                                                   out.numel() * 8, self._stream()), "spd_model_spectra_read(%s)" % name)
        return out

    def spectrum(self, names=None, first=0, count=None):
        """The same quantities of the state as it stands, without a ring: dict name -> float64 tensor [count][...] on the model's
        device for `names` (default: all of SPECTRA_NAMES; the SPECTRA_DERIVED names are accepted).  One launch."""
        asked = [str(n) for n in (self.SPECTRA_NAMES if names is None else names)]
        stored = []
        for a in asked:
            for n in self.SPECTRA_DERIVED.get(a, (a,)):
                if n not in stored:
                    stored.append(n)
        first, count = self._range(first, count)
        sizes = [count * int(np.prod(self._SPECTRA_SHAPES.get(n, (1,)))) for n in stored]
        buf = torch.empty(sum(sizes), dtype=torch.float64, device=self.sp.device)
        arr = _c_names(stored)
        with torch.cuda.device(self.sp.device):
            check(self._lib.spd_model_spectra_compute(self._m, arr, len(stored), first, count, C.c_void_p(buf.data_ptr()),
                                                      buf.numel() * 8, self._stream()), "spd_model_spectra_compute")
        got, at = {}, 0
        for n, size in zip(stored, sizes):
            got[n] = buf[at:at + size].view((count,) + self._SPECTRA_SHAPES[n])
            at += size
        return {a: self._spectra_derive(a, *(got[n] for n in self.SPECTRA_DERIVED[a])) if a in self.SPECTRA_DERIVED else got[a]
                for a in asked}

    # ---- pressure-level fields and mean sea-level pressure (spd_model_plev_*, include/pyspeedy_amd.h) -------------------
    PLEV_VARIABLES = ("u_plev", "v_plev", "t_plev", "q_plev", "z_plev", "mslp")

    def plev_configure(self, levels_hpa):
        """Set the target pressure levels, in hPa (the C ABI speaks Pa): at most 32, positive, strictly increasing or strictly
        decreasing; results keep this order.  An empty list clears them.  Refused while statistics of a pressure-level variable
        are configured."""
        pa = [float(p) * 100.0 for p in levels_hpa]
        arr = _c_array(C.c_double, pa)
        check(self._lib.spd_model_plev_configure(self._m, arr, len(pa)), "spd_model_plev_configure")

    @property
    def plev_levels(self):
        """The configured target levels in hPa (a tuple, the caller's order)."""
        buf = (C.c_double * 32)()
        n = self._lib.spd_model_plev_levels(self._m, buf, 32)
        if n < 0:
            check(n, "spd_model_plev_levels")
        return tuple(buf[j] / 100.0 for j in range(n))

    def plev(self, names=None, first=0, count=None, refresh=True):
        """Pressure-level fields of members [first, first + count) at the configured levels: a dict of float64 tensors on the
        model's device, [count][n][48][96] (u_plev, v_plev: m/s, t_plev: K, q_plev: kg/kg, z_plev: m) and [count][48][96] (mslp:
        Pa); `names`: any of PLEV_VARIABLES, None = all.  Linear in ln p between the model's full levels, isothermal above the
        top one, constant lapse rate (6 K/km) below the lowest.  Points under the ground (p > ps) are extrapolated like any other
        point below the lowest level, not masked: compare with ps_grid to find them.  With `refresh` the grid arrays are first
        brought up to date (spectral2grid() of those members); without, they are used as they are."""
        names = list(self.PLEV_VARIABLES) if names is None else [str(v) for v in names]
        first, count = self._range(first, count)
        arr = _c_names(names)
        out = {}
        with torch.cuda.device(self.sp.device):
            check(self._lib.spd_model_plev_compute(self._m, arr, len(names), first, count, int(bool(refresh)), self._stream()),
                  "spd_model_plev_compute")
            for name in names:
                t = torch.empty((count,) + self._stats_shape(name), dtype=torch.float64, device=self.sp.device)
                check(self._lib.spd_model_plev_read(self._m, name.encode(), first, count, C.c_void_p(t.data_ptr()), t.numel() * 8,
                                                    self._stream()), "spd_model_plev_read(%s)" % name)
                out[name] = t
        return out

    # ---- derived fields (spd_model_derive_*, include/pyspeedy_amd.h) ------------------------------------------------------
    # Every recorder that takes STATS_VARIABLES takes these names as well (the window tape: next to WINTAPE_NAMES).
    DERIVED_VARIABLES = ("vor_grid", "div_grid", "omega_grid", "rh_grid", "theta_grid", "tcwv", "ivt_u", "ivt_v", "ke_col",
                         "omega_plev", "vor_plev", "div_plev", "rh_plev", "theta_plev")  # (the last five: after plev_configure)

    def derived(self, names=None, first=0, count=None, refresh=True):
        """Derived fields of members [first, first + count): a dict of float64 tensors on the model's device.  [count][8][48][96]:
        vor_grid, div_grid (1/s), omega_grid (Pa/s, the model's own continuity equation), rh_grid (a fraction, not clipped),
        theta_grid (K); [count][48][96]: tcwv (kg/m^2), ivt_u, ivt_v (kg/(m s)), ke_col (J/m^2); [count][n][48][96] at the levels
        of plev_configure: omega_plev, vor_plev, div_plev, rh_plev, theta_plev (linear in ln p between the full levels, the
        nearest full level's value outside them; points under the ground are not masked).  `names`: any of DERIVED_VARIABLES,
        None = all that can be computed (the pressure-level ones only with levels configured).  With `refresh` the grid arrays
        are first brought up to date (spectral2grid() of those members); without, they are used as they are."""
        if names is None:
            names = [v for v in self.DERIVED_VARIABLES if not v.endswith("_plev") or self.plev_levels]
        names = [str(v) for v in names]
        first, count = self._range(first, count)
        arr = _c_names(names)
        out = {}
        with torch.cuda.device(self.sp.device):
            check(self._lib.spd_model_derive_compute(self._m, arr, len(names), first, count, int(bool(refresh)), self._stream()),
                  "spd_model_derive_compute")
            for name in names:
                t = torch.empty((count,) + self._stats_shape(name), dtype=torch.float64, device=self.sp.device)
                check(self._lib.spd_model_derive_read(self._m, name.encode(), first, count, C.c_void_p(t.data_ptr()), t.numel() * 8,
                                                      self._stream()), "spd_model_derive_read(%s)" % name)
                out[name] = t
        return out

    def set_flags(self, land_coupling_flag=True, sst_anomaly_coupling_flag=True, increase_co2=False):
        check(self._lib.spd_model_set_flags(self._m, int(land_coupling_flag), int(sst_anomaly_coupling_flag),
                                            int(increase_co2)), "spd_model_set_flags")

    # ---- time stepping -------------------------------------------------------------------------------------
    def set_time_step(self, dt):
        check(self._lib.spd_model_set_time_step(self._m, float(dt)), "spd_model_set_time_step")

    def step_dynamics(self, j1, j2, dt, compute_shortwave):
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        check(self._lib.spd_model_step_dynamics(self._m, int(j1), int(j2), float(dt), int(bool(compute_shortwave)), stream),
              "spd_model_step_dynamics")

    def check_begin(self, time_level=2):
        """Enqueue the range check of the current state; returns a token for check_end (at most two may be in flight)."""
        slot = self._lib.spd_model_check_begin(self._m, int(time_level), self._stream())
        if slot < 0:
            check(slot, "spd_model_check_begin")
        return slot

    def check_defer(self, time_level=2):
        """check_begin without a launch of its own: the check rides in the next single-step run() on this stream, or goes out when
        anything else would touch the state first (spd_model_check_defer).  Returns the token for check_end."""
        slot = self._lib.spd_model_check_defer(self._m, int(time_level), self._stream())
        if slot < 0:
            check(slot, "spd_model_check_defer")
        return slot

    def check_counts(self):
        """(range checks launched on their own, range checks carried by a step's launch)"""
        alone, rode = C.c_int32(0), C.c_int32(0)
        check(self._lib.spd_model_check_counts(self._m, C.byref(alone), C.byref(rode)), "spd_model_check_counts")
        return alone.value, rode.value

    def check_end(self, token):
        codes = np.zeros(self.nmembers, dtype=np.int32)
        check(self._lib.spd_model_check_end(self._m, int(token), codes.ctypes.data_as(C.c_void_p)), "spd_model_check_end")
        return codes

    def check(self, time_level=2, with_diag=False):
        """diagnostics.f90 range check; returns int32 codes per member (0 ok, -2 out of range) [and the diagnostics]."""
        codes = np.zeros(self.nmembers, dtype=np.int32)
        diag = np.zeros((self.nmembers, 3, 8)) if with_diag else None
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        check(self._lib.spd_model_check(self._m, int(time_level), codes.ctypes.data_as(C.c_void_p),
                                        diag.ctypes.data_as(C.c_void_p) if with_diag else None, stream), "spd_model_check")
        return (codes, diag) if with_diag else codes
