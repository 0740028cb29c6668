"""States at the edges of the range check (diagnostics.f90:16-76) for tests/golden/range_check.npz.  TEST INFRASTRUCTURE.

The base state is d1_vor / d1_div / d1_t of tests/golden/run.npz (the reference after one day, both time levels).  A case is that
state with a few edits, each one a row (slot, kind, level, value) of the case table (0-based slot and level):

  VOR    the eddy coefficients (m >= 1) of vorticity on that level times `value`
  DIV    the same for divergence
  TMEAN  Re t(m=0, n=0) on that level := `value`
  ZONAL  the zonal-mean coefficients (m = 0) of vorticity and divergence on that level times `value`

Per level k the eddy kinetic energies are brought to 500 (1 -+ DELTA) -- value = sqrt(500 (1 -+ DELTA) / D_k), D_k the oracle's
diag(k, 1) / diag(k, 2) of the base state's first time level -- and the global-mean temperature to 180 and 320 K exactly and to
the next double outside.  The edits are plain numpy arithmetic: oracle/gen_golden_range.py (the reference's codes) and the
tests build the same bits from the stored table.
"""
import numpy as np

KX = 8
DELTA = 1e-9
VOR, DIV, TMEAN, ZONAL = 0, 1, 2, 3
SQRT_HALF = float(np.sqrt(np.float32(0.5)))  # diagnostics.f90:40: sqrt(0.5) of a default (single precision) real
T_HI = 452.5483477044255    # SQRT_HALF * T_HI == 320.0: accepted (the test is `> 320`)
T_LO = 254.55844558373934   # SQRT_HALF * T_LO == 180.0: accepted (`< 180`)


def t_edges():
    """[accepted at 320, the next double up, accepted at 180, the next double down]"""
    return np.array([T_HI, np.nextafter(T_HI, np.inf), T_LO, np.nextafter(T_LO, -np.inf)])


def base(run):
    """(vor, div, t) of a mapping with run.npz's arrays: complex (31, 32, 8, 2), Fortran order."""
    return tuple(np.asfortranarray(run["d1_" + n]) for n in ("vor", "div", "t"))


def scales(ke_base):
    """ke_base [KX, 2]: eddy KE (vorticity, divergence) per level -> [2, KX, 2] value of the VOR / DIV edits: (1 - DELTA, 1 + DELTA)"""
    target = 500.0 * np.array([1.0 - DELTA, 1.0 + DELTA])
    return np.sqrt(target[None, None, :] / ke_base.T[:, :, None])


def table(ke_base):
    """-> (names, rows): the cases in order and their edits, rows [n, 5] float64 = (case, slot, kind, level, value)."""
    s, te = scales(ke_base), t_edges()
    names, rows = [], []

    def case(name, *edits):
        for slot, kind, level, value in edits:
            rows.append((len(names), slot, kind, level, value))
        names.append(name)

    for k in range(KX):
        for kind, tag in ((VOR, "vor"), (DIV, "div")):
            case("%s_ke_below_l%d" % (tag, k), (0, kind, k, s[kind, k, 0]))
            case("%s_ke_above_l%d" % (tag, k), (0, kind, k, s[kind, k, 1]))
        for j, tag in enumerate(("t_320_l%d", "t_above_320_l%d", "t_180_l%d", "t_below_180_l%d")):
            case(tag % k, (0, TMEAN, k, te[j]))
    case("base")
    case("zonal_mean_x30", *[(0, ZONAL, k, 30.0) for k in range(KX)])  # far above 500, but the zonal mean does not count
    case("two_levels_inside", (0, VOR, 2, s[VOR, 2, 0]), (0, TMEAN, 5, te[2]))
    case("two_levels_outside", (0, DIV, 6, s[DIV, 6, 1]), (0, TMEAN, 1, te[1]))
    # outside through all three conditions, but in the time level the check does not look at
    case("other_time_level", (1, TMEAN, 3, te[1]), (1, VOR, 0, s[VOR, 0, 1] * 2.0), (1, DIV, 5, s[DIV, 5, 1] * 2.0))
    return np.array(names), np.array(rows, dtype=np.float64).reshape(-1, 5)


def build(state, rows, index):
    """Case `index` of the table on the base state (vor, div, t): new arrays, the base is not touched."""
    vor, div, t = (a.copy(order="F") for a in state)
    for _, slot, kind, level, value in rows[rows[:, 0] == index]:
        slot, kind, level = int(slot), int(kind), int(level)
        if kind == VOR:
            vor[1:, :, level, slot] *= value
        elif kind == DIV:
            div[1:, :, level, slot] *= value
        elif kind == TMEAN:
            t[0, 0, level, slot] = complex(value, t[0, 0, level, slot].imag)
        elif kind == ZONAL:
            vor[0, :, level, slot] *= value
            div[0, :, level, slot] *= value
        else:
            raise ValueError(kind)
    return vor, div, t


def swap(state):
    """The two time levels exchanged: a case built for time level 1 is what a check of time level 2 then sees."""
    return tuple(np.asfortranarray(a[..., ::-1]) for a in state)


def oracle_check(orc, state, time_level):
    """check_diagnostics of the CPU oracle (module `orc`) on (vor, div, t) -> (code, diag [KX, 3])"""
    vor, div, t = state
    arrays = {"vor": vor, "div": div, "t": t}
    arrays.update({n: np.zeros((96, 48)) for n in orc.PHYS_IN_2D[1:]})  # (read by the step only)
    return orc.check_diagnostics(orc.ModelState(arrays, False, 0.0), time_level)
