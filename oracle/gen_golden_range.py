"""Generate tests/golden/range_check.npz: the codes of the REFERENCE's range check (the driver's `check`, speedy_driver.f90:81-91:
check_diagnostics of time level 1, diagnostics.f90:16-76) for the edge cases of oracle/range_cases.py.  TEST INFRASTRUCTURE;
needs oracle/_ref/libspeedy_ref.so, and the CPU oracle for the eddy kinetic energies of the base state that size the edits.

    python oracle/gen_golden_range.py

Stored -- no states: the tests rebuild every case from tests/golden/run.npz and the edit table (range_cases.build):
  delta      the DELTA of the kinetic-energy edits
  ke_base    [8, 2]     the oracle's diag(k, 1), diag(k, 2) of the base state's time level 1
  ke_scale   [2, 8, 2]  the factors of the VOR / DIV edits: (vorticity, divergence), level, (just inside, just outside)
  t_edges    [4]        Re t(0, 0) at 320 K, the next double up, at 180 K, the next double down (range_cases.t_edges)
  names      [N]        the cases;  edits [n, 5]: (case, slot, kind, level, value) per edit
  code       [N] int32  the reference's error code of each case (0 or -2)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import oracle as O  # noqa: E402
import range_cases as RC  # noqa: E402
import refmodel as R  # noqa: E402

GOLD = os.path.join(HERE, "..", "tests", "golden")


def expected(name):
    """the code each case is built to give"""
    return -2 if ("above" in name or "below_180" in name or name.endswith("_outside")) else 0


def main():
    state = RC.base(np.load(os.path.join(GOLD, "run.npz")))
    rc, diag = RC.oracle_check(O, state, 1)
    assert rc == 0, rc
    ke = diag[:, :2].copy()
    names, edits = RC.table(ke)
    m = R.RefModel()
    m.set_bc(np.load(os.path.join(HERE, "..", "pyspeedy_amd", "data", "example_bc.npz")))
    codes = []
    for i in range(len(names)):
        vor, div, t = RC.build(state, edits, i)
        m.set("vor", vor)
        m.set("div", div)
        m.set("t", t)
        codes.append(m.check())
    codes = np.array(codes, dtype=np.int32)
    for name, c in zip(names, codes):  # a disagreement is a finding about the reference: it is recorded, and followed
        if c != expected(name):
            print("the reference gives %d for %s" % (c, name))
    out = dict(delta=np.float64(RC.DELTA), ke_base=ke, ke_scale=RC.scales(ke), t_edges=RC.t_edges(), names=names, edits=edits,
               code=codes)
    dst = os.path.join(GOLD, "range_check.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, "%d cases, %d of them out of range" % (len(names), int((codes != 0).sum())))


if __name__ == "__main__":
    main()
