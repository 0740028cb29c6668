"""Generate the boundary-set goldens from the flang-compiled REFERENCE: the three sets of tests/boundary_cases.py (mirrored, icy,
patchy) at both of its start dates, unperturbed, zero SST anomaly, 12 steps each.  TEST INFRASTRUCTURE.

  tests/golden/bounds_<set>_<mmdd>_spec.npz   vor, div, t, tr, ps at time level 1 (as run10.npz stores them)
  tests/golden/bounds_<set>_<mmdd>_surf.npz   the surface and flux fields of boundary_cases.SURFACE (hfluxn: the two planes the
                                              reference writes), cal_ymdhm [5] and cal_month_idx

The inputs are not stored: boundary_cases.py rebuilds them from the committed example file.  Every file stays under 1 MiB (asserted)
and is written with fixed zip time stamps, so that a second run reproduces the committed files byte for byte.

Needs oracle/_ref/libspeedy_ref.so (oracle/build_ref.sh); a few seconds:  python oracle/gen_golden_boundaries.py
"""
import ctypes as C
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", "tests"))
import refmodel as R  # noqa: E402
import boundary_cases as bcs  # noqa: E402

GOLD = os.path.join(HERE, "..", "tests", "golden")
MAX_FILE_BYTES = 1 << 20
STEPS = 12


def control(m):
    ymdhm = (C.c_int * 5)()
    mi, im = C.c_int(0), C.c_int(0)
    tm, ty = C.c_double(0), C.c_double(0)
    R.lib().shim_control_params(m.ctl, ymdhm, C.byref(mi), C.byref(im), C.byref(tm), C.byref(ty))
    return list(ymdhm), mi.value


def save(dst, arrays):
    """np.savez_compressed with the members' time stamps fixed (numpy stamps them with the time of writing)."""
    with zipfile.ZipFile(dst, "w", zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays.items():
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with z.open(info, "w", force_zip64=True) as f:
                np.lib.format.write_array(f, np.asarray(a), allow_pickle=False)
    size = os.path.getsize(dst)
    assert size < MAX_FILE_BYTES, (dst, size)
    print("wrote %s: %d arrays, %.2f MB" % (os.path.basename(dst), len(arrays), size / 1e6), flush=True)


def main():
    bc = np.load(os.path.join(HERE, "..", "pyspeedy_amd", "data", "example_bc.npz"))
    for name in bcs.SETS:
        for start in bcs.START_DATES:
            y, mo = start[0], start[1]
            m = R.RefModel(start=start, end=(y, mo + 1, 2, 0, 0))  # (two months: the run from 30 June ends in July)
            m.set_bc(bcs.fields(bc, name))
            for k in range(STEPS):
                assert m.step() == 0, "%s %s: the reference left the accepted range at step %d" % (name, bcs.tag(start), k)
            spec = {}
            for n in bcs.SPEC:
                a = m.get(n)
                spec[n] = (a[..., 0] if n == "tr" else a)[..., 0]  # (tr: a trailing tracer axis of length 1), time level 1
            surf = {n: (m.get(n)[:, :, :2] if n == "hfluxn" else m.get(n)) for n in bcs.SURFACE}
            assert all(np.isfinite(a).all() for a in list(spec.values()) + list(surf.values())), (name, start)
            ymdhm, month_idx = control(m)
            surf["cal_ymdhm"], surf["cal_month_idx"] = np.array(ymdhm, dtype=np.int32), np.int32(month_idx)
            save(bcs.golden_path(GOLD, name, start, "spec"), spec)
            save(bcs.golden_path(GOLD, name, start, "surf"), surf)


if __name__ == "__main__":
    main()
