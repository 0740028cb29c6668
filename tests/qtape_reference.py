"""The quantile tape's values (include/pyspeedy_amd.h) restated in numpy.

At a point the members' values are x_0 ... x_(r-1) in ascending member index and s = np.sort(x, axis=0, kind="stable") their
stable ascending order (x_j before x_k iff x_j < x_k, or neither is less and j < k):

    min = s[0];  max = s[r - 1]
    quantile q:  h = fl(q (r - 1));  lo = floor(h);  f = h - lo;  hi = min(lo + 1, r - 1)
                 f == 0: s[lo].  Otherwise d = s[hi] - s[lo];  t = f d;  v = s[lo] + t;  v = s[hi] where v > s[hi]
    prob_above thr = #{j : x_j > thr} / r;  prob_below thr = #{j : x_j < thr} / r

The order comes from numpy's sort; each further line is one elementwise IEEE fp64 operation of numpy over the points.  Nothing
here is shared with the library."""
import numpy as np

OPS = {"min": 0, "max": 1, "quantile": 2, "prob_above": 3, "prob_below": 4}


def order(x):
    """x [r][...] -> the stable ascending order over the members"""
    return np.sort(np.asarray(x, dtype=np.float64), axis=0, kind="stable")


def descriptor(q, r):
    """-> (lo, hi, f) of the quantile q for r members"""
    h = np.float64(q) * np.float64(r - 1)
    lo = int(np.floor(h))
    f = h - np.float64(lo)
    return lo, min(lo + 1, r - 1), f


def quantile(s, q):
    """s: order(x) -> the quantile q at every point"""
    r = s.shape[0]
    lo, hi, f = descriptor(q, r)
    if f == 0.0:
        return s[lo].copy()
    d = s[hi] - s[lo]
    t = f * d
    v = s[lo] + t
    return np.where(v > s[hi], s[hi], v)


def value(x, op, param=0.0, s=None):
    """one entry: x [r][...] in ascending member index (s: order(x), if the caller has it) -> float64 [...]"""
    x = np.asarray(x, dtype=np.float64)
    r = x.shape[0]
    assert r >= 2
    if op == "prob_above":
        return (x > param).sum(axis=0) / float(r)
    if op == "prob_below":
        return (x < param).sum(axis=0) / float(r)
    s = order(x) if s is None else s
    if op == "min":
        return s[0].copy()
    if op == "max":
        return s[r - 1].copy()
    assert op == "quantile"
    return quantile(s, param)


def event(planes, members, entries):
    """The planes of one event.  planes: {(name, level): array [M][48][96]} as an fp64 tape holds them; members: the masked member
    indices in ascending order; entries: (name, level, op[, param]) -> float64 [E][48][96]"""
    ordered, out = {}, []
    for entry in entries:
        key = (entry[0], entry[1])
        x = planes[key][list(members)]
        if key not in ordered:  # (once per distinct plane)
            ordered[key] = order(x)
        out.append(value(x, entry[2], entry[3] if len(entry) > 3 else 0.0, s=ordered[key]))
    return np.stack(out)
