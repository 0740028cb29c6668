"""The track tape's rule for one plane (csrc/track_point.hpp) restated in numpy, step for step:

    1. candidates: the points of the region whose value is not NaN; with radius > 0 and prev = q >= 0 only those with
       |j - j_q| <= radius and a circular distance of i and i_q <= radius
    2. winner: the smallest (op 0) or largest (op 1) candidate, among equal values the smallest p = 96 j + i; none: NaN, -1, 0, 0
    3. a = x[j][(i + 95) % 96], b = x[p], c = x[j][(i + 1) % 96];  den = (a - 2 b) + c;  num = 0.5 (a - c);  di = num / den where
       den is finite and not zero and the quotient is finite, else 0; clamped to [-0.5, 0.5]; dj from rows j - 1, j + 1, 0 on rows
       0 and 47

The minimum and the maximum are exact (comparisons only); every arithmetic operation of step 3 is one IEEE fp64 operation on numpy
scalars.  `track_loop` is the same rule as a loop over Python floats in ascending p, which tests/test_tracktape_cpu.py holds
`track` to.  `follow` carries the follow-state over the samples of a series as the recorder does."""
import math

import numpy as np

IX, IL = 96, 48
POINTS = IX * IL
MIN, MAX = 0, 1
NAN = float("nan")


def window(prev, radius):
    """[4608] bool: the points within `radius` rows and columns (circular) of the point prev"""
    p = np.arange(POINTS)
    dj = np.abs(p // IX - prev // IX)
    di = np.abs(p % IX - prev % IX)
    di = np.minimum(di, IX - di)
    return (dj <= radius) & (di <= radius)


def offset(a, b, c):
    a, b, c = np.float64(a), np.float64(b), np.float64(c)
    with np.errstate(all="ignore"):
        den = (a - np.float64(2.0) * b) + c
        num = np.float64(0.5) * (a - c)
        if not np.isfinite(den) or den == 0.0:
            return np.float64(0.0)
        q = num / den
    if not np.isfinite(q):
        return np.float64(0.0)
    return np.float64(-0.5) if q < -0.5 else np.float64(0.5) if q > 0.5 else q


def track(x, mask, prev=-1, radius=0, op=MIN):
    """x: one plane [48][96] or [4608]; mask: the region, non-zero inside -> (value, p, di, dj) as four np.float64"""
    x = np.asarray(x, dtype=np.float64).reshape(POINTS)
    cand = (np.asarray(mask).reshape(POINTS) != 0) & ~np.isnan(x)
    if radius > 0 and prev >= 0:
        cand &= window(prev, radius)
    if not cand.any():
        return np.float64(NAN), np.float64(-1.0), np.float64(0.0), np.float64(0.0)
    best = x[cand].max() if op == MAX else x[cand].min()
    p = int(np.flatnonzero(cand & (x == best))[0])  # (== : the two zeros are equal values)
    j, i = divmod(p, IX)
    grid = x.reshape(IL, IX)
    di = offset(grid[j, (i + IX - 1) % IX], grid[j, i], grid[j, (i + 1) % IX])
    dj = np.float64(0.0) if j in (0, IL - 1) else offset(grid[j - 1, i], grid[j, i], grid[j + 1, i])
    return grid[j, i], np.float64(p), di, dj


def offset_loop(a, b, c):
    den = (a - 2.0 * b) + c
    num = 0.5 * (a - c)
    if math.isnan(den) or math.isinf(den) or den == 0.0:
        return 0.0
    q = num / den
    if math.isnan(q) or math.isinf(q):
        return 0.0
    return -0.5 if q < -0.5 else 0.5 if q > 0.5 else q


def track_loop(x, mask, prev=-1, radius=0, op=MIN):
    """one plane, with Python floats, in ascending p -> four Python floats"""
    x = [float(v) for v in np.asarray(x, dtype=np.float64).reshape(POINTS)]
    inside = [bool(v) for v in np.asarray(mask).reshape(POINTS) != 0]
    best, at = 0.0, -1
    for p in range(POINTS):
        v = x[p]
        if not inside[p] or v != v:
            continue
        if radius > 0 and prev >= 0:
            dj = abs(p // IX - prev // IX)
            di = abs(p % IX - prev % IX)
            if dj > radius or min(di, IX - di) > radius:
                continue
        if at < 0 or (v > best if op == MAX else v < best):  # (ascending p: a tie keeps the lower index)
            best, at = v, p
    if at < 0:
        return NAN, -1.0, 0.0, 0.0
    j, i = divmod(at, IX)
    di = offset_loop(x[IX * j + (i + IX - 1) % IX], best, x[IX * j + (i + 1) % IX])
    dj = 0.0 if j in (0, IL - 1) else offset_loop(x[at - IX], best, x[at + IX])
    return best, float(at), di, dj


def follow(planes, mask, radius, op, prev=-1):
    """planes: the samples of one member and plane, [T][48][96] -> ([T][4] float64, the follow-state after the last sample)"""
    out = np.empty((len(planes), 4), dtype=np.float64)
    for s, x in enumerate(planes):
        out[s] = track(x, mask, prev, radius, op)
        prev = int(out[s, 1])
    return out, prev


def bits(values):
    """the bit patterns of four (or any number of) doubles, for bitwise comparisons that tell -0.0 from 0.0 and compare NaN"""
    return np.asarray(values, dtype=np.float64).view(np.uint64).tolist()
