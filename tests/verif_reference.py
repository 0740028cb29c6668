"""The verification tape's scores (csrc/verif_point.hpp) restated in numpy, operation for operation.

At a point the truth is y and the ensemble x_1 ... x_r in ascending member index:

    s = x_1;  s = s + x_j (j = 2 ... r);  mean = s / r;  e = mean - y;  se = e e
    a = (x_1 - mean)^2;  a = a + (x_j - mean)^2 (j = 2 ... r);  v = a / (r - 1)
    b = |x_1 - y|;  b = b + |x_j - y| (j = 2 ... r)
    c = 0;  c = c + |x_j - x_k| for j = 1 ... r - 1 (outer), k = j + 1 ... r (inner)
    crps = b / r - c / (r r);  rank = #{j : x_j < y};  tie = 1 if some x_j == y

The loops over the members are Python loops; each line inside them is one elementwise IEEE fp64 operation of numpy over the
points.  No np.sum and no np.mean takes part.  An entry is the four sums of w e, w se, w v, w crps in the projection tape's
order (tests/projtape_reference.py) and r + 2 counts over the points with w != 0.  `point_loop` is one point with Python floats."""
import numpy as np

import projtape_reference as proj

COUNTS = 66  # int32 per entry in a ring slot: hist[0 ... r], ties at r + 1, zero behind
NAMES = ("bias", "mse", "variance", "crps")


def points(x, y):
    """x: the ensemble [r][...], y: the truth [...] -> dict(mean, e, se, v, crps: float64 [...]; rank: int [...]; tie: bool [...])"""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    r = x.shape[0]
    assert r >= 2
    s = x[0].copy()
    for j in range(1, r):
        s = s + x[j]
    mean = s / float(r)
    e = mean - y
    se = e * e
    d = x[0] - mean
    a = d * d
    for j in range(1, r):
        d = x[j] - mean
        a = a + d * d
    v = a / float(r - 1)
    b = np.abs(x[0] - y)
    for j in range(1, r):
        b = b + np.abs(x[j] - y)
    c = np.zeros_like(y)
    for j in range(r - 1):
        for k in range(j + 1, r):
            c = c + np.abs(x[j] - x[k])
    crps = b / float(r) - c / (float(r) * float(r))
    rank = np.zeros(y.shape, dtype=np.int64)
    tie = np.zeros(y.shape, dtype=bool)
    for j in range(r):
        rank = rank + (x[j] < y)
        tie = tie | (x[j] == y)
    return dict(mean=mean, e=e, se=se, v=v, crps=crps, rank=rank, tie=tie)


def point_loop(x, y):
    """one point with Python floats: x a sequence of r values, y a value -> (e, se, v, crps, rank, tie)"""
    x = [float(v) for v in x]
    y = float(y)
    r = len(x)
    s = x[0]
    for j in range(1, r):
        s = s + x[j]
    mean = s / float(r)
    e = mean - y
    se = e * e
    a = (x[0] - mean) * (x[0] - mean)
    for j in range(1, r):
        a = a + (x[j] - mean) * (x[j] - mean)
    v = a / float(r - 1)
    b = abs(x[0] - y)
    for j in range(1, r):
        b = b + abs(x[j] - y)
    c = 0.0
    for j in range(r - 1):
        for k in range(j + 1, r):
            c = c + abs(x[j] - x[k])
    crps = b / float(r) - c / (float(r) * float(r))
    return e, se, v, crps, len([1 for xj in x if xj < y]), any(xj == y for xj in x)


def entry(scored, w):
    """scored: points() of one plane ([4608] or [48][96]); w: one weight map -> (float64 [4], int32 [COUNTS])"""
    w = np.asarray(w, dtype=np.float64).reshape(proj.POINTS)
    out = np.array([proj.project(w, scored[k].reshape(proj.POINTS)) for k in ("e", "se", "v", "crps")], dtype=np.float64)
    rank, tie = scored["rank"].reshape(proj.POINTS), scored["tie"].reshape(proj.POINTS)
    r = int(rank.max(initial=0))
    hist = np.zeros(COUNTS, dtype=np.int32)
    for k in range(r + 1):
        hist[k] = np.count_nonzero((w != 0.0) & ~tie & (rank == k))
    return out, hist, int(np.count_nonzero((w != 0.0) & tie))


def score(x, y, w):
    """One entry: x [r][4608] (or [r][48][96]), y, w one plane each -> (float64 [4] = bias, mse, variance, crps, int32 [COUNTS])"""
    x = np.asarray(x, dtype=np.float64)
    r = x.shape[0]
    out, hist, ties = entry(points(x, y), w)
    hist[r + 1] = ties
    return out, hist


def event(planes, truth, members, entries, weights):
    """The rows of one event.  planes: {(name, level): array [M][48][96]} as an fp64 tape holds them; members: the masked member
    indices in ascending order; entries: (name, level, pattern) -> (float64 [E][4], int32 [E][COUNTS])"""
    scored = {}
    scores, hists = [], []
    for name, level, pattern in entries:
        key = (name, level)
        if key not in scored:  # (once per distinct plane)
            scored[key] = points(planes[key][list(members)], planes[key][truth])
        out, hist, ties = entry(scored[key], weights[pattern])
        hist[len(members) + 1] = ties
        scores.append(out)
        hists.append(hist)
    return np.stack(scores), np.stack(hists)
