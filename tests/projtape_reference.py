"""The projection tape's sum (csrc/projtape.hpp) restated in numpy, operation for operation:

    lane t of 256:   s_t = w[t] * x[t];  for r = 1 ... 17 in that order  s_t = s_t + w[t + 256 r] * x[t + 256 r]
    tree[t] = s_t;   for half = 128, 64, ..., 1:  tree[t] = tree[t] + tree[t + half]  for t < half;   result = tree[0]

Every product and every sum is one elementwise IEEE fp64 operation of numpy; no np.sum (which adds pairwise in blocks of its own
choosing) takes part.  `project_loop` is the same order as a loop over Python floats, which tests/test_projtape_cpu.py holds
`project` to."""
import numpy as np

LANES, PASSES = 256, 18
POINTS = LANES * PASSES  # 4608 = 48 * 96


def project(w, x):
    """w: one weight map, [48][96] or [4608]; x: planes [..., 48, 96] or [..., 4608] -> the sum of each plane, shape [...]"""
    w = np.asarray(w, dtype=np.float64).reshape(POINTS)
    x = np.asarray(x, dtype=np.float64)
    lead = x.shape[:-2] if x.shape[-1] != POINTS else x.shape[:-1]
    terms = (w * x.reshape(lead + (POINTS,))).reshape(lead + (PASSES, LANES))  # [..., r, t]: the product at point t + 256 r
    tree = terms[..., 0, :].copy()
    for r in range(1, PASSES):  # a sequential add along the passes, per lane
        tree = tree + terms[..., r, :]
    half = LANES // 2
    while half > 0:
        tree = tree[..., :half] + tree[..., half:2 * half]
        half //= 2
    return tree[..., 0]


def project_loop(w, x):
    """one plane, with Python floats"""
    w = [float(v) for v in np.asarray(w, dtype=np.float64).reshape(POINTS)]
    x = [float(v) for v in np.asarray(x, dtype=np.float64).reshape(POINTS)]
    tree = []
    for t in range(LANES):
        s = w[t] * x[t]
        for r in range(1, PASSES):
            s = s + w[t + LANES * r] * x[t + LANES * r]
        tree.append(s)
    half = LANES // 2
    while half > 0:
        for t in range(half):
            tree[t] = tree[t] + tree[t + half]
        half //= 2
    return tree[0]
