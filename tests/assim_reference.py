"""The arbiter of the assimilation tests: numpy and Python floats only, written from the definition (DESIGN section 4l,
include/pyspeedy_amd.h), sharing nothing with csrc/.

weights(Y, yo, R, inflation): the serial ensemble square-root filter's member-mixing matrix.  Y is [E][r] (entry e, member i), yo[E]
the observations (NaN: missing), R[E] their error variances.  Every operation is one IEEE fp64 operation of a Python float, every
sum is a loop in ascending index that starts from its first term:

    a = (1 - rho) / r;  W[i][j] = a for i != j,  W[i][i] = a + rho
    for e = 0 ... E-1:
        y_j = sum_i Y[e][i] W[i][j];  ybar = (sum_j y_j) / r;  d_j = y_j - ybar;  s = (sum_j d_j d_j) / (r - 1)
        unused if yo_e is NaN or s is not a finite number > 0; otherwise
        t = s + R_e;  alpha = 1 / (1 + sqrt(R_e / t));  v = yo_e - ybar;  q = (r - 1) t
        g_i = d_i / q;  c_j = v - alpha d_j;  u_k = sum_i W[k][i] g_i;  W[k][j] = W[k][j] + u_k c_j

-> (W [r][r], stats [E][4] = ybar, s, v, used; v = 0.0 for a missing observation).

transform(states, W): X'_j = (...((W[0][j] X_0) + W[1][j] X_1) + ...) + W[r-1][j] X_(r-1) on real and imaginary parts separately,
for the coefficients with m + n <= 31 of both time levels; one elementwise numpy operation per product and per sum.  A state is a
dict name -> complex (31 m, 32 n[, 8 levels], 2 time levels) over vor, div, t, tr, ps, as EnsembleModel.get returns a member."""
import math

import numpy as np

NAMES = ("vor", "div", "t", "tr", "ps")
INSIDE = np.add.outer(np.arange(31), np.arange(32)) <= 31


def weights(Y, yo, R, inflation=1.0):
    Y = np.asarray(Y, dtype=np.float64)
    E, r = Y.shape
    Y = [[float(v) for v in row] for row in Y]
    yo, R, rho = [float(v) for v in yo], [float(v) for v in R], float(inflation)
    a = (1.0 - rho) / float(r)
    W = [[a + rho if i == j else a for j in range(r)] for i in range(r)]
    stats = []
    for e in range(E):
        y = []
        for j in range(r):
            acc = Y[e][0] * W[0][j]
            for i in range(1, r):
                acc = acc + Y[e][i] * W[i][j]
            y.append(acc)
        total = y[0]
        for j in range(1, r):
            total = total + y[j]
        ybar = total / float(r)
        d = [y[j] - ybar for j in range(r)]
        ss = d[0] * d[0]
        for j in range(1, r):
            ss = ss + d[j] * d[j]
        s = ss / float(r - 1)
        missing = math.isnan(yo[e])
        used = (not missing) and s > 0.0 and s < math.inf
        v = 0.0 if missing else yo[e] - ybar
        stats.append([ybar, s, v, 1.0 if used else 0.0])
        if not used:
            continue
        t = s + R[e]
        alpha = 1.0 / (1.0 + math.sqrt(R[e] / t))
        q = float(r - 1) * t
        g = [d[i] / q for i in range(r)]
        c = [v - alpha * d[j] for j in range(r)]
        u = []
        for k in range(r):
            acc = W[k][0] * g[0]
            for i in range(1, r):
                acc = acc + W[k][i] * g[i]
            u.append(acc)
        for k in range(r):
            for j in range(r):
                W[k][j] = W[k][j] + u[k] * c[j]
    return np.array(W, dtype=np.float64), np.array(stats, dtype=np.float64).reshape(E, 4)


def transform_variable(xs, W):
    """xs: one variable of the r members (a list of equal-shaped complex arrays); -> the list of the r new ones"""
    W = np.asarray(W, dtype=np.float64)
    r = len(xs)
    out = []
    for j in range(r):
        re = W[0, j] * xs[0].real
        im = W[0, j] * xs[0].imag
        for i in range(1, r):
            re = re + W[i, j] * xs[i].real
            im = im + W[i, j] * xs[i].imag
        new = np.empty_like(xs[j])
        new.real, new.imag = re, im
        moved = np.array(xs[j], copy=True)
        moved[INSIDE] = new[INSIDE]
        out.append(moved)
    return out


def transform(states, W):
    """states: the r members' dicts -> the r new dicts"""
    columns = {n: transform_variable([np.asarray(x[n]) for x in states], W) for n in NAMES}
    return [{n: columns[n][j] for n in NAMES} for j in range(len(states))]
