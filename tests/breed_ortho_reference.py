"""The arbiter of the orthonormalised-breeding tests: numpy fp64, Python floats and math.fsum, written from the definition
(include/pyspeedy_amd.h), sharing nothing with csrc/.

States, elm2 and weights are those of tests/breed_reference.py.  A family is a list of member states in ascending member index and
the state xc of their control; D_j = X_j - X_c.

    B_P(i, j) = f_P sum [elm2] w_m (Re D_i Re D_j + Im D_i Im D_j) on time level 1 for m + n <= 31,   G_ij = sum_P weight_P B_P(i, j)
    G = R^T R (R upper triangular, the family breaks at the first radicand that is not a finite number > 0),  C = target R^-1
    X'_j = X_c + C_1j D_1 + ... + C_jj D_j on both time levels for m + n <= 31, for j below the rank

gram() sums with math.fsum (the device's order of summation is its own: it is held to this within a bound); factor() and
transform() round every operation on its own in the order of the definition, which the device must restate bit for bit."""
import math

import numpy as np

import breed_reference as ref

NAMES = ref.NAMES
INSIDE = ref.INSIDE


def _planes(x, name):
    """time level 1 of a variable as a list of (31, 32) planes"""
    a = np.asarray(x[name])[..., 0]
    return [a] if a.ndim == 2 else [a[:, :, k] for k in range(a.shape[2])]


def _plane_factor(name, elm2):
    return (0.25 * np.asarray(elm2) * ref.W_M if name in ("vor", "div") else 0.5 * ref.W_M * np.ones((31, 32)))[INSIDE]


def weighted_vector(x, xc, weights, elm2):
    """The real vector v of a member with v_i . v_j = G_ij: sqrt(weight f [elm2] w_m) times the real and imaginary parts of D over
    the 33 planes x 527 coefficients."""
    out = []
    for n in NAMES:
        w = np.atleast_1d(np.asarray(weights.get(n, np.zeros(8)), dtype=np.float64))
        f = _plane_factor(n, elm2)
        for k, (p, c) in enumerate(zip(_planes(x, n), _planes(xc, n))):
            d = (p - c)[INSIDE]
            s = np.sqrt(float(w[k]) * f)
            out += [s * d.real, s * d.imag]
    return np.concatenate(out)


def pair_terms(xi, xj, xc, weights, elm2):
    """All 34 782 terms of G_ij, each with its plane's weight applied (signed unless i = j)"""
    out = []
    for n in NAMES:
        w = np.atleast_1d(np.asarray(weights.get(n, np.zeros(8)), dtype=np.float64))
        f = _plane_factor(n, elm2)
        for k, (pi, pj, c) in enumerate(zip(_planes(xi, n), _planes(xj, n), _planes(xc, n))):
            di, dj = (pi - c)[INSIDE], (pj - c)[INSIDE]
            out += [float(w[k]) * (f * (di.real * dj.real)), float(w[k]) * (f * (di.imag * dj.imag))]
    terms = np.concatenate(out)
    assert terms.shape == (33 * 527 * 2,)
    return terms


def gram(members, xc, weights, elm2):
    """(G, S): G_ij = math.fsum of the pair's terms, S_ij = math.fsum of their absolute values (the scale of a summation error)"""
    r = len(members)
    g, s = np.zeros((r, r)), np.zeros((r, r))
    for i in range(r):
        for j in range(i, r):
            t = pair_terms(members[i], members[j], xc, weights, elm2)
            g[i, j] = g[j, i] = math.fsum(t)
            s[i, j] = s[j, i] = math.fsum(np.abs(t))
    return g, s


def factor(g, target):
    """(R, C, rank) of the definition from the upper triangle of g, every operation a Python float operation (IEEE double, one
    rounding each).  R and C are (r, r) arrays, 0.0 outside the upper triangle of the first `rank` rows and columns."""
    r = len(g)
    G = [[float(g[i][j]) for j in range(r)] for i in range(r)]
    R = [[0.0] * r for _ in range(r)]
    target = float(target)
    rank = r
    for j in range(r):
        for i in range(j):
            acc = G[i][j]
            for k in range(i):
                acc = acc - R[k][i] * R[k][j]
            R[i][j] = acc / R[i][i]
        d = G[j][j]
        for k in range(j):
            d = d - R[k][j] * R[k][j]
        if not (d > 0.0 and d < math.inf):
            rank = j
            break
        R[j][j] = math.sqrt(d)
    C = [[0.0] * r for _ in range(r)]
    for j in range(rank):
        C[j][j] = target / R[j][j]
        for i in range(j - 1, -1, -1):
            acc = 0.0
            for k in range(i + 1, j + 1):
                acc = acc + R[i][k] * C[k][j]
            C[i][j] = (-acc) / R[i][i]
    R, C = np.array(R).reshape(r, r), np.array(C).reshape(r, r)
    R[rank:], R[:, rank:] = 0.0, 0.0
    return R, C, rank


def combine(parts, c, j):
    """C_1j D_1 + ... + C_jj D_j of real arrays `parts` (0-based j), in the definition's order"""
    acc = np.float64(c[0, j]) * parts[0]
    for i in range(1, j + 1):
        acc = acc + np.float64(c[i, j]) * parts[i]
    return acc


def transform_variable(xs, xc, c, rank):
    """One variable of a family, both time levels: the list of the members' new arrays (members from `rank` on: untouched)"""
    xs, xc = [np.asarray(x) for x in xs], np.asarray(xc)
    re, im = [x.real - xc.real for x in xs[:rank]], [x.imag - xc.imag for x in xs[:rank]]
    out = []
    for j, x in enumerate(xs):
        new = x.copy()
        if j < rank:
            moved = np.empty_like(x)
            moved.real = xc.real + combine(re, c, j)
            moved.imag = xc.imag + combine(im, c, j)
            new[INSIDE] = moved[INSIDE]
        out.append(new)
    return out


def transform(members, xc, c, rank):
    """The list of the members' new states (dict name -> array)"""
    per_name = {n: transform_variable([x[n] for x in members], xc[n], c, rank) for n in NAMES}
    return [{n: per_name[n][j] for n in NAMES} for j in range(len(members))]


def families(control):
    """dict control -> the ascending list of its bred members"""
    out = {}
    for i, c in enumerate(control):
        if c >= 0:
            out.setdefault(int(c), []).append(i)
    return out
