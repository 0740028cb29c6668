"""The filter tape restated in numpy and in Python floats (include/pyspeedy_amd.h: spd_model_filtape_*).  The
arbiter of tests/test_filtape_cpu.py and tests/test_filtape_gpu.py: it shares nothing with pyspeedy_amd/csrc/.

A section is (b0, b1, b2, a1, a2), a0 = 1.  Its zero-frequency gain is g = ((b0 + b1) + b2) / ((1 + a1) + a2).  For filter sample 1
a section starts in the steady state of a constant input: y = g x, s1 = y - b0 x, s2 = b2 x - a2 y; afterwards it is the transposed
direct form II with both state updates from the state before the sample: y = b0 x + s1, s1 <- (b1 x - a1 y) + s2, s2 <- b2 x - a2 y.
The sections run in order.  numpy's elementwise operators round every operation on its own and fuse nothing, and so do Python's
floats, which is all the definition asks for."""
import numpy as np

MEAN, COV, LAST = 0, 1, 2
MAX_SECTIONS, MAX_FILTERS, MAX_PLANES, MAX_ENTRIES = 4, 8, 32, 64


def stable(section):
    b0, b1, b2, a1, a2 = (float(v) for v in section)
    return all(np.isfinite(v) for v in (b0, b1, b2, a1, a2)) and abs(a2) < 1.0 and abs(a1) < 1.0 + a2


def gain(section):
    b0, b1, b2, a1, a2 = (float(v) for v in section)
    return ((b0 + b1) + b2) / ((1.0 + a1) + a2)


def filter_scalar(sections, xs):
    """a series of Python floats through the cascade from filter sample 1 on -> list of Python floats"""
    sections = [tuple(float(v) for v in s) for s in sections]
    state = [[0.0, 0.0] for _ in sections]
    out = []
    for i, x in enumerate(xs):
        v = float(x)
        for k, (b0, b1, b2, a1, a2) in enumerate(sections):
            if i == 0:
                y = gain(sections[k]) * v
                s1 = y - b0 * v
            else:
                y = b0 * v + state[k][0]
                s1 = (b1 * v - a1 * y) + state[k][1]
            s2 = b2 * v - a2 * y
            state[k] = [s1, s2]
            v = y
        out.append(v)
    return out


def filter_series(sections, x):
    """x: float64 array [T][...], sample after sample along axis 0 from filter sample 1 on -> y of the same shape"""
    x = np.asarray(x, dtype=np.float64)
    sections = [tuple(np.float64(v) for v in s) for s in sections]
    gains = [np.float64(gain(s)) for s in sections]
    state = [None] * len(sections)
    y = np.empty_like(x)
    for i in range(x.shape[0]):
        v = x[i]
        for k, (b0, b1, b2, a1, a2) in enumerate(sections):
            if i == 0:
                out = gains[k] * v
                s1 = out - b0 * v
            else:
                out = b0 * v + state[k][0]
                s1 = (b1 * v - a1 * out) + state[k][1]
            s2 = b2 * v - a2 * out
            state[k] = (s1, s2)
            v = out
        y[i] = v
    return y


def reduce_windows(ya, yb, op, windows):
    """ya, yb: filtered series [T][...] (yb is read by COV only); windows: per window the indices of its COUNTED samples in sample
    order -> [W][...]: the sum from the first counted value itself in sample order and one division by their number (MEAN, COV), the
    last counted value (LAST), quiet NaN for a window without one"""
    out = []
    for idx in windows:
        if not idx:
            out.append(np.full(ya.shape[1:], np.nan))
        elif op == LAST:
            out.append(ya[idx[-1]].copy())
        else:
            value = (lambda k: ya[k] * yb[k]) if op == COV else (lambda k: ya[k])
            s = value(idx[0]).copy()
            for k in idx[1:]:
                s = s + value(k)
            out.append(s / np.float64(len(idx)))
    return np.stack(out) if out else np.empty((0,) + ya.shape[1:])


def counted_windows(rows, step0, sample_steps, spinup, first_k=1):
    """rows: the schedule's closed windows (step after the window in column 0), the first of which opened at step0; sample_steps:
    the step of each sample of the series, whose sample 0 is filter sample `first_k` -> per window the indices of the samples that
    lie in it and whose filter sample number is beyond the spin-up"""
    out, prev = [], step0
    for row in rows:
        out.append([i for i, s in enumerate(sample_steps) if prev < s <= row[0] and first_k + i > spinup])
        prev = row[0]
    return out


def magnitude2(sections, omega):
    """|H(e^{i omega})|^2 of a cascade"""
    z = np.exp(-1j * np.asarray(omega, dtype=np.float64))
    h = np.ones_like(z)
    for b0, b1, b2, a1, a2 in sections:
        h = h * (b0 + b1 * z + b2 * z * z) / (1.0 + a1 * z + a2 * z * z)
    return np.abs(h) ** 2


def butterworth_magnitude2(kind, order, periods, sample_interval, omega):
    """the analytic 1 / (1 + W^(2 N)) of a bilinear-transformed Butterworth filter with pre-warped edges at the digital frequencies
    omega (radians per sample), and the digital frequencies of its edges and, for a band-pass, of its centre"""
    warped = np.sort(np.tan(np.pi * float(sample_interval) / np.atleast_1d(np.asarray(periods, dtype=np.float64))))
    t = np.tan(0.5 * np.asarray(omega, dtype=np.float64))
    if kind == "lowpass":
        w = t / warped[0]
    elif kind == "highpass":
        w = warped[0] / t
    else:
        w = (t * t - warped[0] * warped[1]) / ((warped[1] - warped[0]) * t)
    special = list(2.0 * np.arctan(warped))
    if kind == "bandpass":
        special.append(2.0 * np.arctan(np.sqrt(warped[0] * warped[1])))
    return 1.0 / (1.0 + w ** (2 * int(order))), np.array(special)
