"""CPU tier: the coefficient blocks of csrc/triangle.hpp that lie wholly beyond the truncation's halo (m + n >= 33), which the
multi-step calls leave alone for members that hold nothing there (tests/test_quiet_rim_gpu.py), against the same set
recomputed here from (m, n).

Device layout of a spectral field: complex128 [32 n][31 m], coefficient k = m + 31 n; spectral_step_kernel gives a wavefront one
block of 8 consecutive k.  Registry layout: (31 m, 32 n[, 8][, 2])."""
import numpy as np
import pytest

import quiet_rim_cases as qr
import triangle_cases as tc
from test_triangle_cpu import host_table


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(golden_dir + "/step.npz")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def test_the_dead_blocks_are_what_the_index_sets_give():
    assert qr.DEAD_BLOCKS.shape == (124,) and qr.DEAD_BLOCKS.sum() == 31
    assert qr.DEAD.shape == (31, 32) and qr.DEAD.sum() == 248
    assert (tc.L >= 33).sum() == 435 and tc.L[qr.DEAD].min() >= 33
    # no coefficient of the triangle or of the halo row is in a dead block
    assert not (qr.DEAD & (tc.L <= 32)).any() and not (qr.DEAD & tc.HALO).any() and not (qr.DEAD & tc.INV_NEEDED).any()
    # without the halo row 36 blocks would be dead: the halo keeps 5 of them alive
    beyond_triangle = np.zeros(992, dtype=bool)
    beyond_triangle[qr.K.ravel()] = (tc.L >= 32).ravel()
    assert beyond_triangle.reshape(124, 8).all(axis=1).sum() == 36


def test_the_dead_blocks_of_the_library(hip_lib):
    t = host_table(hip_lib, "tri_dead_blocks")
    assert t.shape == (124,)
    assert np.array_equal(t == 1.0, qr.DEAD_BLOCKS) and np.array_equal(t == 0.0, ~qr.DEAD_BLOCKS)


def test_the_golden_initial_state_is_plus_zero_on_the_dead_blocks(gold):
    for n in ("vor", "div", "t", "tr", "ps", "phis"):
        assert not bits(gold["s0_" + n][qr.DEAD]).any(), n
        assert gold["s0_" + n][~qr.DEAD].any(), n
    for n in ("tcorh", "qcorh"):
        assert not bits(gold["tab_" + n][qr.DEAD]).any(), n
