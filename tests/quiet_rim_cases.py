"""Helper of the quiet-rim tests (not a test): the coefficient blocks that lie wholly beyond the truncation's halo, recomputed
from (m, n), in the registry layout of a spectral array: complex (31 m, 32 n[, 8 levels][, 2 time levels]).

On the device a spectral field is [32 n][31 m], coefficient k = m + 31 n, and the spectral step gives a wavefront one block of 8
consecutive k (one 128-byte line per level).  Nothing the model computes looks at a coefficient with m + n >= 33 (the inverse
transform reads m + n <= 31, vort2vel reaches the halo row m + n = 32), so a block whose 8 coefficients all lie there is dead."""
import numpy as np

_M, _N = np.meshgrid(np.arange(31), np.arange(32), indexing="ij")  # (31, 32): m, n of the registry layout
K = _M + 31 * _N                                                    # coefficient index on the device
_beyond = np.zeros(992, dtype=bool)
_beyond[K.ravel()] = (_M + _N >= 33).ravel()
DEAD_BLOCKS = _beyond.reshape(124, 8).all(axis=1)                   # [124 blocks of 8 coefficients]
DEAD = DEAD_BLOCKS[K // 8]                                          # (31, 32): the coefficients of the dead blocks
