// The index sets of the triangular truncation, in one place, for host and device.
//
// A spectral field is stored as the rectangle [n = 32][m = 31] of complex128 (coefficient k = m + 31 n), but the reference's
// Legendre transforms only ever touch a triangle of it (nsh2, legendre.f90:73):
//   inverse (legendre.f90:150-161) reads  input(m, n) for m + n <= 31               527 coefficients
//   direct  (legendre.f90:187, 206-217) sets output = 0 and fills n <= 30, m + n <= 31   526 coefficients
// The work arrays that only the forward transforms of a model step write and only spectral_step_kernel reads are therefore
// kept PACKED: the filled coefficients in (n, m) order, row n behind the rows before it (31, 31, 30, 29, ..., 2 long for
// n = 0 ... 30), padded to whole 128-byte lines.
#pragma once
#include "tables.hpp"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SPD_TRI_HD __host__ __device__
#else
#define SPD_TRI_HD
#endif

namespace spd {
namespace tri {

constexpr int kFilled = 526;                       // coefficients the direct transform fills
constexpr int kPacked = 528;                       // ... padded to whole 128-byte lines: a packed field is 8448 B = 33 x 256
static_assert(kPacked >= kFilled && kPacked * 16 % 256 == 0, "a packed field keeps the arena's 256-byte carving");

// read by the inverse Legendre transform
SPD_TRI_HD constexpr bool inv_needed(int m, int n) { return m + n <= TRUNC + 1; }
// written (anything but +0.0) by the direct Legendre transform
SPD_TRI_HD constexpr bool fwd_filled(int m, int n) { return n <= TRUNC && m + n <= TRUNC + 1; }

// first packed index of row n (1 <= n <= 31): 31 + sum over j = 1 ... n-1 of (32 - j); row 0 starts at 0
SPD_TRI_HD constexpr int row_start(int n) { return n == 0 ? 0 : MX + (n - 1) * (TRUNC + 2) - (n - 1) * n / 2; }
// packed index of a filled coefficient (meaningless where fwd_filled does not hold)
SPD_TRI_HD constexpr int packed_index(int m, int n) { return row_start(n) + m; }

static_assert(row_start(1) == 31 && row_start(2) == 62 && row_start(3) == 92, "rows are 31, 31, 30, ... long");
static_assert(packed_index(1, TRUNC) == kFilled - 1, "the last filled coefficient is (m = 1, n = 30)");

// Beyond the halo: vort2vel's n + 1 neighbour reaches the row m + n = 32 and nothing the model computes looks further, so a
// coefficient with m + n >= 33 only ever feeds itself (spectral_step_kernel carries it forward from its own two time levels).
SPD_TRI_HD constexpr bool beyond_halo(int m, int n) { return m + n >= TRUNC + 3; }

// spectral_step_kernel gives a wavefront one BLOCK of 8 consecutive coefficients k = m + 31 n (one 128-byte line per level).
// A block is dead when all 8 of its coefficients lie beyond the halo; the mask over the 124 blocks is two 64-bit words.
constexpr int kBlock = 8, kBlocks = MX * NX / kBlock;
static_assert(MX * NX % kBlock == 0 && kBlocks == 124, "124 blocks of 8 coefficients");
SPD_TRI_HD constexpr bool block_is_dead(int b) {
    bool dead = true;
    for (int k = kBlock * b; k < kBlock * (b + 1); ++k) dead = dead && beyond_halo(k % MX, k / MX);
    return dead;
}
SPD_TRI_HD constexpr unsigned long long dead_word(int word) {
    unsigned long long bits = 0;
    for (int b = 64 * word; b < 64 * (word + 1) && b < kBlocks; ++b) bits |= static_cast<unsigned long long>(block_is_dead(b)) << (b - 64 * word);
    return bits;
}
constexpr unsigned long long kDeadLo = dead_word(0), kDeadHi = dead_word(1);
// (a run-time block index against the compile-time mask)
SPD_TRI_HD constexpr bool dead_block(int b) { return ((b < 64 ? kDeadLo >> b : kDeadHi >> (b - 64)) & 1ull) != 0; }

constexpr int popcount64(unsigned long long x) { return x == 0 ? 0 : static_cast<int>(x & 1ull) + popcount64(x >> 1); }
constexpr int kDeadBlocks = popcount64(kDeadLo) + popcount64(kDeadHi);
constexpr int count_beyond_halo() {
    int c = 0;
    for (int k = 0; k < MX * NX; ++k) c += beyond_halo(k % MX, k / MX) ? 1 : 0;
    return c;
}
static_assert(kDeadBlocks == 31, "31 of the 124 blocks lie wholly beyond the halo");
static_assert(kDeadBlocks * kBlock == 248 && count_beyond_halo() == 435, "248 of the 435 coefficients beyond the halo are in dead blocks");
static_assert(!dead_block(0) && dead_block(kBlocks - 1) && !block_is_dead(4), "(0, 0) is alive, (30, 31) is dead, (1, 1) is alive");

}  // namespace tri
}  // namespace spd
