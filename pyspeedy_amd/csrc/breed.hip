// Breeding: rescale the perturbation of a bred member against its control run (spd_model_breed_*, include/pyspeedy_amd.h;
// DESIGN section 4i).
//
// For a bred member p with control c, D = X_p - X_c on time level 1, w_m = 1 for m = 0 and 2 otherwise, over the 527 coefficients
// with m + n <= 31 of a plane (a level of vor, div, t, tr, or ps):
//   E(vor | div, k) = 1/4 sum elm2(m + n) w_m |D|^2        E(t | tr | ps, k) = 1/2 sum w_m |D|^2
//   A = sqrt(sum over the 33 planes of weight * E),  s = target / A,  X_p' = X_c + s * (X_p - X_c) on both time levels.
// Two launches.  breed_norm_kernel: a workgroup per (plane, bred member) reads the plane of both members with 16-byte loads -- a lane
// holds the coefficients k = lane, lane + 256, lane + 512, lane + 768 and adds their terms in that order -- and the 256 lane sums
// go through a tree in the LDS whose shape is fixed; one partial per plane and member is left in device scratch.  Nothing is
// atomic and nothing depends on which members are bred, on the member groups, the rounds or the call length: A is the same bits in
// every plan.  breed_rescale_kernel: shaped like nudge_kernel; every workgroup first adds its member's 33 weighted partials in
// ascending plane order (the reduce at the launch boundary: the partials are complete when this launch starts), forms A and s
// uniformly, and then moves its coefficients.  Every operation is rounded on its own (no contraction, the __d*_rn intrinsics), so
// that numpy's xc + s * (xp - xc) gives the same bits.  A coefficient with m + n >= 32 is neither loaded nor stored: a quiet member
// stays quiet.  Only bred members are written, and a control is never bred: no workgroup reads what another one writes.
//
// Orthonormalised breeding (spd_model_breed_orthogonalize) replaces the two launches by three for the bred
// members that share a control: breed_gram_kernel (the Gram matrix of their differences, every pair summed in breed_norm_kernel's
// order), breed_factor_kernel (G = R^T R, C = target R^-1: breed_factor.hpp) and breed_transform_kernel (X'_j = X_c + sum C_ij D_i).
#include <hip/hip_runtime.h>

#include "breed.hpp"
#include "breed_factor.hpp"
#include "global_mem.hpp"
#include "model_state.hpp"
#include "tables.hpp"

namespace spd {

namespace {
constexpr int kT = 256;
constexpr int kBlocks = (NSPEC + kT - 1) / kT;  // 4 blocks (or 4 coefficients a lane) over the 992 coefficients
constexpr int kLmax = TRUNC + 1;                // the largest total wavenumber that takes part

// blockIdx.x: plane, blockIdx.y: bred member
__global__ __launch_bounds__(kT) void breed_norm_kernel(const BreedPlane *__restrict__ planes, const BreedPair *__restrict__ pairs,
                                                        const double *__restrict__ elm2, double *__restrict__ partial) {
#pragma clang fp contract(off)
    __shared__ double tree[kT];
    const BreedPlane d = planes[blockIdx.x];
    const BreedPair pr = pairs[blockIdx.y];
    const double *xp = d.state + pr.member * d.member_stride, *xc = d.state + pr.control * d.member_stride;
    double sum = 0.0;
    for (int j = 0; j < kBlocks; ++j) {
        const int k = j * kT + threadIdx.x;
        if (k >= NSPEC) break;
        const int n = k / MX, m = k - n * MX, l = m + n;
        if (l > kLmax) continue;
        const double2v p = load_pair(xp + 2 * k), c = load_pair(xc + 2 * k);
        const double dx = __dsub_rn(p.x, c.x), dy = __dsub_rn(p.y, c.y);
        double q = __dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy));
        if (m != 0) q = __dmul_rn(2.0, q);
        if (d.kinetic) q = __dmul_rn(elm2[MX * l], q);
        sum = __dadd_rn(sum, q);
    }
    tree[threadIdx.x] = sum;
    __syncthreads();
    for (int half = kT / 2; half > 0; half >>= 1) {
        if (threadIdx.x < half) tree[threadIdx.x] = __dadd_rn(tree[threadIdx.x], tree[threadIdx.x + half]);
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.y * kBreedPlanes + blockIdx.x] = __dmul_rn(d.kinetic ? 0.25 : 0.5, tree[0]);
}

// the amplitude of bred member b from its partials: ascending plane order; a plane of weight zero takes no part
__device__ __forceinline__ double amplitude_of(const BreedPlane *__restrict__ planes, const double *__restrict__ partial, int b) {
#pragma clang fp contract(off)
    double sum = 0.0;
    for (int p = 0; p < kBreedPlanes; ++p) {
        const double w = planes[p].weight;
        if (w != 0.0) sum = __dadd_rn(sum, __dmul_rn(w, partial[b * kBreedPlanes + p]));
    }
    return __dsqrt_rn(sum);
}

// blockIdx.x: coefficients, blockIdx.y: plane, blockIdx.z: bred member
__global__ __launch_bounds__(kT) void breed_rescale_kernel(const BreedPlane *__restrict__ planes, const BreedPair *__restrict__ pairs,
                                                           const double *__restrict__ partial, double target,
                                                           double *__restrict__ amplitude, double *__restrict__ factor) {
#pragma clang fp contract(off)
    const int b = blockIdx.z;
    const BreedPair pr = pairs[b];
    const double a = amplitude_of(planes, partial, b);
    const bool alone = !(a > 0.0) || !(a < __builtin_inf());  // zero or not finite: s = 1 and not one bit of the member moves
    const double s = alone ? 1.0 : __ddiv_rn(target, a);
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
        if (amplitude) amplitude[pr.member] = a;
        if (factor) factor[pr.member] = s;
    }
    if (alone) return;
    const int k = blockIdx.x * kT + threadIdx.x;
    if (k >= NSPEC) return;
    const int n = k / MX, l = k - n * MX + n;
    if (l > kLmax) return;
    const BreedPlane d = planes[blockIdx.y];
    double *p0 = d.state + pr.member * d.member_stride + 2 * k, *p1 = p0 + d.level_stride;
    const double *c0 = d.state + pr.control * d.member_stride + 2 * k, *c1 = c0 + d.level_stride;
    const double2v xc = load_pair(c0), yc = load_pair(c1);
    double2v x = load_pair(p0), y = load_pair(p1);
    x.x = __dadd_rn(xc.x, __dmul_rn(s, __dsub_rn(x.x, xc.x)));
    x.y = __dadd_rn(xc.y, __dmul_rn(s, __dsub_rn(x.y, xc.y)));
    y.x = __dadd_rn(yc.x, __dmul_rn(s, __dsub_rn(y.x, yc.x)));
    y.y = __dadd_rn(yc.y, __dmul_rn(s, __dsub_rn(y.y, yc.y)));
    store_pair(p0, x);
    store_pair(p1, y);
}

// a lane per member
__global__ __launch_bounds__(kT) void breed_amplitude_kernel(const BreedPlane *__restrict__ planes, const int *__restrict__ slot_of, int members,
                                                             const double *__restrict__ partial, double *__restrict__ out) {
    const int i = blockIdx.x * kT + threadIdx.x;
    if (i >= members) return;
    const int b = slot_of[i];
    out[i] = b < 0 ? 0.0 : amplitude_of(planes, partial, b);
}

// ---- orthonormalised breeding: Gram matrix of a family, its factor, the triangular recombination ----
constexpr int kTile = 8;              // the Gram kernel serves kTile x kTile pairs of one (plane, family)
constexpr int kTreeBatch = 16;        // pairs whose 256 lane sums go through the LDS tree together (32 KB)
constexpr int kW = 64;                // lanes (one wave) and coefficients of a transform workgroup
constexpr int kChunks = (NSPEC + kW - 1) / kW;
constexpr int kLD = kBreedMaxFamily;

// blockIdx.x: plane, blockIdx.y: tile (ti <= tj) of the family's pairs, blockIdx.z: family.  B_P(i, j) of the differences of the
// family's members i and j against their control, for the pairs i <= j of the tile.  The terms of a pair are those of
// breed_norm_kernel with dx_i dx_j + dy_i dy_j for dx^2 + dy^2 and are added in its order -- a lane's coefficients lane, + 256,
// + 512, + 768, then the tree 128 ... 1 over the lanes -- whatever the tile: B_P(j, j) is breed_norm_kernel's partial bit for bit.
// A lane keeps the 64 sums of its tile in registers and the differences of 16 members at one coefficient at a time.
__global__ __launch_bounds__(kT) void breed_gram_kernel(const BreedPlane *__restrict__ planes, const BreedFamily *__restrict__ fams,
                                                        const int *__restrict__ members, const double *__restrict__ elm2,
                                                        double *__restrict__ partial) {
#pragma clang fp contract(off)
    __shared__ double tree[kTreeBatch][kT];
    const BreedFamily fam = fams[blockIdx.z];
    const int r = fam.count;
    int tj = 0, ti = blockIdx.y;
    while (ti > tj) ti -= ++tj;  // (tile t = tj (tj + 1) / 2 + ti)
    if (tj * kTile >= r) return;
    const BreedPlane d = planes[blockIdx.x];
    const double *xc = d.state + fam.control * d.member_stride;
    const double *row[kTile], *col[kTile];  // (a position beyond the family reads its last member: computed, never stored)
#pragma unroll
    for (int a = 0; a < kTile; ++a) {
        const int i = ti * kTile + a, j = tj * kTile + a;
        row[a] = d.state + members[fam.first + (i < r ? i : r - 1)] * d.member_stride;
        col[a] = d.state + members[fam.first + (j < r ? j : r - 1)] * d.member_stride;
    }
    double sum[kTile][kTile];
#pragma unroll
    for (int a = 0; a < kTile; ++a)
#pragma unroll
        for (int b = 0; b < kTile; ++b) sum[a][b] = 0.0;
    for (int blk = 0; blk < kBlocks; ++blk) {
        const int k = blk * kT + threadIdx.x;
        if (k >= NSPEC) break;
        const int n = k / MX, m = k - n * MX, l = m + n;
        if (l > kLmax) continue;
        const double2v c = load_pair(xc + 2 * k);
        const double e = elm2[MX * l];
        double2v di[kTile], dj[kTile];
#pragma unroll
        for (int a = 0; a < kTile; ++a) {
            const double2v p = load_pair(row[a] + 2 * k), q = load_pair(col[a] + 2 * k);
            di[a].x = __dsub_rn(p.x, c.x), di[a].y = __dsub_rn(p.y, c.y);
            dj[a].x = __dsub_rn(q.x, c.x), dj[a].y = __dsub_rn(q.y, c.y);
        }
#pragma unroll
        for (int a = 0; a < kTile; ++a)
#pragma unroll
            for (int b = 0; b < kTile; ++b) {
                double q = __dadd_rn(__dmul_rn(di[a].x, dj[b].x), __dmul_rn(di[a].y, dj[b].y));
                if (m != 0) q = __dmul_rn(2.0, q);
                if (d.kinetic) q = __dmul_rn(e, q);
                sum[a][b] = __dadd_rn(sum[a][b], q);
            }
    }
    double *out = partial + fam.pair0 * kBreedPlanes + blockIdx.x;
#pragma unroll
    for (int batch = 0; batch < kTile * kTile / kTreeBatch; ++batch) {
#pragma unroll
        for (int q = 0; q < kTreeBatch; ++q) tree[q][threadIdx.x] = sum[(batch * kTreeBatch + q) / kTile][(batch * kTreeBatch + q) % kTile];
        __syncthreads();
        for (int half = kT / 2; half > 0; half >>= 1) {  // kTreeBatch trees side by side, every one in the order 128 ... 1
            for (int w = threadIdx.x; w < kTreeBatch * half; w += kT) {
                const int q = w / half, t = w - q * half;
                tree[q][t] = __dadd_rn(tree[q][t], tree[q][t + half]);
            }
            __syncthreads();
        }
        if (threadIdx.x < kTreeBatch) {
            const int pq = batch * kTreeBatch + threadIdx.x;
            const long i = ti * kTile + pq / kTile, j = tj * kTile + pq % kTile;
            if (i <= j && j < r) out[(j * (j + 1) / 2 + i) * kBreedPlanes] = __dmul_rn(d.kinetic ? 0.25 : 0.5, tree[threadIdx.x][0]);
        }
        __syncthreads();
    }
}

// G of one pair from its partials: ascending plane order; a plane of weight zero takes no part (amplitude_of's sum)
__device__ __forceinline__ double gram_of(const BreedPlane *__restrict__ planes, const double *__restrict__ pair_partial) {
#pragma clang fp contract(off)
    double sum = 0.0;
    for (int p = 0; p < kBreedPlanes; ++p) {
        const double w = planes[p].weight;
        if (w != 0.0) sum = __dadd_rn(sum, __dmul_rn(w, pair_partial[p]));
    }
    return sum;
}

// blockIdx.x: family.  G from the partials, then breed_factor (breed_factor.hpp) with a lane per column; C goes to device memory
// for the transform, R's diagonal and target / R_jj to the ring slot, the number of members to transform to rank[family].  The
// members from the break on show amplitude 0.0 and factor 1.0, as a member that plain breeding leaves alone.
__global__ __launch_bounds__(kT) void breed_factor_kernel(const BreedPlane *__restrict__ planes, const BreedFamily *__restrict__ fams,
                                                          const int *__restrict__ members, const double *__restrict__ partial, double target,
                                                          double *__restrict__ coef, int *__restrict__ rank, double *__restrict__ amplitude,
                                                          double *__restrict__ factor) {
    __shared__ double a[kLD * kLD], c[kLD * kLD];
    const BreedFamily fam = fams[blockIdx.x];
    const int r = fam.count;
    for (int e = threadIdx.x; e < r * r; e += kT) {
        const long i = e / r, j = e - i * r;
        if (i <= j) a[i * kLD + j] = gram_of(planes, partial + (fam.pair0 + j * (j + 1) / 2 + i) * kBreedPlanes);
    }
    __syncthreads();
    const int rk = breed_factor(a, c, r, target, static_cast<int>(threadIdx.x), kT, [] { __syncthreads(); });
    double *out = coef + static_cast<long>(blockIdx.x) * kLD * kLD;
    for (int e = threadIdx.x; e < rk * kLD; e += kT) {
        const int i = e / kLD, j = e - i * kLD;
        out[e] = i <= j && j < rk ? c[e] : 0.0;
    }
    for (int j = threadIdx.x; j < r; j += kT) {
        const int p = members[fam.first + j];
        if (amplitude) amplitude[p] = j < rk ? a[j * kLD + j] : 0.0;
        if (factor) factor[p] = j < rk ? c[j * kLD + j] : 1.0;
    }
    if (threadIdx.x == 0) rank[blockIdx.x] = rk;
}

// blockIdx.x: 64 coefficients, blockIdx.y: 2 * plane + time level, blockIdx.z: family.  X'_j = X_c + C_1j D_1 + ... + C_jj D_j for
// the members j below the family's rank, D_i = X_i - X_c of the members as they stand: the workgroup (one wave) loads the control
// and every member of its coefficients once, keeps the differences in the LDS (a lane reads back only what it wrote: no barrier),
// forms eight members at a time and stores them.  It owns its coefficients of the whole family, so no workgroup reads what
// another writes.  C is uniform: scalar loads.  A coefficient with m + n >= 32 and a member at or beyond the rank are neither
// loaded nor stored.
__global__ __launch_bounds__(kW) void breed_transform_kernel(const BreedPlane *__restrict__ planes, const BreedFamily *__restrict__ fams,
                                                            const int *__restrict__ members, const double *__restrict__ coef,
                                                            const int *__restrict__ rank) {
#pragma clang fp contract(off)
    constexpr int kJ = 8;
    __shared__ double2v delta[kLD][kW];
    const int rk = rank[blockIdx.z];
    const int k = blockIdx.x * kW + threadIdx.x;
    if (rk <= 0 || rk > kLD || k >= NSPEC) return;
    const int n = k / MX, l = k - n * MX + n;
    if (l > kLmax) return;
    const BreedFamily fam = fams[blockIdx.z];
    const BreedPlane d = planes[blockIdx.y >> 1];
    double *base = d.state + (blockIdx.y & 1) * d.level_stride + 2 * k;
    const double2v xc = load_pair(base + fam.control * d.member_stride);
    for (int i = 0; i < rk; ++i) {
        const double2v x = load_pair(base + members[fam.first + i] * d.member_stride);
        double2v v;
        v.x = __dsub_rn(x.x, xc.x), v.y = __dsub_rn(x.y, xc.y);
        delta[i][threadIdx.x] = v;
    }
    const double *cm = coef + static_cast<long>(blockIdx.z) * kLD * kLD;
    for (int j0 = 0; j0 < rk; j0 += kJ) {
        double2v acc[kJ];
        const double2v d0 = delta[0][threadIdx.x];
#pragma unroll
        for (int b = 0; b < kJ; ++b) acc[b].x = __dmul_rn(cm[j0 + b], d0.x), acc[b].y = __dmul_rn(cm[j0 + b], d0.y);
        for (int i = 1; i < j0; ++i) {  // rows above the block: every column takes part
            const double2v di = delta[i][threadIdx.x];
#pragma unroll
            for (int b = 0; b < kJ; ++b) {
                const double cij = cm[i * kLD + j0 + b];
                acc[b].x = __dadd_rn(acc[b].x, __dmul_rn(cij, di.x)), acc[b].y = __dadd_rn(acc[b].y, __dmul_rn(cij, di.y));
            }
        }
        const int top = j0 + kJ < rk ? j0 + kJ : rk;
        for (int i = j0 > 1 ? j0 : 1; i < top; ++i) {  // the block's triangle: column j takes the rows i <= j
            const double2v di = delta[i][threadIdx.x];
#pragma unroll
            for (int b = 0; b < kJ; ++b)
                if (i <= j0 + b) {
                    const double cij = cm[i * kLD + j0 + b];
                    acc[b].x = __dadd_rn(acc[b].x, __dmul_rn(cij, di.x)), acc[b].y = __dadd_rn(acc[b].y, __dmul_rn(cij, di.y));
                }
        }
#pragma unroll
        for (int b = 0; b < kJ; ++b)
            if (j0 + b < rk) {
                double2v x;
                x.x = __dadd_rn(xc.x, acc[b].x), x.y = __dadd_rn(xc.y, acc[b].y);
                store_pair(base + members[fam.first + j0 + b] * d.member_stride, x);
            }
    }
}

// a lane per entry of the [M][M] Gram matrix: G of two members of one family, 0.0 otherwise.  place[2 i]: the family of member i
// (-1: not bred), place[2 i + 1]: its position there.
__global__ __launch_bounds__(kT) void breed_gram_expand_kernel(const BreedPlane *__restrict__ planes, const BreedFamily *__restrict__ fams,
                                                              const int *__restrict__ place, int M, const double *__restrict__ partial,
                                                              double *__restrict__ out) {
    const long e = static_cast<long>(blockIdx.x) * kT + threadIdx.x;
    if (e >= static_cast<long>(M) * M) return;
    const int a = static_cast<int>(e / M), b = static_cast<int>(e - static_cast<long>(a) * M);
    const int fa = place[2 * a], fb = place[2 * b];
    double g = 0.0;
    if (fa >= 0 && fa == fb) {
        const long pa = place[2 * a + 1], pb = place[2 * b + 1], i = pa < pb ? pa : pb, j = pa < pb ? pb : pa;
        g = gram_of(planes, partial + (fams[fa].pair0 + j * (j + 1) / 2 + i) * kBreedPlanes);
    }
    out[e] = g;
}

}  // namespace

constexpr int kMaxZ = 32768;  // (grid.y and grid.z are limited to 65535: many bred members go out in pieces)

// The norm launch for the bred members pairs[0 ... nbred): partial[b][plane] = E(plane) of the difference X_p - X_c on time level 1,
// summed over the 527 coefficients with m + n <= 31 in an order that depends on nothing but the plane.
static hipError_t run_breed_norm(const BreedPlane *planes, const BreedPair *pairs, int nbred, const double *elm2, double *partial, hipStream_t s) {
    for (int z0 = 0; z0 < nbred; z0 += kMaxZ) {
        const int nz = nbred - z0 < kMaxZ ? nbred - z0 : kMaxZ;
        hipLaunchKernelGGL(breed_norm_kernel, dim3(kBreedPlanes, nz), dim3(kT), 0, s, planes, pairs + z0, elm2,
                           partial + static_cast<long>(z0) * kBreedPlanes);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// The rescale launch behind it.  Every workgroup sums its member's 33 weighted partials in ascending plane order:
//   A = sqrt(sum weight[plane] * partial[b][plane]),  s = target / A  (s = 1 and the member left alone if A is zero or not finite)
// and then X_p' = X_c + s * (X_p - X_c) on both time levels for the coefficients with m + n <= 31, each operation rounded on its
// own.  amplitude / factor: [M] of the ring slot, written at the member's index; either may be null.
static hipError_t run_breed_rescale(const BreedPlane *planes, const BreedPair *pairs, int nbred, const double *partial, double target,
                                    double *amplitude, double *factor, hipStream_t s) {
    for (int z0 = 0; z0 < nbred; z0 += kMaxZ) {
        const int nz = nbred - z0 < kMaxZ ? nbred - z0 : kMaxZ;
        hipLaunchKernelGGL(breed_rescale_kernel, dim3(kBlocks, kBreedPlanes, nz), dim3(kT), 0, s, planes, pairs + z0,
                           partial + static_cast<long>(z0) * kBreedPlanes, target, amplitude, factor);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// Amplitudes only, behind run_breed_norm: out[i] = A of member i, 0.0 for a member that is not bred (slot_of[i] < 0: its index in
// pairs otherwise).  Writes nothing else.
static hipError_t run_breed_amplitude(const BreedPlane *planes, const int *slot_of, int members, const double *partial, double *out, hipStream_t s) {
    if (members == 0) return hipSuccess;
    hipLaunchKernelGGL(breed_amplitude_kernel, dim3((members + kT - 1) / kT), dim3(kT), 0, s, planes, slot_of, members, partial, out);
    return hipGetLastError();
}

// The Gram launch for families fams[0 ... nfam): partial[pair][plane] = B_plane(i, j) for the pairs i <= j of every family, each
// summed in breed_norm_kernel's order.  largest: the size of the largest family (it sets the number of tiles).
static hipError_t run_breed_gram(const BreedPlane *planes, const BreedFamily *fams, int nfam, int largest, const int *members, const double *elm2,
                                 double *partial, hipStream_t s) {
    const int nt = (largest + kTile - 1) / kTile;
    for (int z0 = 0; z0 < nfam; z0 += kMaxZ) {
        const int nz = nfam - z0 < kMaxZ ? nfam - z0 : kMaxZ;
        hipLaunchKernelGGL(breed_gram_kernel, dim3(kBreedPlanes, nt * (nt + 1) / 2, nz), dim3(kT), 0, s, planes, fams + z0, members, elm2, partial);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// The factor and transform launches behind it: G = R^T R and C = target R^-1 per family (breed_factor.hpp), amplitude = R_jj and
// factor = target / R_jj at the members' indices of the ring slot, then X'_j = X_c + sum_{i <= j} C_ij (X_i - X_c) on both time
// levels for the coefficients with m + n <= 31 and the members below the family's rank.
static hipError_t run_breed_orthonormalise(const BreedPlane *planes, const BreedFamily *fams, int nfam, const int *members, const double *partial,
                                           double target, double *coef, int *rank, double *amplitude, double *factor, hipStream_t s) {
    for (int z0 = 0; z0 < nfam; z0 += kMaxZ) {
        const int nz = nfam - z0 < kMaxZ ? nfam - z0 : kMaxZ;
        hipLaunchKernelGGL(breed_factor_kernel, dim3(nz), dim3(kT), 0, s, planes, fams + z0, members, partial, target,
                           coef + static_cast<long>(z0) * kLD * kLD, rank + z0, amplitude, factor);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(breed_transform_kernel, dim3(kChunks, 2 * kBreedPlanes, nz), dim3(kW), 0, s, planes, fams + z0, members,
                           coef + static_cast<long>(z0) * kLD * kLD, rank + z0);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// The [M][M] Gram matrix behind run_breed_gram.  Writes nothing else.
static hipError_t run_breed_gram_expand(const BreedPlane *planes, const BreedFamily *fams, const int *place, int members, const double *partial,
                                        double *out, hipStream_t s) {
    const long entries = static_cast<long>(members) * members;
    if (entries == 0) return hipSuccess;
    hipLaunchKernelGGL(breed_gram_expand_kernel, dim3(static_cast<unsigned>((entries + kT - 1) / kT)), dim3(kT), 0, s, planes, fams, place, members,
                       partial, out);
    return hipGetLastError();
}

}  // namespace spd

// ---- host side: the step loop's rescale, the configuration and the C ABI (spd_model_breed_*, spd_breed_check) ----

namespace {
constexpr int kBreedNames = 5, kBreedRows = 8;  // weights: [5][8] for vor, div, t, tr, ps; ps reads entry 0 of its row
const char *const kBreedName[kBreedNames] = {"vor", "div", "t", "tr", "ps"};
const char *const kBreedOff = "no breeding configured (spd_model_breed_configure)";
int breed_levels(int id) { return id == 4 ? 1 : 8; }
}  // namespace

// The rescale of all bred members on the state as it stands, on stream s: the norm launch, the rescale launch behind it, one slot
// of the ring.  What the model derived from the state is dropped as spd_model_set drops it (the look-ahead geopotential, the day's
// interpolated climatologies); a range check that was put off looks at the state as it is now and goes out first.
int spd::breed_rescale(spd_model *m, hipStream_t s, const char *who) {
    spd_model::Breed &br = m->breed;
    if (br.nbred == 0) return SPD_OK;
    if (int rc = settle_deferred_check(m)) return rc;
    m->surf_cache_valid = m->phi_ahead = false;
    const size_t M = static_cast<size_t>(m->M), slot = static_cast<size_t>(br.ring.slot(br.ring.taken + 1));
    double *amplitude = br.data + slot * 2 * M;
    hipError_t e;
    if (br.ortho.on) {  // Gram matrix, factor and recombination of every family for norm and rescale of every member
        const spd_model::Breed::Ortho &o = br.ortho;
        e = run_breed_gram(br.planes, o.fams, o.families, o.largest, o.members, m->ctx->dev.elm2, o.partial, s);
        if (e == hipSuccess)
            e = run_breed_orthonormalise(br.planes, o.fams, o.families, o.members, o.partial, br.target, o.coef, o.rank, amplitude, amplitude + M, s);
    } else {
        e = run_breed_norm(br.planes, br.pairs, br.nbred, m->ctx->dev.elm2, br.partial, s);
        if (e == hipSuccess) e = run_breed_rescale(br.planes, br.pairs, br.nbred, br.partial, br.target, amplitude, amplitude + M, s);
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return m_fail(SPD_E_DEVICE, std::string(who) + ": breeding: " + hipGetErrorString(e));
    }
    ++br.ring.taken;
    br.ring.stamp(br.ring.taken, m->current_step, m->cal);
    ++br.applied;
    return SPD_OK;
}

// the checks of a control list, for spd_breed_check and spd_breed_family_check
static int breed_check_controls(const char *who, const int32_t *control, int members) {
    for (int i = 0; control && i < members; ++i) {
        const int c = control[i];
        if (c == -1) continue;
        if (c < -1 || c >= members)
            return m_fail(SPD_E_ARG, std::string(who) + ": the control of member " + std::to_string(i) + " (" + std::to_string(c) + ") is out of range (-1 ... " +
                                         std::to_string(members - 1) + ")");
        if (c == i) return m_fail(SPD_E_ARG, std::string(who) + ": member " + std::to_string(i) + " is its own control");
        if (control[c] != -1)
            return m_fail(SPD_E_ARG, std::string(who) + ": the control of member " + std::to_string(i) + " (" + std::to_string(c) +
                                         ") is itself bred: a control must have -1 (no chains)");
    }
    return SPD_OK;
}

// The families of a control list that passed its checks, by ascending control, each in ascending member index.
static std::map<int, std::vector<int>> breed_families(const int32_t *control, int members) {
    std::map<int, std::vector<int>> out;
    for (int i = 0; control && i < members; ++i)
        if (control[i] >= 0) out[control[i]].push_back(i);
    return out;
}

// the largest family's size, or -1 with the message if it cannot be orthogonalised
static int breed_family_limit(const std::map<int, std::vector<int>> &families) {
    int largest = 0;
    for (const auto &f : families) {
        const int size = static_cast<int>(f.second.size());
        if (size > spd::kBreedMaxFamily)
            return m_fail(SPD_E_ARG, "spd_model_breed_orthogonalize: the family of control " + std::to_string(f.first) + " has " + std::to_string(size) +
                                         " members: at most " + std::to_string(spd::kBreedMaxFamily) + " can be orthogonalised");
        largest = std::max(largest, size);
    }
    return largest;
}

// Free what spd_model_breed_orthogonalize allocated (the device is idle); plain breeding from here on.
static void ortho_release(spd_model::Breed &br) {
    if (br.ortho.alloc) (void)hipFree(br.ortho.alloc);
    br.ortho = spd_model::Breed::Ortho{};
}

// The families of the configuration, their member and pair lists, and the scratch of the three launches: one allocation.
static int ortho_build(spd_model *m, const char *who) {
    spd_model::Breed &br = m->breed;
    std::vector<int32_t> control(static_cast<size_t>(m->M), -1);
    for (const BreedPair &pr : br.host_pairs) control[pr.member] = pr.control;
    const auto families = breed_families(control.data(), m->M);
    spd_model::Breed::Ortho next;
    std::vector<BreedFamily> fams;
    std::vector<int> members, place(2 * static_cast<size_t>(m->M), -1);
    for (const auto &f : families) {
        const int count = static_cast<int>(f.second.size());
        for (int i = 0; i < count; ++i) {
            place[2 * f.second[i]] = static_cast<int>(fams.size());
            place[2 * f.second[i] + 1] = i;
        }
        fams.push_back({f.first, static_cast<int>(members.size()), count, next.pairs});
        members.insert(members.end(), f.second.begin(), f.second.end());
        next.pairs += static_cast<long>(count) * (count + 1) / 2;
        next.largest = std::max(next.largest, count);
    }
    next.families = static_cast<int>(fams.size());
    const size_t one = 1, nfam = std::max(fams.size(), one);
    const size_t fam_bytes = sample_up(nfam * sizeof(BreedFamily)), member_bytes = sample_up(std::max(members.size(), one) * sizeof(int));
    const size_t place_bytes = sample_up(place.size() * sizeof(int)), rank_bytes = sample_up(nfam * sizeof(int));
    const size_t partial_bytes = sample_up(std::max<size_t>(next.pairs, 1) * kBreedPlanes * sizeof(double));
    const size_t coef_bytes = sample_up(nfam * spd::kBreedMaxFamily * spd::kBreedMaxFamily * sizeof(double));
    const size_t total = fam_bytes + member_bytes + place_bytes + rank_bytes + partial_bytes + coef_bytes;
    void *p = nullptr;
    if (hipMalloc(&p, total) != hipSuccess) {
        (void)hipGetLastError();
        return m_fail(SPD_E_DEVICE, std::string(who) + ": cannot allocate the Gram partials and factors (" + std::to_string(total) + " bytes asked for)");
    }
    Carve carve{static_cast<char *>(p)};
    next.alloc = p;
    next.fams = carve.take<BreedFamily>(fam_bytes);
    next.members = carve.take<int>(member_bytes);
    next.place = carve.take<int>(place_bytes);
    next.rank = carve.take<int>(rank_bytes);
    next.partial = carve.take<double>(partial_bytes);
    next.coef = carve.take<double>(coef_bytes);
    hipError_t e = hipMemset(p, 0, total);
    if (e == hipSuccess && !fams.empty()) e = hipMemcpy(next.fams, fams.data(), fams.size() * sizeof(BreedFamily), hipMemcpyHostToDevice);
    if (e == hipSuccess && !members.empty()) e = hipMemcpy(next.members, members.data(), members.size() * sizeof(int), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(next.place, place.data(), place.size() * sizeof(int), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return upload_failed(who, e, p);
    br.ortho = next;
    return SPD_OK;
}

extern "C" {

int spd_breed_check(const int32_t *control, int members, const double *weights, double target, int every, int capacity, int in_loop) {
    const char *who = "spd_model_breed_configure";
    if (int rc = breed_check_controls(who, control, members)) return rc;
    if (!weights) return m_fail(SPD_E_ARG, std::string(who) + ": null weights");
    bool some = false;
    for (int v = 0; v < kBreedNames; ++v)
        for (int k = 0; k < breed_levels(v); ++k) {
            const double w = weights[v * kBreedRows + k];
            if (!std::isfinite(w) || w < 0.0)
                return m_fail(SPD_E_ARG, std::string(who) + ": the weight of '" + kBreedName[v] + "' at level " + std::to_string(k) +
                                             " is not a finite number >= 0");
            some = some || w > 0.0;
        }
    if (!some) return m_fail(SPD_E_ARG, std::string(who) + ": all weights are zero");
    if (!std::isfinite(target) || !(target > 0.0)) return m_fail(SPD_E_ARG, std::string(who) + ": target must be a finite number > 0");
    if (every < 1) return m_fail(SPD_E_ARG, std::string(who) + ": every must be at least 1");
    if (capacity < 1) return m_fail(SPD_E_ARG, std::string(who) + ": capacity must be at least 1");
    if (in_loop != 0 && in_loop != 1) return m_fail(SPD_E_ARG, std::string(who) + ": in_loop must be 0 or 1");
    return SPD_OK;
}

int spd_model_breed_configure(spd_model_handle m, const int32_t *control, const double *weights, double target, int every, int capacity,
                              int in_loop) {
    const char *who = "spd_model_breed_configure";
    // (the arguments first: what does not need the member count, then the model, then the controls)
    if (control)
        if (int rc = spd_breed_check(nullptr, 0, weights, target, every, capacity, in_loop)) return rc;
    if (int rc = configure_allowed(m, who)) return rc;
    if (control)
        if (int rc = spd_breed_check(control, m->M, weights, target, every, capacity, in_loop)) return rc;
    if (control && in_loop && m->assim.loops())
        return m_fail(SPD_E_ARG, std::string(who) + ": in-loop breeding cannot be configured while in-loop assimilation (spd_model_assim_configure) is: "
                                                    "both cut the call at their own steps; switch one of them off or to in_loop = 0");
    spd_model::Breed &br = m->breed;
    void *const ortho = br.ortho.alloc;  // (retired with the rest, behind retire's synchronisation)
    br.ortho.alloc = nullptr;
    const int retired = retire(m, br);
    if (ortho) (void)hipFree(ortho);
    if (retired) return retired;
    if (!control) return SPD_OK;  // off
    spd_model::Breed next;
    next.in_loop = in_loop != 0;
    next.every = every;
    next.target = target;
    const size_t M = static_cast<size_t>(m->M);
    std::vector<BreedPair> pairs;
    std::vector<int> slot_of(M, -1);
    for (int i = 0; i < m->M; ++i)
        if (control[i] >= 0) {
            slot_of[i] = static_cast<int>(pairs.size());
            pairs.push_back({i, control[i]});
        }
    next.nbred = static_cast<int>(pairs.size());
    next.host_pairs = pairs;
    if (static_cast<size_t>(capacity) > (static_cast<size_t>(-1) / 64) / M)
        return m_fail(SPD_E_ARG, std::string(who) + ": the ring's size does not fit size_t");
    std::vector<BreedPlane> planes;
    double *const base[kBreedNames] = {m->P.vor, m->P.div, m->P.t, m->P.tr, m->P.ps};
    for (int v = 0; v < kBreedNames; ++v)
        for (int k = 0; k < breed_levels(v); ++k) {
            const size_t levels = static_cast<size_t>(breed_levels(v));
            BreedPlane d{};
            d.state = base[v] + static_cast<size_t>(k) * NSPEC * C;
            d.member_stride = static_cast<long>(2 * levels * NSPEC * C);
            d.level_stride = static_cast<long>(levels * NSPEC * C);
            d.weight = weights[v * kBreedRows + k];
            d.kinetic = v < 2 ? 1 : 0;
            planes.push_back(d);
        }
    // one allocation: plane descriptors | pairs | each member's index among the pairs | partial norms | ring
    const size_t plane_bytes = sample_up(planes.size() * sizeof(BreedPlane)), pair_bytes = sample_up(std::max<size_t>(pairs.size(), 1) * sizeof(BreedPair));
    const size_t slot_bytes = sample_up(M * sizeof(int)), partial_bytes = sample_up(std::max<size_t>(pairs.size(), 1) * kBreedPlanes * sizeof(double));
    const size_t ring_doubles = static_cast<size_t>(capacity) * 2 * M, ring_bytes = sample_up(ring_doubles * sizeof(double));
    const size_t total = plane_bytes + pair_bytes + slot_bytes + partial_bytes + ring_bytes;
    void *p = nullptr;
    if (hipMalloc(&p, total) != hipSuccess) {  // breeding is off; the model is as usable as before
        (void)hipGetLastError();
        return m_fail(SPD_E_DEVICE, std::string(who) + ": cannot allocate the ring (" + std::to_string(total) + " bytes asked for: " +
                                        std::to_string(capacity) + " events); breeding is off");
    }
    Carve carve{static_cast<char *>(p)};
    next.alloc = p;
    next.planes = carve.take<BreedPlane>(plane_bytes);
    next.pairs = carve.take<BreedPair>(pair_bytes);
    next.slot_of = carve.take<int>(slot_bytes);
    next.partial = carve.take<double>(partial_bytes);
    next.data = carve.take<double>(ring_bytes);
    std::vector<double> ring(ring_doubles);  // what a member that is not bred shows: amplitude 0.0, factor 1.0
    for (size_t slot = 0; slot < static_cast<size_t>(capacity); ++slot) {
        std::fill(ring.begin() + slot * 2 * M, ring.begin() + slot * 2 * M + M, 0.0);
        std::fill(ring.begin() + slot * 2 * M + M, ring.begin() + (slot + 1) * 2 * M, 1.0);
    }
    hipError_t e = hipMemcpy(next.planes, planes.data(), planes.size() * sizeof(BreedPlane), hipMemcpyHostToDevice);
    if (e == hipSuccess && !pairs.empty()) e = hipMemcpy(next.pairs, pairs.data(), pairs.size() * sizeof(BreedPair), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(next.slot_of, slot_of.data(), M * sizeof(int), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(next.partial, 0, partial_bytes);
    if (e == hipSuccess) e = hipMemcpy(next.data, ring.data(), ring_doubles * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return upload_failed(who, e, p);
    next.ring = SampleRing(capacity, 6);
    next.on = true;
    br = std::move(next);
    return SPD_OK;
}

int spd_model_breed_apply(spd_model_handle m, void *stream) {
    const char *who = "spd_model_breed_apply";
    if (!m) return m_fail(SPD_E_ARG, std::string(who) + ": null model");
    if (int rc = usable(m, who)) return rc;
    if (!m->breed.on) return m_fail(SPD_E_ARG, std::string(who) + ": " + kBreedOff);
    if (!m->initialized) return m_fail(SPD_E_ARG, std::string(who) + ": model state not initialized");
    if (m->steps_pending) return m_fail(SPD_E_ARG, std::string(who) + ": a checked multi-step call is in flight; end it first");
    M_HIP(hipSetDevice(m->ctx->device));
    return breed_rescale(m, static_cast<hipStream_t>(stream), who);
}

int spd_model_breed_compute(spd_model_handle m, void *dst_device, size_t dst_bytes, void *stream) {
    const char *who = "spd_model_breed_compute";
    if (!m) return m_fail(SPD_E_ARG, std::string(who) + ": null model");
    if (int rc = usable(m, who)) return rc;
    const spd_model::Breed &br = m->breed;
    if (!br.on) return m_fail(SPD_E_ARG, std::string(who) + ": " + kBreedOff);
    if (!m->initialized) return m_fail(SPD_E_ARG, std::string(who) + ": model state not initialized");
    if (m->steps_pending) return m_fail(SPD_E_ARG, std::string(who) + ": a checked multi-step call is in flight; end it first");
    const size_t need = static_cast<size_t>(m->M) * sizeof(double);
    if (int rc = destination_fits(who, dst_device, dst_bytes, need, sizeof(double))) return rc;
    M_HIP(hipSetDevice(m->ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = run_breed_norm(br.planes, br.pairs, br.nbred, m->ctx->dev.elm2, br.partial, s);
    if (e == hipSuccess) e = run_breed_amplitude(br.planes, br.slot_of, m->M, br.partial, static_cast<double *>(dst_device), s);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return m_fail(SPD_E_DEVICE, std::string(who) + ": " + hipGetErrorString(e));
    }
    return SPD_OK;
}

int spd_breed_family_check(const int32_t *control, int members) {
    const char *who = "spd_breed_family_check";
    if (!control || members < 0) return m_fail(SPD_E_ARG, std::string(who) + ": null control");
    if (int rc = breed_check_controls(who, control, members)) return rc;
    return breed_family_limit(breed_families(control, members));
}

int spd_breed_factor_host(const double *gram, int r, double target, double *rdiag, double *coef, int *rank) {
    const char *who = "spd_breed_factor_host";
    if (!gram || !rdiag || !coef || !rank) return m_fail(SPD_E_ARG, std::string(who) + ": null argument");
    if (r < 1 || r > spd::kBreedMaxFamily)
        return m_fail(SPD_E_ARG, std::string(who) + ": r must be 1 ... " + std::to_string(spd::kBreedMaxFamily) + ", got " + std::to_string(r));
    constexpr int LD = spd::kBreedMaxFamily;
    std::vector<double> a(LD * LD, 0.0), c(LD * LD, 0.0);
    for (int i = 0; i < r; ++i)
        for (int j = i; j < r; ++j) a[i * LD + j] = gram[i * r + j];
    const int rk = spd::breed_factor(a.data(), c.data(), r, target, 0, 1, [] {});
    for (int i = 0; i < r; ++i) {
        rdiag[i] = i < rk ? a[i * LD + i] : 0.0;
        for (int j = 0; j < r; ++j) coef[i * r + j] = i <= j && j < rk ? c[i * LD + j] : 0.0;
    }
    *rank = rk;
    return SPD_OK;
}

int spd_model_breed_orthogonalize(spd_model_handle m, int on) {
    const char *who = "spd_model_breed_orthogonalize";
    if (int rc = configure_allowed(m, who)) return rc;
    spd_model::Breed &br = m->breed;
    if (!br.on) return m_fail(SPD_E_ARG, std::string(who) + ": " + kBreedOff);
    if (on != 0 && on != 1) return m_fail(SPD_E_ARG, std::string(who) + ": on must be 0 or 1");
    if (on) {
        std::vector<int32_t> control(static_cast<size_t>(m->M), -1);
        for (const BreedPair &pr : br.host_pairs) control[pr.member] = pr.control;
        if (breed_family_limit(breed_families(control.data(), m->M)) < 0) return SPD_E_ARG;
    }
    M_HIP(hipSetDevice(m->ctx->device));
    M_HIP(hipDeviceSynchronize());  // (steps in flight may still use the allocation)
    ortho_release(br);
    if (!on) return SPD_OK;
    if (int rc = ortho_build(m, who)) return rc;
    br.ortho.on = true;
    return SPD_OK;
}

int spd_model_breed_gram(spd_model_handle m, void *dst_device, size_t dst_bytes, void *stream) {
    const char *who = "spd_model_breed_gram";
    if (!m) return m_fail(SPD_E_ARG, std::string(who) + ": null model");
    if (int rc = usable(m, who)) return rc;
    spd_model::Breed &br = m->breed;
    if (!br.on) return m_fail(SPD_E_ARG, std::string(who) + ": " + kBreedOff);
    if (!m->initialized) return m_fail(SPD_E_ARG, std::string(who) + ": model state not initialized");
    if (m->steps_pending) return m_fail(SPD_E_ARG, std::string(who) + ": a checked multi-step call is in flight; end it first");
    const size_t need = static_cast<size_t>(m->M) * m->M * sizeof(double);
    if (int rc = destination_fits(who, dst_device, dst_bytes, need, sizeof(double))) return rc;
    M_HIP(hipSetDevice(m->ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const bool lent = !br.ortho.alloc;  // plain breeding: the lists and the partials for this call only
    if (lent) {
        M_HIP(hipDeviceSynchronize());
        if (int rc = ortho_build(m, who)) return rc;
    }
    const spd_model::Breed::Ortho &o = br.ortho;
    hipError_t e = run_breed_gram(br.planes, o.fams, o.families, o.largest, o.members, m->ctx->dev.elm2, o.partial, s);
    if (e == hipSuccess) e = run_breed_gram_expand(br.planes, o.fams, o.place, m->M, o.partial, static_cast<double *>(dst_device), s);
    if (lent) {
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        ortho_release(br);
    }
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return m_fail(SPD_E_DEVICE, std::string(who) + ": " + hipGetErrorString(e));
    }
    return SPD_OK;
}

int spd_model_breed_ortho_info(spd_model_handle m, int *on, int *families, int *largest) {
    if (!m) return m_fail(SPD_E_ARG, "spd_model_breed_ortho_info: null model");
    const spd_model::Breed &br = m->breed;  // (a model without breeding: all zero)
    std::map<int, int> size;
    int most = 0;
    for (const BreedPair &pr : br.host_pairs) most = std::max(most, ++size[pr.control]);
    if (on) *on = br.ortho.on ? 1 : 0;
    if (families) *families = static_cast<int>(size.size());
    if (largest) *largest = most;
    return SPD_OK;
}

int spd_model_breed_read(spd_model_handle m, int what, int t0, int nt, void *dst_device, size_t dst_bytes, void *stream) {
    const char *who = "spd_model_breed_read";
    if (what != 0 && what != 1) return m_fail(SPD_E_ARG, std::string(who) + ": what is 0 (amplitude) or 1 (factor)");
    if (!m) return m_fail(SPD_E_ARG, std::string(who) + ": null model");
    if (int rc = usable(m, who)) return rc;
    const spd_model::Breed &br = m->breed;
    if (!br.on) return m_fail(SPD_E_ARG, std::string(who) + ": " + kBreedOff);
    if (m->steps_pending) return m_fail(SPD_E_ARG, std::string(who) + ": a checked multi-step call is in flight; end it first");
    if (int rc = held_range(who, br.ring, t0, nt, "event")) return rc;
    const size_t M = static_cast<size_t>(m->M), need = static_cast<size_t>(nt) * M * sizeof(double);
    if (int rc = destination_fits(who, dst_device, dst_bytes, need, sizeof(double))) return rc;
    if (nt == 0) return SPD_OK;
    M_HIP(hipSetDevice(m->ctx->device));
    // (the spectra's gather with one "member" whose entry is the M values of a slot: dst[t][i] = ring[slot(t)][what][i])
    const hipError_t e = run_spectra_gather(br.data + static_cast<size_t>(what) * M, static_cast<double *>(dst_device), m->M, static_cast<long>(2 * M), 1, nt,
                                            br.ring.slot_of_held(t0), br.ring.capacity, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) return m_fail(SPD_E_DEVICE, std::string(who) + ": " + hipGetErrorString(e));
    return SPD_OK;
}

int spd_model_breed_rows(spd_model_handle m, int32_t *rows, int max_rows) {
    return ring_rows(m, "spd_model_breed_rows", &spd_model::breed, kBreedOff, rows, max_rows);
}

int spd_model_breed_reset(spd_model_handle m) {
    if (!m) return m_fail(SPD_E_ARG, "spd_model_breed_reset: null model");
    if (!m->breed.on) return m_fail(SPD_E_ARG, std::string("spd_model_breed_reset: ") + kBreedOff);
    if (m->steps_pending) return m_fail(SPD_E_ARG, "spd_model_breed_reset: a checked multi-step call is in flight; end it first");
    m->breed.ring.clear();
    return SPD_OK;
}

int spd_model_breed_info(spd_model_handle m, int *bred, int *every, int *capacity, long long *taken, int *in_loop, long long *applied) {
    if (!m) return m_fail(SPD_E_ARG, "spd_model_breed_info: null model");
    const spd_model::Breed &br = m->breed;  // (a model without breeding: all zero)
    if (bred) *bred = br.nbred;
    if (every) *every = br.every;
    if (capacity) *capacity = br.ring.capacity;
    if (taken) *taken = br.ring.taken;
    if (in_loop) *in_loop = br.in_loop ? 1 : 0;
    if (applied) *applied = br.applied;
    return SPD_OK;
}

}  // extern "C"
