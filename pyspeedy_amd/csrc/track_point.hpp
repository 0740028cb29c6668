// The extreme of one plane over a region and where it lies: the rule of the track tape for one (member, entry) and one sample
// (tracktape_kernel of tracktape.hip and spd_track_point_host run these routines).  The header is compiled for
// the device, for the host side of the library and, with no HIP header at all, by the sanitizer program of tests/sanitize/.
//
// A plane is x[p], p = 96 j + i, row j = 0 southernmost; a region is one byte per point, non-zero inside.
//   1. Candidates: the points of the region whose value is not NaN; when radius > 0 and the entry follows a point q >= 0 (`prev`),
//      only those with |j - j_q| <= radius and a circular distance of i and i_q <= radius (rows end at 0 and 47, columns wrap).
//   2. Winner: the smallest (op 0) or largest (op 1) candidate, infinities as numbers; among equal values the smallest p.  Without
//      a candidate: value NaN, index -1, offsets 0.
//   3. Offsets from the winner's four neighbours in the plane, candidates or not: with a = x[j][(i + 95) % 96], b = x[p],
//      c = x[j][(i + 1) % 96]:  den = (a - 2 b) + c,  num = 0.5 (a - c),  di = num / den where den is finite and not zero and the
//      quotient is finite, else 0, then clamped to [-0.5, 0.5]; dj likewise from rows j - 1 and j + 1, 0 on rows 0 and 47.  Every
//      operation is rounded on its own.
// The order (value, p) is total on the candidates, so any reduction tree gives the same winner: a lane that scans its points in
// ascending p and keeps a strictly better value (track_take), and a merge of two lanes' results that breaks ties by p (track_merge).
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SPD_TRACK_HD __host__ __device__
#else
#define SPD_TRACK_HD
#endif

namespace spd {

constexpr int kTrackIX = 96, kTrackIL = 48, kTrackPoints = kTrackIX * kTrackIL;  // a plane
constexpr int kTrackLanes = 256, kTrackPer = kTrackPoints / kTrackLanes;          // lanes of a workgroup; points of a lane
constexpr int kTrackMin = 0, kTrackMaxOp = 1;                                     // the ops of the C ABI (SPD_TRACK_*)
constexpr int kTrackMaxRadius = 24, kTrackMaxRegions = 64, kTrackMaxEntries = 1024;
static_assert(2 * kTrackMaxRadius + 1 <= kTrackIX, "a window does not meet itself round the globe");

namespace track_ops {
// one rounding each: the intrinsics on the device, plain IEEE operations that nothing can contract on the host
SPD_TRACK_HD inline double mul(double a, double b) {
#pragma clang fp contract(off)
#if defined(__HIP_DEVICE_COMPILE__)
    return __dmul_rn(a, b);
#else
    return a * b;
#endif
}
SPD_TRACK_HD inline double add(double a, double b) {
#pragma clang fp contract(off)
#if defined(__HIP_DEVICE_COMPILE__)
    return __dadd_rn(a, b);
#else
    return a + b;
#endif
}
SPD_TRACK_HD inline double sub(double a, double b) {
#pragma clang fp contract(off)
#if defined(__HIP_DEVICE_COMPILE__)
    return __dsub_rn(a, b);
#else
    return a - b;
#endif
}
SPD_TRACK_HD inline double div(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __ddiv_rn(a, b);
#else
    return a / b;
#endif
}
SPD_TRACK_HD inline bool finite(double a) { return __builtin_fabs(a) < __builtin_inf(); }  // (false for NaN)
}  // namespace track_ops

// The best candidate so far: p < 0 while there is none (v then means nothing).
struct TrackBest {
    double v;
    int p;
};

// v is strictly better than b under op; neither is NaN
SPD_TRACK_HD inline bool track_beats(double v, double b, int op) { return op == kTrackMaxOp ? v > b : v < b; }

// step 1 for the point p with value v and region byte `inside`
SPD_TRACK_HD inline bool track_candidate(double v, unsigned char inside, int p, int prev, int radius) {
    if (inside == 0 || v != v) return false;
    if (radius <= 0 || prev < 0) return true;
    int dj = p / kTrackIX - prev / kTrackIX, di = p % kTrackIX - prev % kTrackIX;
    if (dj < 0) dj = -dj;
    if (di < 0) di = -di;
    if (di > kTrackIX - di) di = kTrackIX - di;
    return dj <= radius && di <= radius;
}

// a lane's scan, in ascending p: only a strictly better value replaces what the lane holds, so its lowest p wins a tie
SPD_TRACK_HD inline void track_take(TrackBest &best, double v, int p, int op) {
    if (best.p < 0 || track_beats(v, best.v, op)) {
        best.v = v;
        best.p = p;
    }
}

// the better of two results by (value, p)
SPD_TRACK_HD inline TrackBest track_merge(TrackBest a, TrackBest b, int op) {
    if (b.p < 0) return a;
    if (a.p < 0) return b;
    if (track_beats(b.v, a.v, op)) return b;
    if (track_beats(a.v, b.v, op)) return a;
    return b.p < a.p ? b : a;
}

// step 3 along one direction: a and c are the neighbours of b
SPD_TRACK_HD inline double track_offset(double a, double b, double c) {
    using namespace track_ops;
    const double den = add(sub(a, mul(2.0, b)), c);
    const double num = mul(0.5, sub(a, c));
    if (!finite(den) || den == 0.0) return 0.0;
    const double q = div(num, den);
    if (!finite(q)) return 0.0;
    return q < -0.5 ? -0.5 : q > 0.5 ? 0.5 : q;
}

// what a sample leaves for one (member, entry): the ring's four doubles
struct TrackResult {
    double value, p, di, dj;
};

// steps 2 (what is stored) and 3 for the winner.  plane: the 4608 values (the kernel's copy in the LDS).
SPD_TRACK_HD inline TrackResult track_finish(const double *plane, TrackBest best) {
    if (best.p < 0) return TrackResult{__builtin_nan(""), -1.0, 0.0, 0.0};
    const int j = best.p / kTrackIX, i = best.p % kTrackIX;
    const double *row = plane + j * kTrackIX;
    const double b = row[i];
    const double di = track_offset(row[(i + kTrackIX - 1) % kTrackIX], b, row[(i + 1) % kTrackIX]);
    const double dj = (j == 0 || j == kTrackIL - 1) ? 0.0 : track_offset(row[i - kTrackIX], b, row[i + kTrackIX]);
    return TrackResult{b, static_cast<double>(best.p), di, dj};
}

// The whole rule for one plane as the kernel's workgroup runs it, lane after lane: 256 scans of 18 points at p = t + 256 r, then
// the halving tree over the lanes' results (the body of spd_track_point_host).  mask: [4608] bytes; prev: -1 or 0 ... 4607.
inline void track_point_host(const double *plane, const unsigned char *mask, int prev, int radius, int op, double *out4) {
    TrackBest lane[kTrackLanes];
    for (int t = 0; t < kTrackLanes; ++t) {
        lane[t] = TrackBest{0.0, -1};
        for (int r = 0; r < kTrackPer; ++r) {
            const int p = t + kTrackLanes * r;
            if (track_candidate(plane[p], mask[p], p, prev, radius)) track_take(lane[t], plane[p], p, op);
        }
    }
    for (int half = kTrackLanes / 2; half > 0; half >>= 1)
        for (int t = 0; t < half; ++t) lane[t] = track_merge(lane[t], lane[t + half], op);
    const TrackResult got = track_finish(plane, lane[0]);
    out4[0] = got.value;
    out4[1] = got.p;
    out4[2] = got.di;
    out4[3] = got.dj;
}

}  // namespace spd
