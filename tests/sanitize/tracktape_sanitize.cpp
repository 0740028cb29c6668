// AddressSanitizer / UndefinedBehaviorSanitizer driver for the host compile of the track tape's routines
// (pyspeedy_amd/csrc/track_point.hpp: track_candidate, track_take, track_merge, track_offset, track_finish and track_point_host,
// the body of spd_track_point_host).  Plane, mask and result are heap blocks of exactly the size the interface states, so a read or
// write beyond them -- a neighbour of a winner on the rim of the grid, say -- is caught; the results are compared with a
// restatement of the definition written here, one ascending scan with the tie rule spelled out, not with the routines under test.
// The planes are those of tests/test_tracktape_cpu.py: the same base plane and the same points set into it.  Compiled by
// tests/test_tracktape_sanitize.py with g++ -fsanitize=address,undefined -ffp-contract=off.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "track_point.hpp"

using namespace spd;

static long checks = 0;
#define REQUIRE(cond, ...)                                             \
    do {                                                               \
        ++checks;                                                      \
        if (!(cond)) {                                                 \
            std::printf("FAILED %s:%d  %s\n  ", __FILE__, __LINE__, #cond); \
            std::printf(__VA_ARGS__);                                  \
            std::printf("\n");                                         \
            return false;                                              \
        }                                                              \
    } while (0)

constexpr int IX = kTrackIX, IL = kTrackIL, N = kTrackPoints;
static const double kNaN = std::numeric_limits<double>::quiet_NaN(), kInf = std::numeric_limits<double>::infinity();

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

struct Point {
    int j, i;
    double v;
};

// 100 + a permutation of 0 ... 4607 eighths
static std::vector<double> base_plane() {
    std::vector<double> x(N);
    for (int p = 0; p < N; ++p) x[p] = 100.0 + static_cast<double>((static_cast<long>(p) * 7919) % N) * 0.125;
    return x;
}
static std::vector<double> constant_plane(double v) { return std::vector<double>(N, v); }
static std::vector<double> with_points(std::vector<double> x, const std::vector<Point> &points) {
    for (const Point &q : points) x[IX * q.j + q.i] = q.v;
    return x;
}
// rows j0 ... j1 and columns i0 ... i1, both ends included; i0 > i1 wraps
static std::vector<unsigned char> box_mask(int j0, int j1, int i0, int i1) {
    std::vector<unsigned char> m(N, 0);
    for (int j = j0; j <= j1; ++j)
        for (int i = 0; i < IX; ++i)
            if (i0 <= i1 ? (i >= i0 && i <= i1) : (i >= i0 || i <= i1)) m[IX * j + i] = 1;
    return m;
}

// the definition again
static double offset_again(double a, double b, double c) {
    const double den = (a - 2.0 * b) + c, num = 0.5 * (a - c);
    if (!std::isfinite(den) || den == 0.0) return 0.0;
    const double q = num / den;
    if (!std::isfinite(q)) return 0.0;
    return q < -0.5 ? -0.5 : q > 0.5 ? 0.5 : q;
}
static void track_again(const double *x, const unsigned char *mask, int prev, int radius, int op, double *out4) {
    int at = -1;
    for (int p = 0; p < N; ++p) {
        if (!mask[p] || std::isnan(x[p])) continue;
        if (radius > 0 && prev >= 0) {
            const int dj = std::abs(p / IX - prev / IX);
            int di = std::abs(p % IX - prev % IX);
            if (IX - di < di) di = IX - di;
            if (dj > radius || di > radius) continue;
        }
        if (at < 0 || (op == kTrackMaxOp ? x[p] > x[at] : x[p] < x[at])) at = p;
    }
    out4[0] = kNaN, out4[1] = -1.0, out4[2] = out4[3] = 0.0;
    if (at < 0) return;
    const int j = at / IX, i = at % IX;
    out4[0] = x[at];
    out4[1] = at;
    out4[2] = offset_again(x[IX * j + (i + IX - 1) % IX], x[at], x[IX * j + (i + 1) % IX]);
    if (j > 0 && j < IL - 1) out4[3] = offset_again(x[at - IX], x[at], x[at + IX]);
}

// want_p: the winner the case was built for, or -2 for "whatever the restatement finds"
static bool run_case(const char *name, const std::vector<double> &plane, const std::vector<unsigned char> &mask, int prev, int radius, int op,
                     int want_p) {
    // heap blocks of exactly the stated sizes
    double *x = new double[N];
    unsigned char *m = new unsigned char[N];
    double *got = new double[4];
    std::memcpy(x, plane.data(), N * sizeof(double));
    std::memcpy(m, mask.data(), N);
    for (int k = 0; k < 4; ++k) got[k] = -7.0;
    double want[4];
    track_point_host(x, m, prev, radius, op, got);
    track_again(x, m, prev, radius, op, want);
    bool ok = true;
    for (int k = 0; k < 4 && ok; ++k) ok = same_bits(got[k], want[k]);
    const double g0 = got[0], g1 = got[1], g2 = got[2], g3 = got[3];
    delete[] x;
    delete[] m;
    delete[] got;
    REQUIRE(ok, "%s: %.17g %.17g %.17g %.17g, restated %.17g %.17g %.17g %.17g", name, g0, g1, g2, g3, want[0], want[1], want[2], want[3]);
    REQUIRE(want_p == -2 || static_cast<int>(g1) == want_p, "%s: winner %d, built for %d", name, static_cast<int>(g1), want_p);
    REQUIRE(g2 >= -0.5 && g2 <= 0.5 && g3 >= -0.5 && g3 <= 0.5, "%s: offsets %.17g %.17g", name, g2, g3);
    return true;
}

static int at(int j, int i) { return IX * j + i; }

int main() {
    const std::vector<unsigned char> all(N, 1);
    const std::vector<double> base = base_plane();
    std::vector<Point> nan_box;
    for (int j = 10; j < 13; ++j)
        for (int i = 30; i < 33; ++i) nan_box.push_back({j, i, kNaN});
    bool ok = true;
    ok = ok && run_case("constant", constant_plane(5.0), box_mask(10, 20, 30, 40), -1, 0, kTrackMin, at(10, 30));
    ok = ok && run_case("constant max", constant_plane(5.0), box_mask(10, 20, 90, 3), -1, 0, kTrackMaxOp, at(10, 0));
    ok = ok && run_case("column 0", with_points(base, {{20, 0, 0.0}, {20, 95, 200.0}, {20, 1, 100.0}, {19, 0, 50.0}, {21, 0, 50.0}}), all, -1, 0,
                        kTrackMin, at(20, 0));
    ok = ok && run_case("column 95", with_points(base, {{20, 95, 0.0}, {20, 94, 100.0}, {20, 0, 200.0}, {19, 95, 50.0}, {21, 95, 150.0}}), all, -1,
                        0, kTrackMin, at(20, 95));
    ok = ok && run_case("row 0", with_points(base, {{0, 50, 0.0}, {0, 49, 64.0}, {0, 51, 32.0}}), all, -1, 0, kTrackMin, at(0, 50));
    ok = ok && run_case("row 47", with_points(base, {{47, 50, 5000.0}, {47, 49, 4000.0}, {47, 51, 4500.0}}), all, -1, 0, kTrackMaxOp, at(47, 50));
    ok = ok && run_case("corner 0", with_points(base, {{0, 0, -5.0}}), all, -1, 0, kTrackMin, at(0, 0));
    ok = ok && run_case("corner 4607", with_points(base, {{47, 95, 5000.0}}), all, -1, 0, kTrackMaxOp, at(47, 95));
    ok = ok && run_case("clamp", with_points(base, {{20, 10, 0.0}, {20, 9, -10.0}, {20, 11, 200.0}, {19, 10, 300.0}, {21, 10, -20.0}}),
                        box_mask(20, 20, 10, 12), -1, 0, kTrackMin, at(20, 10));
    ok = ok && run_case("nan in the region", with_points(base, {{12, 33, kNaN}, {12, 34, 1.0}, {13, 34, 3.0}, {11, 34, 4.0}, {12, 35, 2.0}}),
                        box_mask(10, 20, 30, 40), -1, 0, kTrackMin, at(12, 34));
    ok = ok && run_case("nan in the region, max", with_points(base, {{12, 33, kNaN}}), box_mask(10, 20, 30, 40), -1, 0, kTrackMaxOp, -2);
    ok = ok && run_case("all nan", with_points(base, nan_box), box_mask(10, 12, 30, 32), -1, 0, kTrackMin, -1);
    ok = ok && run_case("all nan, followed", with_points(base, nan_box), box_mask(10, 12, 30, 32), at(11, 31), 1, kTrackMaxOp, -1);
    ok = ok && run_case("-inf wins", with_points(base, {{5, 5, -kInf}}), all, -1, 0, kTrackMin, at(5, 5));
    ok = ok && run_case("+inf wins", with_points(base, {{5, 5, kInf}, {40, 7, kInf}}), all, -1, 0, kTrackMaxOp, at(5, 5));
    ok = ok && run_case("+inf loses", with_points(base, {{5, 5, kInf}, {30, 30, 0.0}, {30, 29, kInf}, {29, 30, 1.0}, {31, 30, 2.0}}), all, -1, 0,
                        kTrackMin, at(30, 30));
    ok = ok && run_case("zeros", with_points(constant_plane(1.0), {{5, 5, 0.0}, {10, 10, -0.0}}), all, -1, 0, kTrackMin, at(5, 5));
    ok = ok && run_case("zeros, minus first", with_points(constant_plane(-1.0), {{5, 5, -0.0}, {10, 10, 0.0}}), all, -1, 0, kTrackMaxOp, at(5, 5));
    ok = ok && run_case("date line", with_points(base, {{20, 50, -1000.0}, {21, 93, -700.0}, {21, 94, -500.0}, {17, 2, -400.0}}), all, at(20, 1), 3,
                        kTrackMin, at(21, 94));
    ok = ok && run_case("pole", with_points(base, {{7, 40, -1000.0}, {0, 38, -500.0}, {6, 45, -400.0}, {1, 46, -900.0}}), all, at(1, 40), 5,
                        kTrackMin, at(0, 38));
    ok = ok && run_case("north pole, max", with_points(base, {{41, 3, 9000.0}, {47, 95, 8000.0}, {42, 90, 7000.0}}), all, at(46, 0), 4, kTrackMaxOp,
                        at(47, 95));
    ok = ok && run_case("radius 24", with_points(base, {{3, 73, -1000.0}, {47, 23, -900.0}, {47, 24, -500.0}, {0, 72, -400.0}}), all, at(24, 48), 24,
                        kTrackMin, at(47, 24));
    ok = ok && run_case("not seeded", with_points(base, {{20, 50, -1000.0}, {21, 94, -500.0}}), all, -1, 3, kTrackMin, at(20, 50));
    ok = ok && run_case("radius 0", with_points(base, {{20, 50, -1000.0}, {21, 94, -500.0}}), all, at(20, 1), 0, kTrackMin, at(20, 50));
    ok = ok && run_case("window and box", base, box_mask(18, 30, 90, 5), at(20, 1), 3, kTrackMaxOp, -2);
    // every seed of a small region at every radius, both ops: the window arithmetic at all four rims of the grid
    const std::vector<unsigned char> rim = box_mask(0, 47, 94, 1);
    for (int radius = 0; radius <= kTrackMaxRadius && ok; radius += 6)
        for (int j : {0, 1, 23, 46, 47})
            for (int i : {94, 95, 0, 1})
                for (int op : {kTrackMin, kTrackMaxOp}) ok = ok && run_case("rim", base, rim, at(j, i), radius, op, -2);
    if (!ok) return 1;
    std::printf("tracktape sanitize ok %ld checks\n", checks);
    return 0;
}
