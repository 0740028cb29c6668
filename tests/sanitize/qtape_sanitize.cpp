// AddressSanitizer / UndefinedBehaviorSanitizer driver for the host compile of the quantile tape's routines
// (pyspeedy_amd/csrc/qtape_point.hpp: qtape_item, qtape_sort, qtape_value and qtape_plane_host, the body of spd_qtape_host).  Every
// array is a heap block of exactly the size the interface states, so a read or write beyond it is caught; the results are compared
// with a restatement of the definition written here -- std::stable_sort under operator<, the interpolation spelled out -- not with
// the routines under test.  Compiled by tests/test_qtape_sanitize.py with g++ -fsanitize=address,undefined -ffp-contract=off.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "qtape_point.hpp"

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

// a small generator of its own: values of both signs and many scales
static uint64_t state = 0x9E3779B97F4A7C15ull;
static double uniform() {
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return static_cast<double>(state >> 11) / 9007199254740992.0;
}
static double value() { return (uniform() - 0.5) * std::pow(10.0, 6.0 * uniform() - 3.0); }

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

static bool plane_case(int r, bool with_ties) {
    const int N = kQtapePoints;
    const double thr = 0.25;
    const int ops[] = {kQtapeMin, kQtapeMaxOp, kQtapeQuantile, kQtapeQuantile, kQtapeQuantile, kQtapeQuantile, kQtapeQuantile, kQtapeProbAbove,
                       kQtapeProbBelow};
    const double params[] = {0.0, 0.0, 0.0, 0.1, 1.0 / 3.0, 0.5, 1.0, thr, thr};
    const int E = sizeof(ops) / sizeof(ops[0]);
    std::vector<double> x(static_cast<size_t>(r) * N), out(static_cast<size_t>(E) * N, -7.0);
    std::vector<QtapeItem> items(E);
    for (double &v : x) v = value();
    if (with_ties)
        for (int p = 0; p < N; ++p) {
            if (p % 7 == 0) x[static_cast<size_t>(p % r) * N + p] = x[static_cast<size_t>((p + 1) % r) * N + p];
            if (p % 11 == 0) x[static_cast<size_t>(p % 2) * N + p] = -0.0, x[static_cast<size_t>(1 - p % 2) * N + p] = 0.0;
            if (p % 13 == 0) x[static_cast<size_t>((p / 13) % r) * N + p] = thr;
        }
    for (int k = 0; k < E; ++k) {
        items[k] = qtape_item(ops[k], params[k], r);
        items[k].entry = k;
        REQUIRE(items[k].lo >= 0 && items[k].lo <= items[k].hi && items[k].hi < r && items[k].f >= 0.0 && items[k].f < 1.0, "r %d entry %d: lo %d hi %d f %g",
                r, k, items[k].lo, items[k].hi, items[k].f);
    }
    qtape_plane_host(x.data(), r, items.data(), E, out.data());
    // the definition again
    int ties = 0;
    for (int p = 0; p < N; ++p) {
        std::vector<double> s(r);
        for (int j = 0; j < r; ++j) s[j] = x[static_cast<size_t>(j) * N + p];
        int above = 0, below = 0;
        for (int j = 0; j < r; ++j) above += s[j] > thr, below += s[j] < thr;
        std::stable_sort(s.begin(), s.end());  // (operator<: equal values and the two zeros keep the order of their member index)
        for (int j = 0; j + 1 < r; ++j) ties += !(s[j] < s[j + 1]);
        for (int k = 0; k < E; ++k) {
            double want;
            if (ops[k] == kQtapeMin) want = s[0];
            else if (ops[k] == kQtapeMaxOp) want = s[r - 1];
            else if (ops[k] == kQtapeProbAbove) want = static_cast<double>(above) / r;
            else if (ops[k] == kQtapeProbBelow) want = static_cast<double>(below) / r;
            else {
                const double h = params[k] * (r - 1);
                const int lo = static_cast<int>(std::floor(h)), hi = std::min(lo + 1, r - 1);
                const double f = h - lo;
                if (f == 0.0) want = s[lo];
                else {
                    const double d = s[hi] - s[lo];
                    const double t = f * d;
                    want = s[lo] + t;
                    if (want > s[hi]) want = s[hi];
                }
            }
            const double got = out[static_cast<size_t>(k) * N + p];
            REQUIRE(same_bits(got, want) && std::isfinite(got), "r %d entry %d point %d: %.17g, restated %.17g", r, k, p, got, want);
        }
    }
    REQUIRE((ties > 0) == with_ties, "r %d: %d ties", r, ties);
    return true;
}

int main() {
    for (int r : {2, 64})
        for (bool ties : {false, true})
            if (!plane_case(r, ties)) return 1;
    std::printf("qtape sanitize ok %ld checks\n", checks);
    return 0;
}
