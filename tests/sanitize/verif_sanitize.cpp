// AddressSanitizer / UndefinedBehaviorSanitizer driver for the host compile of the verification tape's routines
// (pyspeedy_amd/csrc/verif_point.hpp: verif_point, verif_fold_host and verif_entry_host, the body of spd_verif_host).  Every array
// is a heap block of exactly the size the interface states, so a read or write beyond it is caught; the results are compared with
// a restatement of the definition written here -- a loop per accumulator, the tree folded out of place -- not with the routines
// under test.  Compiled by tests/test_verif_sanitize.py with g++ -fsanitize=address,undefined -ffp-contract=off.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "verif_point.hpp"

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

static bool entry_case(int r, bool with_ties) {
    const int N = kVerifPoints;
    std::vector<double> x(static_cast<size_t>(r) * N), y(N), w(N), out(4), scratch(4 * kVerifLanes);
    std::vector<int> hist(kVerifCounts, -7);
    for (double &v : x) v = value();
    for (int p = 0; p < N; ++p) {
        y[p] = value();
        w[p] = p % 5 == 3 ? 0.0 : value();
        if (with_ties && p % 7 == 0) x[static_cast<size_t>(p % r) * N + p] = y[p];
    }
    verif_entry_host(x.data(), r, y.data(), w.data(), out.data(), hist.data(), scratch.data());
    // the definition again
    std::vector<double> term(4 * static_cast<size_t>(N));
    std::vector<int> want(kVerifCounts, 0);
    int weighted = 0;
    for (int p = 0; p < N; ++p) {
        std::vector<double> v(r);
        for (int j = 0; j < r; ++j) v[j] = x[static_cast<size_t>(j) * N + p];
        double s = v[0];
        for (int j = 1; j < r; ++j) s = s + v[j];
        const double mean = s / r, e = mean - y[p];
        double a = (v[0] - mean) * (v[0] - mean);
        for (int j = 1; j < r; ++j) {
            const double d = v[j] - mean;
            a = a + d * d;
        }
        double b = std::fabs(v[0] - y[p]);
        for (int j = 1; j < r; ++j) b = b + std::fabs(v[j] - y[p]);
        double c = 0.0;
        for (int j = 0; j < r - 1; ++j)
            for (int k = j + 1; k < r; ++k) c = c + std::fabs(v[j] - v[k]);
        const double rr = r;
        const double score[4] = {e, e * e, a / (r - 1), b / rr - c / (rr * rr)};
        for (int k = 0; k < 4; ++k) term[static_cast<size_t>(k) * N + p] = w[p] * score[k];
        int rank = 0;
        bool tie = false;
        for (int j = 0; j < r; ++j) rank += v[j] < y[p], tie = tie || v[j] == y[p];
        if (w[p] != 0.0) ++want[tie ? r + 1 : rank], ++weighted;
    }
    for (int k = 0; k < 4; ++k) {
        std::vector<double> tree(kVerifLanes);
        for (int t = 0; t < kVerifLanes; ++t) {
            double s = term[static_cast<size_t>(k) * N + t];
            for (int i = 1; i < kVerifPasses; ++i) s = s + term[static_cast<size_t>(k) * N + t + kVerifLanes * i];
            tree[t] = s;
        }
        for (int half = kVerifLanes / 2; half > 0; half /= 2) {
            std::vector<double> next(half);
            for (int t = 0; t < half; ++t) next[t] = tree[t] + tree[t + half];
            tree = next;
        }
        REQUIRE(same_bits(out[k], tree[0]) && std::isfinite(out[k]), "r %d score %d: %.17g, restated %.17g", r, k, out[k], tree[0]);
    }
    int total = 0;
    for (int k = 0; k < kVerifCounts; ++k) {
        REQUIRE(hist[k] == want[k], "r %d count %d: %d, restated %d", r, k, hist[k], want[k]);
        total += hist[k];
    }
    REQUIRE(total == weighted, "r %d: %d points counted, %d have a weight", r, total, weighted);
    REQUIRE((hist[r + 1] > 0) == with_ties, "r %d: %d ties", r, hist[r + 1]);
    return true;
}

int main() {
    for (int r : {2, 64})
        for (bool ties : {false, true})
            if (!entry_case(r, ties)) return 1;
    std::printf("verif sanitize ok %ld checks\n", checks);
    return 0;
}
