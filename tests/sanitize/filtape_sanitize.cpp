// AddressSanitizer / UndefinedBehaviorSanitizer driver for the host compile of the filter tape's routines
// (pyspeedy_amd/csrc/filter_point.hpp: fil_section_finite, fil_section_stable, fil_section, fil_first, fil_next and
// fil_series_host, the body of spd_filtape_filter_host).  Coefficients, series and results are heap blocks of exactly the size the
// interface states, so a read or write beyond them -- a section past the cascade's last, say -- is caught; the results are compared
// with a restatement of the definition written here as one loop with the state in plain arrays, not with the routines under test.
// Compiled by tests/test_filtape_sanitize.py with g++ -fsanitize=address,undefined -ffp-contract=off.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "filter_point.hpp"

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

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

// a stable section with poles of radius r at angle th and zeros at z0, z1
static void make_section(double *c, double r, double th, double z0, double z1, double scale) {
    c[0] = scale;
    c[1] = -scale * (z0 + z1);
    c[2] = scale * z0 * z1;
    c[3] = -2.0 * r * std::cos(th);
    c[4] = r * r;
}

// the definition, restated: volatile keeps every intermediate a rounded double of its own
static std::vector<double> restated(const std::vector<double> &c, int n_sections, const std::vector<double> &x) {
    std::vector<double> y(x.size()), s1(n_sections, 0.0), s2(n_sections, 0.0);
    for (size_t i = 0; i < x.size(); ++i) {
        volatile double v = x[i];
        for (int s = 0; s < n_sections; ++s) {
            const double b0 = c[5 * s], b1 = c[5 * s + 1], b2 = c[5 * s + 2], a1 = c[5 * s + 3], a2 = c[5 * s + 4];
            volatile double out, n1, n2;
            if (i == 0) {
                volatile double num = b0 + b1, den = 1.0 + a1;
                num = num + b2;
                den = den + a2;
                volatile double g = num / den;
                out = g * v;
                volatile double t = b0 * v;
                n1 = out - t;
            } else {
                volatile double t = b0 * v;
                out = t + s1[s];
                volatile double p = b1 * v, q = a1 * out;
                volatile double d = p - q;
                n1 = d + s2[s];
            }
            volatile double p2 = b2 * v, q2 = a2 * out;
            n2 = p2 - q2;
            s1[s] = n1;
            s2[s] = n2;
            v = out;
        }
        y[i] = v;
    }
    return y;
}

static bool run_case(int n_sections, int kind, int n, unsigned seed) {
    std::vector<double> c(5 * static_cast<size_t>(n_sections));
    for (int s = 0; s < n_sections; ++s) {
        const double r = 0.55 + 0.1 * s, th = 0.4 + 0.3 * s;
        if (kind == 0) make_section(&c[5 * s], r, th, -1.0, -1.0, 0.05 + 0.01 * s);     // low-pass: zeros at -1
        else if (kind == 1) make_section(&c[5 * s], r, th, 1.0, 1.0, 0.6 - 0.05 * s);   // high-pass: zeros at +1
        else make_section(&c[5 * s], r, th, 1.0, -1.0, 0.2 + 0.02 * s);                 // band-pass: zeros at +1 and -1
    }
    std::vector<FilSection> cascade;
    for (int s = 0; s < n_sections; ++s) {
        REQUIRE(fil_section_finite(&c[5 * s]) && fil_section_stable(&c[5 * s]), "section %d of kind %d", s, kind);
        cascade.push_back(fil_section(&c[5 * s]));
    }
    std::vector<double> x(static_cast<size_t>(n)), y(static_cast<size_t>(n), -1.0);
    unsigned state = seed;
    for (int i = 0; i < n; ++i) {
        state = state * 1664525u + 1013904223u;
        x[i] = 5500.0 + 50.0 * (static_cast<double>(state >> 8) / 8388608.0 - 1.0);
    }
    fil_series_host(cascade.data(), n_sections, x.data(), n, y.data());
    const std::vector<double> ref = restated(c, n_sections, x);
    for (int i = 0; i < n; ++i) REQUIRE(same_bits(y[i], ref[i]), "sections %d kind %d sample %d: %.17g against %.17g", n_sections, kind, i, y[i], ref[i]);
    // a constant through a band-pass is exactly zero from the first sample on
    if (kind == 2) {
        std::vector<double> k(static_cast<size_t>(n), 5500.0), z(static_cast<size_t>(n), -1.0);
        fil_series_host(cascade.data(), n_sections, k.data(), n, z.data());
        for (int i = 0; i < n; ++i) REQUIRE(z[i] == 0.0, "band-pass of a constant, sample %d: %.17g", i, z[i]);
    }
    return true;
}

static bool refusals() {
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    double ok[5] = {0.2, 0.4, 0.2, -0.5, 0.3};
    REQUIRE(fil_section_finite(ok) && fil_section_stable(ok), "a stable section");
    for (int k = 0; k < 5; ++k) {
        double c[5];
        std::memcpy(c, ok, sizeof c);
        c[k] = nan;
        REQUIRE(!fil_section_finite(c), "NaN at %d", k);
        c[k] = k % 2 ? inf : -inf;
        REQUIRE(!fil_section_finite(c), "infinity at %d", k);
    }
    const double unstable[][2] = {{0.0, 1.0}, {0.0, -1.0}, {1.5, 0.5}, {-1.5, 0.5}, {2.0, 1.0}, {0.0, 1.5}};
    for (const auto &a : unstable) {
        double c[5] = {1.0, 0.0, 0.0, a[0], a[1]};
        REQUIRE(!fil_section_stable(c), "a1 %g a2 %g", a[0], a[1]);
    }
    const double edge[][2] = {{1.49, 0.5}, {-1.49, 0.5}, {0.0, 0.99}, {0.0, -0.99}, {0.0, 0.0}};
    for (const auto &a : edge) {
        double c[5] = {1.0, 0.0, 0.0, a[0], a[1]};
        REQUIRE(fil_section_stable(c), "a1 %g a2 %g", a[0], a[1]);
    }
    return true;
}

int main() {
    bool ok = refusals();
    for (int n_sections = 1; ok && n_sections <= kFilMaxSections; ++n_sections)
        for (int kind = 0; ok && kind < 3; ++kind) ok = run_case(n_sections, kind, 40, 17u * n_sections + kind) && run_case(n_sections, kind, 1, 5u) &&
                                                        run_case(n_sections, kind, 0, 5u);
    if (!ok) return 1;
    std::printf("filtape sanitize ok (%ld checks)\n", checks);
    return 0;
}
