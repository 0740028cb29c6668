// Assimilation: the member-mixing matrix W of a serial ensemble square-root filter (spd_assim_weights_host and
// assim_weights_kernel of assim.hip run this one routine).
//
// Y[e][i] is the value of entry e for member i (r members, E entries), yo[e] the observation (NaN: missing), R[e] its error
// variance, rho the inflation.  Every operation is rounded on its own and every sum is sequential in ascending index, starting
// from its first term (the definition: include/pyspeedy_amd.h):
//   a = (1 - rho) / r;  W[i][j] = a for i != j,  W[i][i] = a + rho
//   for e = 0 ... E - 1:
//     y_j = sum_i Y[e][i] W[i][j];  ybar = (sum_j y_j) / r;  d_j = y_j - ybar;  s = (sum_j d_j d_j) / (r - 1)
//     unused (W as it is) if yo[e] is NaN or s is not a finite number > 0; otherwise
//     t = s + R[e];  alpha = 1 / (1 + sqrt(R[e] / t));  v = yo[e] - ybar;  q = (r - 1) t;  g_i = d_i / q;  c_j = v - alpha d_j
//     u_k = sum_i W[k][i] g_i;  W[k][j] = W[k][j] + u_k c_j
// The work is spread over `lanes` lanes: y_j and c_j with a lane per column, u_k with a lane per row, the rank-one update over all
// entries; every lane forms ybar, s and the decision for itself, so the decision is the same in all of them.  The host runs it with
// one lane.
#pragma once
#include <hip/hip_runtime.h>

#include "breed_factor.hpp"

namespace spd {

constexpr int kAssimMax = 64;  // members of an analysis, and entries (scalar observations) of one

// W: [r][ld] (ld >= r; rows and columns below r are written).  Y: [E][ldy].  vec: 4 * kAssimMax doubles of scratch that all lanes
// share (y, g, c, u).  stats: [E][4] = ybar, s, v, used (1.0 / 0.0); v is stored as 0.0 for a missing observation.  `barrier`
// stands between what one lane writes and another reads.
template <class Barrier>
__host__ __device__ inline void assim_weights(const double *Y, int ldy, int E, int r, const double *yo, const double *R, double rho, double *W,
                                              int ld, double *vec, double *stats, int lane, int lanes, Barrier barrier) {
    using namespace breed_ops;
    double *y = vec, *g = vec + kAssimMax, *c = vec + 2 * kAssimMax, *u = vec + 3 * kAssimMax;
    const double rr = static_cast<double>(r), rm1 = static_cast<double>(r - 1);
    const double a = div(sub(1.0, rho), rr), diag = add(a, rho);
    for (int x = lane; x < r * r; x += lanes) {
        const int i = x / r, j = x - i * r;
        W[i * ld + j] = i == j ? diag : a;
    }
    barrier();
    for (int e = 0; e < E; ++e) {
        const double *row = Y + static_cast<long>(e) * ldy;
        for (int j = lane; j < r; j += lanes) {
            double acc = mul(row[0], W[j]);
#pragma unroll 8
            for (int i = 1; i < r; ++i) acc = add(acc, mul(row[i], W[i * ld + j]));
            y[j] = acc;
        }
        barrier();
        double sum = y[0];
#pragma unroll 8
        for (int j = 1; j < r; ++j) sum = add(sum, y[j]);
        const double ybar = div(sum, rr);
        const double d0 = sub(y[0], ybar);
        double ss = mul(d0, d0);
#pragma unroll 8
        for (int j = 1; j < r; ++j) {
            const double dj = sub(y[j], ybar);
            ss = add(ss, mul(dj, dj));
        }
        const double s = div(ss, rm1), obs = yo[e];
        const bool missing = obs != obs;
        const bool used = !missing && s > 0.0 && s < __builtin_inf();
        const double v = missing ? 0.0 : sub(obs, ybar);
        if (lane == 0) {
            stats[4 * e] = ybar;
            stats[4 * e + 1] = s;
            stats[4 * e + 2] = v;
            stats[4 * e + 3] = used ? 1.0 : 0.0;
        }
        if (!used) {
            barrier();  // (every lane has read y before the next entry overwrites it)
            continue;
        }
        const double t = add(s, R[e]);
        const double alpha = div(1.0, add(1.0, root(div(R[e], t))));
        const double q = mul(rm1, t);
        for (int j = lane; j < r; j += lanes) {
            const double dj = sub(y[j], ybar);
            g[j] = div(dj, q);
            c[j] = sub(v, mul(alpha, dj));
        }
        barrier();
        for (int k = lane; k < r; k += lanes) {
            double acc = mul(W[k * ld], g[0]);
#pragma unroll 8
            for (int i = 1; i < r; ++i) acc = add(acc, mul(W[k * ld + i], g[i]));
            u[k] = acc;
        }
        barrier();
        for (int x = lane; x < r * r; x += lanes) {
            const int k = x / r, j = x - k * r;
            W[k * ld + j] = add(W[k * ld + j], mul(u[k], c[j]));
        }
        barrier();
    }
}

}  // namespace spd
