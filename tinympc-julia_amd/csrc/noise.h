// THE DRAW RULE of the closed loop's process and measurement noise (tinympc_set_process_noise / _set_measurement_noise): a
// counter-based generator, every draw a pure function of (seed, kind, instance, step) — nothing is stored or uploaded, and a
// loop continues its noise stream as it continues its state.  One text for the device kernels (solver.hip) and for the host
// export tinympc_host_noise (capi.hip).
//
// Standard normals xi[which][b][t][i], which 0 process / 1 measurement, b the instance, t >= 0 the step, i < nx:
//   Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; Weyl increments 0x9E3779B9, 0xBB67AE85),
//   key (seed low, seed high), counter (b low, b high, t, (which << 16) | j) with j = i / 2; from its words w0..w3
//   u1 = (((w1:w0) >> 11) + 1) 2^-53 in (0, 1], u2 = ((w3:w2) >> 11) 2^-53 in [0, 1), r = sqrt(-2 ln u1),
//   xi[2j] = r cos(2 pi u2), xi[2j+1] = r sin(2 pi u2), all fp64; an odd nx drops the last sine.
// Noise vector n = G xi, G nx x nx column-major fp64 (any matrix; the covariance is G G'): row r is acc = 0, then
// acc = fma(G[r + i nx], xi[i], acc) for i ascending.
// Every product below is either a single rounding (one multiply, one call) or an explicit fma: there is no a * b + c the
// compiler could contract in one caller and not in another.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TMPC_NOISE_HD __host__ __device__
#else
#define TMPC_NOISE_HD
#endif

namespace tmpc {

enum { NOISE_PROCESS = 0, NOISE_MEASUREMENT = 1 };

TMPC_NOISE_HD inline void philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
    uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = key[0], k1 = key[1];
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0, c1 = n1, c2 = n2, c3 = n3;
        k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
    }
    out[0] = c0, out[1] = c1, out[2] = c2, out[3] = c3;
}

// the pair (xi[2j], xi[2j+1]) of one (seed, which, b, t)
TMPC_NOISE_HD inline void noise_pair(uint64_t seed, int which, uint64_t b, uint32_t t, uint32_t j, double &even, double &odd) {
    const uint32_t ctr[4] = {(uint32_t)b, (uint32_t)(b >> 32), t, ((uint32_t)which << 16) | j};
    const uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
    uint32_t w[4];
    philox4x32_10(ctr, key, w);
    const double two_m53 = 1.0 / 9007199254740992.0;
    const double u1 = (double)(((((uint64_t)w[1] << 32) | w[0]) >> 11) + 1) * two_m53;   // (exact: 53 bits, a power of two)
    const double u2 = (double)((((uint64_t)w[3] << 32) | w[2]) >> 11) * two_m53;
    const double r = sqrt(-2.0 * log(u1)), a = 6.283185307179586476925286766559 * u2;
    even = r * cos(a);
    odd = r * sin(a);
}

// row r of n = G xi
TMPC_NOISE_HD inline double noise_row(const double *G, int nx, int r, const double *xi) {
    double acc = 0.0;
    for (int i = 0; i < nx; ++i) acc = fma(G[r + i * nx], xi[i], acc);
    return acc;
}

}  // namespace tmpc
