/*
 * gle_force.hip -- device-resident anharmonic pair force field (gle_set_pair_force).
 *
 * The field is a static list of atom pairs (harmonic, Morse or Lennard-Jones bonds), the force the
 * sum over exactly those pairs: no cutoff, no list rebuild.  It plays the role of a host driver's
 * force(q) (lammpsdriver.force, lammpsdriver.py:70-84: x = xyz + conv q, f = conv F - f0) without
 * leaving the device: the result lands in Fc, where a host force is uploaded today, and the chain
 * stages run in their host-force variants.
 *
 * Gather form: the pair list is turned into a per-atom CSR neighbour table at set time, every pair
 * stored from both ends in pair-list order.  One thread per (atom, trajectory), trajectory fastest,
 * so the q loads and the Fc / Q0 stores of a wave are contiguous over the trajectories.  No atomics
 * and a fixed neighbour order: a trajectory's force does not depend on the batch width or on its
 * column.  fp64 throughout, one rsqrt per pair (plus one exp for a Morse pair).  The neighbour loop
 * is left rolled: a row has ~2-12 entries, the kernel is latency-bound (natom B threads, a few
 * waves), and the fp64 exp / rsqrt sequences are long enough that unrolling buys register pressure,
 * not overlap; the 64-byte neighbour records are wave-uniform loads when B >= 64.
 *
 * md.potforce's cache rule (sameq, md.py:449-450, 767-779) per trajectory needs max_d |q - Q0| over
 * all DOFs of the trajectory before any of its threads may skip or overwrite Q0: a pre-pass launch
 * (pair_dist_kernel, one workgroup per 64 trajectories and chunk of DOFs, at most 32 chunks) writes
 * one flag per chunk and trajectory with plain stores (set as well when the trajectory's cache is
 * empty), the force launch ORs a trajectory's flags and reads nothing that it writes itself.
 * Q0 is the field's own buffer: the point of the last *evaluation* (the chain's Q0 is rewritten to
 * q~ by the host-force velocity stage whether or not the force was evaluated there).
 */
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gle_internal.h"

namespace gle {

namespace {

// U'(r) / r of one pair from r^2 (the force on atom i is this times d = x_j + shift - x_i)
__device__ __forceinline__ double pair_g(int style, const double* __restrict__ p, double r2) {
  const double rinv = rsqrt(r2);
  const double r = r2 * rinv;
  if (style == PAIR_MORSE) {  // U = D (1 - exp(-a (r - r0)))^2, p = (D, a, r0)
    const double e = exp(-p[1] * (r - p[2]));
    return 2.0 * p[0] * p[1] * e * (1.0 - e) * rinv;
  }
  if (style == PAIR_LJ) {  // U = 4 eps ((sigma / r)^12 - (sigma / r)^6), p = (eps, sigma)
    const double ri2 = rinv * rinv;
    const double s2 = p[1] * p[1] * ri2;
    const double s6 = s2 * s2 * s2;
    return -24.0 * p[0] * (2.0 * s6 * s6 - s6) * ri2;
  }
  return p[0] * (r - p[1]) * rinv;  // U = k / 2 (r - r0)^2, p = (k, r0)
}

// c f - f0 with the product rounded on its own (never fused into the subtraction): f0 is this
// product at q = 0, and the force there must be exactly zero
__device__ __forceinline__ double mul_sub(double c, double f, double f0) {
#pragma clang fp contract(off)
  const double m = c * f;
  return m - f0;
}

__global__ __launch_bounds__(256) void pair_dist_kernel(PairFFArgs a) {
  __shared__ int bad_s[4][64];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int b = blockIdx.x * 64 + tx;
  const int i1 = min(3 * a.natom, ((int)blockIdx.y + 1) * a.chunk);
  // an empty cache (valid = 0) misses in every chunk: the force launch decides from these flags
  // alone and never reads a word it writes (valid, Q0, count)
  int bad = (b < a.B && ty == 0) ? (a.valid[b] == 0) : 0;
  if (b < a.B) {
#pragma unroll 8
    for (int i = (int)blockIdx.y * a.chunk + ty; i < i1; i += 4) {
      const int64_t o = (int64_t)i * a.B + b;
      bad |= !(fabs(a.q[o] - a.Q0[o]) < 10e-10);  // NaN: miss
    }
  }
  bad_s[ty][tx] = bad;
  __syncthreads();
  if (ty == 0 && b < a.B)
    a.bad[(int64_t)blockIdx.y * a.B + b] = bad_s[0][tx] | bad_s[1][tx] | bad_s[2][tx] | bad_s[3][tx];
}

__global__ __launch_bounds__(256) void pair_force_kernel(PairFFArgs a) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= (int64_t)a.natom * a.B) return;
  const int at = (int)(g / a.B), b = (int)(g - (int64_t)at * a.B);
  if (a.cached) {  // md.potforce cache hit (the pre-pass found every chunk valid and within 1e-9 of Q0): Fc stays
    int bad = 0;
    int w[PAIR_MAXCHUNK];  // every flag load in flight at once (one latency, not nchunk of them)
#pragma unroll
    for (int c = 0; c < PAIR_MAXCHUNK; ++c) w[c] = c < a.nchunk ? a.bad[(int64_t)c * a.B + b] : 0;
#pragma unroll
    for (int c = 0; c < PAIR_MAXCHUNK; ++c) bad |= w[c];
    if (!bad) return;
  }
  const int64_t o0 = (int64_t)(3 * at) * a.B + b, o1 = o0 + a.B, o2 = o1 + a.B;
  const double q0 = a.q[o0], q1 = a.q[o1], q2 = a.q[o2];
  const double c0 = a.conv[3 * at], c1 = a.conv[3 * at + 1], c2 = a.conv[3 * at + 2];
  const double x0 = a.xyz0[3 * at] + c0 * q0;
  const double x1 = a.xyz0[3 * at + 1] + c1 * q1;
  const double x2 = a.xyz0[3 * at + 2] + c2 * q2;
  double f0 = 0.0, f1 = 0.0, f2 = 0.0;
  const int k0 = a.rp[at], k1 = a.rp[at + 1];
  for (int k = k0; k < k1; ++k) {
    const PairNbr* __restrict__ n = a.nbr + k;
    const int j = n->j;
    const int64_t j0 = (int64_t)(3 * j) * a.B + b;
    const double d0 = (a.xyz0[3 * j] + a.conv[3 * j] * a.q[j0]) + n->s[0] - x0;
    const double d1 = (a.xyz0[3 * j + 1] + a.conv[3 * j + 1] * a.q[j0 + a.B]) + n->s[1] - x1;
    const double d2 = (a.xyz0[3 * j + 2] + a.conv[3 * j + 2] * a.q[j0 + 2 * (int64_t)a.B]) + n->s[2] - x2;
    const double gg = pair_g(n->style, n->p, d0 * d0 + d1 * d1 + d2 * d2);
    f0 += gg * d0;
    f1 += gg * d1;
    f2 += gg * d2;
  }
  a.F[o0] = mul_sub(c0, f0, a.f0[3 * at]);
  a.F[o1] = mul_sub(c1, f1, a.f0[3 * at + 1]);
  a.F[o2] = mul_sub(c2, f2, a.f0[3 * at + 2]);
  if (a.cached) {
    a.Q0[o0] = q0;
    a.Q0[o1] = q1;
    a.Q0[o2] = q2;
    if (at == 0) {  // one thread per trajectory and launch; launches are ordered on the stream
      a.valid[b] = 1;
      a.count[b] += 1ull;
    }
  }
}

}  // namespace

void launch_pair_dist(const PairFFArgs& a, hipStream_t s) {
  if (a.B <= 0 || a.natom <= 0) return;
  GLE_BOUNDS_SYNC();
  pair_dist_kernel<<<dim3((unsigned)((a.B + 63) / 64), (unsigned)a.nchunk), 256, 0, s>>>(a);
}

void launch_pair_force(const PairFFArgs& a, hipStream_t s) {
  const int64_t n = (int64_t)a.natom * a.B;
  if (n <= 0) return;
  GLE_BOUNDS_SYNC();
  pair_force_kernel<<<(unsigned)((n + 255) / 256), 256, 0, s>>>(a);
}

}  // namespace gle
