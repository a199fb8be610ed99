// What the transition densities share (abc_mvn.hip, abc_mvn_scaled.hip,
// abc_mvn_x3.hip, abc_local.hip, abc_local_wide.hip): constants, the (m, l)
// log-sum-exp pair, the whitened MFMA operand image, the tile / chunk plan,
// and the prototypes these files call each other through.
#pragma once
#include "abc_common.h"

namespace abc {

constexpr double LOG2E = 1.4426950408889634074;
constexpr double LN2 = 0.69314718055994530942;
constexpr double LOG_2PI = 1.8378770664093454836;

// ---- the (m, l) pair --------------------------------------------------------
// A sum of terms base^s is kept as (m, l) with value l * base^m: m a reference
// near the largest s, l the terms relative to it.  The pair is empty iff
// l == 0, and m of an empty pair means nothing (-inf, a start value, whatever
// the site left there): no rule below may read it as a term.  The base is a
// tag: natural (the direct fp64 kernels) or 2 (beside the MFMA kernels, whose
// exponents are in log2 units).
struct BaseE {
  static __device__ __forceinline__ double ex(double v) { return exp(v); }
};
struct Base2 {
  static __device__ __forceinline__ double ex(double v) { return exp2(v); }
};

struct LsePair { double m, l; };

// push one term base^s; m starts at -inf.  s = -inf onto an empty pair gives
// NaN: a site that can see it tests for it itself.
template <class B>
__device__ __forceinline__ void lse_add(double s, double& m, double& l) {
  if (s > m) { l = l * B::ex(m - s) + 1.0; m = s; }
  else l += B::ex(s - m);
}

// (m, l) += (mo, lo).  The new reference is the larger of both m, also when
// one side is empty (its l is not read, its m is).  Right where an empty
// side's m cannot lie far above a live one: it is -inf (lse_add's start), or
// mvn_lse_kernel's start |z|^2 log2e / 2, below which a live m sinks only as
// far as the density itself is small -- a sum 2^-1022 below that start is
// zero in the fp64 reference too.
template <class B>
__device__ __forceinline__ void lse_merge(double& m, double& l, double mo, double lo) {
  const double mx = fmax(m, mo);
  double s = 0.0;
  if (l > 0.0) s += l * B::ex(m - mx);
  if (lo > 0.0) s += lo * B::ex(mo - mx);
  m = (l > 0.0 || lo > 0.0) ? mx : m;
  l = s;
}

// The same, but an empty side does not raise the other side's reference.
// mvn_scaled_kernel needs this: its references start at 0 and move per grid
// point by hundreds of log2 units, so an empty side's start can lie far above
// the live side's m and the rescale to it would underflow the live sum.
// (m and l are read once, up front: mvn_scaled_kernel's code depends on it.)
template <class B>
__device__ __forceinline__ void lse_merge_live(double& m, double& l, double mo, double lo) {
  const double ma = m, la = l;
  const bool ha = la > 0.0, hb = lo > 0.0;
  const double mx = (ha && hb) ? fmax(ma, mo) : (ha ? ma : mo);
  double s = 0.0;
  if (ha) s += la * B::ex(ma - mx);
  if (hb) s += lo * B::ex(mo - mx);
  m = mx;
  l = s;
}

// The lane butterfly around either rule stays at its site -- offsets 16, 32
// for the four lane groups of an MFMA result, 32 .. 1 for a wave: inside a
// helper it changes how the compiler schedules the MFMA kernels' hot loops.

// Pairs pm / pl [c * stride + i], c < n (one per population chunk, slice or
// wave), into one: the largest m among the non-empty ones, then their sum
// rescaled to it.  All empty: {-inf, 0}.
template <class B>
__device__ __forceinline__ LsePair lse_combine(const double* pm, const double* pl,
                                               int64_t stride, int n, int64_t i) {
  double mx = -INFINITY;
  for (int c = 0; c < n; ++c)
    if (pl[(int64_t)c * stride + i] > 0.0) mx = fmax(mx, pm[(int64_t)c * stride + i]);
  double s = 0.0;
  for (int c = 0; c < n; ++c) {
    const double lv = pl[(int64_t)c * stride + i];
    if (lv > 0.0) s += lv * B::ex(pm[(int64_t)c * stride + i] - mx);
  }
  return {mx, s};
}

// The end of a direct kernel (one block of 256 per candidate, each thread's
// pair over its strided rows): wave butterfly, the waves' pairs through LDS,
// thread 0 writes the log density.
__device__ __forceinline__ void direct_finish(double m, double l, double log_const,
                                              double* __restrict__ out) {
  __shared__ double sm[4], sl[4];
  for (int o = 32; o > 0; o >>= 1) {
    const double mo = __shfl_xor(m, o, 64), lo = __shfl_xor(l, o, 64);
    lse_merge<BaseE>(m, l, mo, lo);
  }
  const int wv = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { sm[wv] = m; sl[wv] = l; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const LsePair p = lse_combine<BaseE>(sm, sl, 1, (int)(blockDim.x >> 6), 0);
    *out = (p.l > 0.0) ? p.m + log(p.l) + log_const : -INFINITY;
  }
}

// sum of one value per thread over a block of 256, fixed tree (deterministic)
__device__ __forceinline__ double block_sum256(double v, double* sh) {
  __syncthreads();
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  return sh[0];
}

// ---- the whitened operand image ---------------------------------------------
// image[tile][lane][kb] of a 16x16x4 MFMA operand (A: population rows, B:
// candidates), KB blocks of 4 columns.  Element (row, k) of a tile sits in
// lane row + 16 (k & 3), block k >> 2: lane L of a wave loads its operand of
// block kb, element (L & 15, 4 kb + (L >> 4)), from operand_lane_at(tile, L,
// kb) -- the layout of v_mfma_{f32,f64}_16x16x4.  The pack kernels write
// through operand_at, the hot kernels read through operand_lane_at (spelling
// their lane as (row, k) there changes their address arithmetic).
__device__ __forceinline__ int64_t operand_lane_at(int64_t tile, int lane, int kb, int KB) {
  return (tile * 64 + lane) * KB + kb;
}
__device__ __forceinline__ int64_t operand_at(int64_t tile, int row, int k, int KB) {
  return operand_lane_at(tile, row + 16 * (k & 3), k >> 2, KB);
}

// column k of (x - mu) U for one row x [d], U [d x r].  The product-sum keeps
// this shape: it contracts to one fma per term, and the bits depend on that.
__device__ __forceinline__ double whiten_row(const double* __restrict__ x,
                                             const double* __restrict__ mu,
                                             const double* __restrict__ U, int d, int r,
                                             int k) {
  double acc = 0.0;
  for (int q = 0; q < d; ++q) acc += (x[q] - mu[q]) * U[q * r + k];
  return acc;
}

// Tiles of 16 over M candidates and N population rows; a block is 4 waves of
// CT candidate tiles (groups of them, padded to MTpad tiles = Mpad columns).
// nc: the population chunks wanted, in [1, 1024] -- enough waves to fill 256
// CUs several times over, chunks of at least 32 tiles.  The caller settles the
// count (a multiple of 8 for the XCD map, or no empty chunk).
struct TilePlan {
  int64_t MT, NT, MTpad, groups, Mpad, nc;
};
inline TilePlan tile_plan(int64_t M, int64_t N, int CT) {
  TilePlan p;
  p.MT = ceil_div(M > 0 ? M : 1, 16);
  p.NT = ceil_div(N > 0 ? N : 1, 16);
  p.groups = ceil_div(ceil_div(p.MT, CT), 4);
  p.MTpad = p.groups * 4 * CT;
  p.Mpad = p.MTpad * 16;
  const int64_t want = ceil_div(16384, p.groups * 4);
  const int64_t maxc = ceil_div(p.NT, 32);
  const int64_t nc = want < maxc ? want : maxc;
  p.nc = nc < 1 ? 1 : (nc > 1024 ? 1024 : nc);
  return p;
}

// ---- between the translation units ------------------------------------------
// abc_mvn_x3.hip, called by abc_mvn.hip (ABC_PREC_X3)
size_t x3_packed_bytes(int64_t N, int r);
int x3_max_rank();
int x3_pack_population(const double* X, const double* w, int64_t N, int d,
                       const double* mu, const double* U, int r,
                       double log_w_shift, const double* shift_dev, void* packed,
                       double* range, hipStream_t s);
size_t x3_logpdf_workspace(int64_t M, int64_t N, int r);
int x3_logpdf(const double* x, int64_t M, int d, const void* packed,
              const double* X, const double* w, int64_t N, const double* mu,
              const double* U, int r, double log_const, double log_norm,
              double* out, const int64_t* hint, void* ws, size_t ws_bytes,
              hipStream_t s, int prof_channel = ABC_PROF_DENSITY,
              const unsigned int* count_dev = nullptr);

// abc_local_wide.hip, called by abc_local.hip: the runtime-d fit (d > 16) and
// the direct-difference density -- d > 16, and behind the MFMA route at
// d <= 16 for the candidates local_pdf_direct(uv, tmax) names
size_t local_wide_fit_workspace(int64_t N, int d);
int local_wide_fit(const double* X, const double* w, int64_t N, int d, int64_t nq,
                   double scaling, double eps, double* covs, double* invs, double* dets,
                   double* chol, double* lnorm, void* ws, size_t ws_bytes, hipStream_t s);
int local_wide_logpdf(const double* x, int64_t M, const double* X, const double* w,
                      int64_t N, int d, const double* inv, const double* lnorm,
                      double* out, hipStream_t s, const double* uv = nullptr,
                      double tmax = 0.0);

}  // namespace abc
