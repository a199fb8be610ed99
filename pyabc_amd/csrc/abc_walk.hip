// Integer parameters on the device: grid priors (a table per coordinate over
// consecutive integers) and DiscreteRandomWalkTransition.
//
// Reference:
//   Distribution.pdf / rvs  pyabc/random_variables.py:412-452 (discrete
//     components: scipy pmf / rvs)            -> abc_grid_prior_logpmf / _draw
//   DiscreteRandomWalkTransition.rvs_single   pyabc/transition/randomwalk.py:42-53
//     + the prior re-draw loop smc.py:649-662 -> abc_walk_propose
//   DiscreteRandomWalkTransition.pdf          randomwalk.py:55-81
//                                             -> abc_walk_logpmf
// The density is the N_acc x N_pop pair loop of the continuous transitions
// with integer work: per pair d subtractions and range tests, and for the few
// pairs within n_steps in every coordinate a gather from the law's table.
// No floating-point atomics anywhere: the sums have one order.
#include "abc_candidate.h"

#pragma clang fp contract(off)

namespace abc {
namespace {

constexpr int WALK_T = 256;            // threads per block, one candidate each
constexpr int WALK_TILE = 256;         // population rows per LDS tile
constexpr int WALK_LAW = 2 * ABC_WALK_MAX_STEPS + 1;
constexpr int WALK_MAX_CHUNKS = 256;   // gridDim.y of the density kernel
constexpr int WALK_BLOCKS = 2048;      // blocks wanted before N is split
constexpr int32_t WALK_CAP = 1 << 30;  // |population entry| <= WALK_CAP
// a candidate coordinate beyond the cap: further than ABC_WALK_MAX_STEPS from
// every packed particle, and (uint32) (FAR - X + n) does not wrap onto
// [0, 2 n] for |X| <= WALK_CAP, n <= 512 (2^31 + 1536 < 2^32)
constexpr int32_t WALK_FAR = WALK_CAP + 2 * ABC_WALK_MAX_STEPS;

struct GridCoord { int64_t k_lo, len, off, last; };

__device__ __forceinline__ GridCoord grid_coord(const int64_t* coord, int k) {
  return {coord[4 * k], coord[4 * k + 1], coord[4 * k + 2], coord[4 * k + 3]};
}

// one coordinate's log mass at the integer v
__device__ __forceinline__ double grid_logpmf_int(const GridCoord& c, const double* logpmf,
                                                  int64_t v) {
  const int64_t i = v - c.k_lo;
  return (i >= 0 && i < c.len) ? logpmf[c.off + i] : -INFINITY;
}

// one coordinate's log mass at the double v: NaN unless v is an integer
__device__ __forceinline__ double grid_logpmf1(const GridCoord& c, const double* logpmf,
                                               double v) {
  if (!(v == floor(v))) return NAN;              // NaN, a fraction
  const double lo = (double)c.k_lo, hi = (double)(c.k_lo + c.len - 1);
  if (v < lo || v > hi) return -INFINITY;        // (+-inf lands here)
  return logpmf[c.off + (int64_t)(v - lo)];
}

__global__ __launch_bounds__(256) void grid_logpmf_kernel(
    const double* __restrict__ theta, int64_t B, int d, const int64_t* __restrict__ coord,
    const double* __restrict__ logpmf, double* __restrict__ lp) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  double s = 0.0;
  for (int k = 0; k < d; ++k)
    s += grid_logpmf1(grid_coord(coord, k), logpmf, theta[b * d + k]);
  lp[b] = s;
}

// first index in [0, n) with a[i] >= t (n when there is none)
__device__ __forceinline__ int64_t first_ge(const double* a, int64_t n, double t) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (a[mid] >= t) hi = mid; else lo = mid + 1;
  }
  return lo;
}

__global__ __launch_bounds__(256) void grid_draw_kernel(
    int64_t B, int d, const int64_t* __restrict__ coord, const double* __restrict__ cdf,
    uint64_t seed, uint32_t gen, int64_t idx0, double* __restrict__ theta) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const uint64_t g = (uint64_t)(idx0 + b);
  for (int k = 0; k < d; ++k) {
    const GridCoord c = grid_coord(coord, k);
    const u32x4 r = philox(g, SLOT_PRIOR + 512u * (uint32_t)k, gen, seed);
    // abc_prior_uniforms' value: 53 bits plus a half, in (0, 1)
    const double u = ((double)(r.x >> 5) * 67108864.0 + (double)(r.y >> 6) + 0.5) *
                     (1.0 / 9007199254740992.0);
    const double* ck = cdf + c.off;
    int64_t i = first_ge(ck, c.len, u * ck[c.len - 1]);
    i = i > c.last ? c.last : i;
    theta[b * d + k] = (double)(c.k_lo + i);
  }
}

// ---- pack -----------------------------------------------------------------
__global__ __launch_bounds__(256) void walk_pack_kernel(
    const double* __restrict__ X, int64_t n, int32_t* __restrict__ Xi,
    unsigned long long* __restrict__ bad) {
  __shared__ int cnt[4];
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int mine = 0;
  if (e < n) {
    const double v = X[e];
    const bool ok = v == floor(v) && fabs(v) <= (double)WALK_CAP;   // NaN: false
    Xi[e] = ok ? (int32_t)v : 0;
    mine = ok ? 0 : 1;
  }
  const int wave = __popcll(__ballot(mine));
  if ((threadIdx.x & 63) == 0) cnt[threadIdx.x >> 6] = wave;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int tot = cnt[0] + cnt[1] + cnt[2] + cnt[3];
    if (tot) atomicAdd(bad, (unsigned long long)tot);   // integer: order-free
  }
}

// ---- proposal ---------------------------------------------------------------
__global__ __launch_bounds__(WALK_T) void walk_propose_kernel(
    const int32_t* __restrict__ Xi, const double* __restrict__ cdf,
    const int32_t* __restrict__ guide, int64_t N, int d, const double* __restrict__ law_cum,
    int n, int law_last, const int64_t* __restrict__ coord, const double* __restrict__ logpmf,
    uint64_t seed, uint32_t gen, int64_t idx0, int64_t B, int max_attempts,
    double* __restrict__ theta, double* __restrict__ lp_out, int64_t* __restrict__ ancestor,
    int32_t* __restrict__ attempts) {
  __shared__ double cum[WALK_LAW];
  const int nl = 2 * n + 1;
  for (int i = threadIdx.x; i < nl; i += WALK_T) cum[i] = law_cum[i];
  __syncthreads();
  const int64_t b = (int64_t)blockIdx.x * WALK_T + threadIdx.x;
  if (b >= B) return;
  const uint64_t g = (uint64_t)(idx0 + b);
  const double total = cdf[N - 1], ltot = cum[nl - 1];
  int64_t j = -1;
  double lp = -INFINITY;
  int used = max_attempts + 1;
  for (int att = 0; att < max_attempts; ++att) {
    const uint32_t s0 = (uint32_t)att * SLOTS_PER_ATTEMPT;
    const u32x4 ra = philox(g, s0 + SLOT_ANCESTOR, gen, seed);
    j = ancestor_search(cdf, guide, N, total, uniform53(ra.x, ra.y) * total);
    u32x4 r = ra;
    double s = 0.0;
    for (int k = 0; k < d; ++k) {
      if ((k & 1) == 0) r = philox(g, s0 + SLOT_PERTURB + (uint32_t)(k >> 1), gen, seed);
      const double t = ((k & 1) ? uniform53(r.z, r.w) : uniform53(r.x, r.y)) * ltot;
      int lo = 0, hi = nl;                     // first index with cum > t
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cum[mid] > t) hi = mid; else lo = mid + 1;
      }
      lo = lo > law_last ? law_last : lo;
      const int32_t v = Xi[j * d + k] + (lo - n);
      theta[b * d + k] = (double)v;
      if (coord) s += grid_logpmf_int(grid_coord(coord, k), logpmf, (int64_t)v);
    }
    if (!coord || s > -INFINITY) {             // prior mass > 0 (smc.py:654-656)
      lp = s;
      used = att + 1;
      break;
    }
  }
  if (lp_out) lp_out[b] = lp;
  if (ancestor) ancestor[b] = j;
  if (attempts) attempts[b] = used;
}

// ---- density ------------------------------------------------------------------
// Block: WALK_T candidates (one per lane, coordinates as int32 in registers)
// against the chunk blockIdx.y of the population, streamed through LDS in
// tiles of WALK_TILE rows.  Every lane reads the same tile address (broadcast,
// no bank conflict).  All d range tests come first, one unsigned compare each;
// the law is gathered only for the pairs that pass all of them.  D > 0: the
// dimension at compile time; D == 0: d <= ABC_WALK_MAX_D at run time.
template <int D>
__global__ __launch_bounds__(WALK_T) void walk_logpmf_kernel(
    const double* __restrict__ x, int64_t M, const int32_t* __restrict__ Xi,
    const double* __restrict__ w, int64_t N, int d_rt, const double* __restrict__ law_g, int n,
    int64_t chunk, double* __restrict__ part) {
  constexpr int DR = D > 0 ? D : ABC_WALK_MAX_D;
  __shared__ double law[WALK_LAW];
  __shared__ double sw[WALK_TILE];
  __shared__ int32_t sX[WALK_TILE * DR];
  const int d = D > 0 ? D : d_rt;
  const int t = threadIdx.x;
  for (int i = t; i < 2 * n + 1; i += WALK_T) law[i] = law_g[i];
  const int64_t i = (int64_t)blockIdx.x * WALK_T + t;
  int32_t xi[DR];
  bool frac = false;   // a coordinate that is no integer (or NaN)
#pragma unroll
  for (int k = 0; k < DR; ++k) {
    xi[k] = WALK_FAR;
    if (k < d && i < M) {
      const double v = x[i * d + k];
      if (!(v == floor(v))) frac = true;
      else if (fabs(v) <= (double)WALK_CAP) xi[k] = (int32_t)v;
      else xi[k] = v > 0.0 ? WALK_FAR : -WALK_FAR;
    }
  }
  const uint32_t un = (uint32_t)n, two_n = 2u * (uint32_t)n;
  const int64_t j0 = (int64_t)blockIdx.y * chunk;
  const int64_t j1 = j0 + chunk < N ? j0 + chunk : N;
  double acc = 0.0;
  for (int64_t jt = j0; jt < j1; jt += WALK_TILE) {
    const int rows = (int)(j1 - jt < WALK_TILE ? j1 - jt : WALK_TILE);
    __syncthreads();                       // the previous tile is consumed
    for (int e = t; e < rows * d; e += WALK_T) sX[e] = Xi[jt * d + e];
    if (t < rows) sw[t] = w[jt + t];
    __syncthreads();
    for (int r = 0; r < rows; ++r) {
      const int32_t* row = sX + r * d;
      bool ok = true;
#pragma unroll
      for (int k = 0; k < DR; ++k)
        if (k < d) ok = ok & ((uint32_t)xi[k] - (uint32_t)row[k] + un <= two_n);
      if (ok) {
        double p = law[(uint32_t)xi[0] - (uint32_t)row[0] + un];
#pragma unroll
        for (int k = 1; k < DR; ++k)
          if (k < d) p = p * law[(uint32_t)xi[k] - (uint32_t)row[k] + un];
        acc = acc + p * sw[r];
      }
    }
  }
  if (i < M) part[(int64_t)blockIdx.y * M + i] = frac ? NAN : acc;
}

// chunks in ascending order, then the log (log 0 = -inf, NaN stays)
__global__ __launch_bounds__(256) void walk_finish_kernel(
    const double* __restrict__ part, int64_t M, int chunks, double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M) return;
  double s = part[i];
  for (int c = 1; c < chunks; ++c) s = s + part[(int64_t)c * M + i];
  out[i] = log(s);
}

// The dimensions the density kernel holds at compile time.
using WalkDims = std::integer_sequence<int, 1, 2, 3, 4, 5, 6, 7, 8>;

// particles per chunk: a multiple of the tile, from (M, N, d) alone.  N is
// split only while the candidate blocks alone are fewer than WALK_BLOCKS.
int64_t walk_chunk(int64_t M, int64_t N, int d) {
  (void)d;
  const int64_t mb = ceil_div(M > 0 ? M : 1, WALK_T);
  const int64_t tiles = ceil_div(N > 0 ? N : 1, WALK_TILE);
  int64_t c = ceil_div(WALK_BLOCKS, mb);
  c = c < 1 ? 1 : (c > WALK_MAX_CHUNKS ? WALK_MAX_CHUNKS : c);
  c = c > tiles ? tiles : c;
  return ceil_div(tiles, c) * WALK_TILE;
}

struct WalkWs {
  double* part;   // [chunks x M]
  void carve(Carver& c, int64_t M, int64_t N, int d) {
    const int64_t len = walk_chunk(M, N, d);
    part = c.take<double>((size_t)(ceil_div(N > 0 ? N : 1, len) * (M > 0 ? M : 1)));
  }
};

int check_grid(const abc_grid_prior* p, const char* who) {
  if (!p) return set_error(ABC_ERR_INVALID, "%s: null prior", who);
  if (p->d < 1 || p->d > 64) return set_error(ABC_ERR_INVALID, "%s: prior d outside 1..64", who);
  if (!p->coord || !p->logpmf || !p->cdf)
    return set_error(ABC_ERR_INVALID, "%s: null prior table", who);
  return ABC_OK;
}

}  // namespace
}  // namespace abc

using namespace abc;

extern "C" int abc_grid_prior_logpmf(const double* theta, int64_t B,
                                     const abc_grid_prior* prior, double* lp, void* stream) {
  ABC_CHECK_ARG(B >= 0, "grid_prior_logpmf: B < 0");
  if (int rc = check_grid(prior, "grid_prior_logpmf")) return rc;
  if (B == 0) return ABC_OK;
  ABC_CHECK_ARG(theta && lp, "grid_prior_logpmf: null pointer");
  hipLaunchKernelGGL(grid_logpmf_kernel, dim3((unsigned)ceil_div(B, 256)), dim3(256), 0,
                     as_stream(stream), theta, B, prior->d, prior->coord, prior->logpmf, lp);
  ABC_LAUNCHED();
  return ABC_OK;
}

extern "C" int abc_grid_prior_draw(const abc_grid_prior* prior, uint64_t seed,
                                   uint32_t generation, int64_t idx0, int64_t B,
                                   double* theta, void* stream) {
  ABC_CHECK_ARG(B >= 0, "grid_prior_draw: B < 0");
  if (int rc = check_grid(prior, "grid_prior_draw")) return rc;
  if (B == 0) return ABC_OK;
  ABC_CHECK_ARG(theta, "grid_prior_draw: null pointer");
  hipLaunchKernelGGL(grid_draw_kernel, dim3((unsigned)ceil_div(B, 256)), dim3(256), 0,
                     as_stream(stream), B, prior->d, prior->coord, prior->cdf, seed, generation,
                     idx0, theta);
  ABC_LAUNCHED();
  return ABC_OK;
}

extern "C" int abc_walk_pack(const double* X, int64_t N, int d, int32_t* Xi, int64_t* bad,
                             void* stream) {
  ABC_CHECK_ARG(N >= 0 && d >= 1, "walk_pack: bad N/d");
  if (d > ABC_WALK_MAX_D)
    return set_error(ABC_ERR_UNSUPPORTED, "walk_pack: d > %d", ABC_WALK_MAX_D);
  ABC_CHECK_ARG(bad, "walk_pack: null pointer");
  ABC_CHECK_ARG(N == 0 || (X && Xi), "walk_pack: null pointer");
  ABC_HIP(hipMemsetAsync(bad, 0, sizeof(int64_t), as_stream(stream)));
  if (N == 0) return ABC_OK;
  const int64_t n = N * d;
  hipLaunchKernelGGL(walk_pack_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0,
                     as_stream(stream), X, n, Xi, reinterpret_cast<unsigned long long*>(bad));
  ABC_LAUNCHED();
  return ABC_OK;
}

extern "C" int abc_walk_propose(const int32_t* Xi, const double* cdf, const int32_t* guide,
                                int64_t N, int d, const double* law_cum, int n_steps,
                                int law_last, const abc_grid_prior* prior, uint64_t seed,
                                uint32_t generation, int64_t idx0, int64_t B,
                                int max_attempts, double* theta, double* prior_logpmf,
                                int64_t* ancestor, int32_t* attempts, void* stream) {
  ABC_CHECK_ARG(d >= 1 && n_steps >= 1 && B >= 0 && max_attempts >= 1,
                "walk_propose: bad d/n_steps/B/max_attempts");
  ABC_CHECK_ARG(max_attempts < (1 << 15), "walk_propose: max_attempts too large");
  if (d > ABC_WALK_MAX_D || n_steps > ABC_WALK_MAX_STEPS)
    return set_error(ABC_ERR_UNSUPPORTED, "walk_propose: d > %d or n_steps > %d",
                     ABC_WALK_MAX_D, ABC_WALK_MAX_STEPS);
  ABC_CHECK_ARG(law_last >= 0 && law_last <= 2 * n_steps, "walk_propose: bad law_last");
  ABC_CHECK_ARG(N >= 1 && N < (1ll << 31), "walk_propose: bad N");
  if (prior) {
    if (int rc = check_grid(prior, "walk_propose")) return rc;
    ABC_CHECK_ARG(prior->d == d, "walk_propose: prior d differs");
  }
  if (B == 0) return ABC_OK;
  ABC_CHECK_ARG(Xi && cdf && law_cum && theta, "walk_propose: null pointer");
  hipLaunchKernelGGL(walk_propose_kernel, dim3((unsigned)ceil_div(B, WALK_T)), dim3(WALK_T), 0,
                     as_stream(stream), Xi, cdf, guide, N, d, law_cum, n_steps, law_last,
                     prior ? prior->coord : nullptr, prior ? prior->logpmf : nullptr, seed,
                     generation, idx0, B, prior ? max_attempts : 1, theta, prior_logpmf,
                     ancestor, attempts);
  ABC_LAUNCHED();
  return ABC_OK;
}

extern "C" int64_t abc_walk_logpmf_chunk(int64_t M, int64_t N, int d) {
  return walk_chunk(M, N, d);
}

extern "C" size_t abc_walk_logpmf_bytes(int64_t M, int64_t N, int d) {
  return measure<WalkWs>(M, N, d);
}

extern "C" int abc_walk_logpmf(const double* x, int64_t M, const int32_t* Xi,
                               const double* w, int64_t N, int d, const double* law,
                               int n_steps, double* out, void* ws, size_t ws_bytes,
                               void* stream) {
  ABC_CHECK_ARG(M >= 0 && N >= 1 && d >= 1 && n_steps >= 1, "walk_logpmf: bad M/N/d/n_steps");
  if (d > ABC_WALK_MAX_D || n_steps > ABC_WALK_MAX_STEPS)
    return set_error(ABC_ERR_UNSUPPORTED, "walk_logpmf: d > %d or n_steps > %d",
                     ABC_WALK_MAX_D, ABC_WALK_MAX_STEPS);
  ABC_CHECK_ARG(M < (1ll << 31) * WALK_T, "walk_logpmf: M too large");
  if (M == 0) return ABC_OK;
  ABC_CHECK_ARG(x && Xi && w && law && out && ws, "walk_logpmf: null pointer");
  WalkWs W;
  ABC_CARVE(W, "walk_logpmf", M, N, d);
  const int64_t chunk = walk_chunk(M, N, d);
  const int chunks = (int)ceil_div(N, chunk);
  const dim3 grid((unsigned)ceil_div(M, WALK_T), (unsigned)chunks);
  hipStream_t s = as_stream(stream);
  auto launch = [&](auto D) {
    hipLaunchKernelGGL(walk_logpmf_kernel<decltype(D)::value>, grid, dim3(WALK_T), 0, s, x, M,
                       Xi, w, N, d, law, n_steps, chunk, W.part);
  };
  if (!dispatch_int(WalkDims{}, d, launch)) launch(std::integral_constant<int, 0>{});
  ABC_LAUNCHED();
  hipLaunchKernelGGL(walk_finish_kernel, dim3((unsigned)ceil_div(M, 256)), dim3(256), 0, s,
                     W.part, M, chunks, out);
  ABC_LAUNCHED();
  return ABC_OK;
}
