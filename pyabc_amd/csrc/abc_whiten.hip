// The measure-list distances' device kernels: PCADistance's whitened norm and
// its accept tail, the centred Gram matrix its whitening matrix is made
// from, and the per-column percentile of PercentileDistance.
//
// Reference: pyabc/distance/distance.py
//   PCADistance.__call__ :731-739
//       la.norm(W.dot(x_vec - x_0_vec), 2)
//   PCADistance._calculate_whitening_transformation_matrix :709-715
//       means = samples_vec.mean(axis=0); centered = samples_vec - means
//       covariance = centered.T.dot(centered)
//   PercentileDistance.upper / lower :860-868
//       np.percentile(parameter_list, 100 - PERCENTILE / PERCENTILE)
//
// Everything is fp64 with a fixed summation order and no floating-point
// atomics: two calls give the same bits.
//
// abc_whitened_norm: [B x S] . [S x S]^T with a row-norm epilogue on
// v_mfma_f64_16x16x4_f64.  A block takes 64 candidates, 16 per wave; a wave
// keeps its 16 rows of x - x0 in registers as the A operand of every K step
// (K = S padded with zeros to 4 KS, KS a power of two <= 64) and W passes
// through LDS in panels of 16 output columns (16 rows of W: 33 KB at
// S = 256, where all of W is 512 KB).  Per panel a wave runs KS MFMAs into
// up to four independent accumulators (the f64 MFMA's dependent latency is
// longer than its issue interval), squares the panel's 16 outputs of each of
// its rows and carries the row sums in registers; after the last panel the
// 16 lanes of a row are summed by shuffles.  LDS rows are KP + 2 doubles:
// the fragment read of lanes (row l & 15, k l >> 4) then touches 32 different
// 8-byte slots per half wave.
// The f64 MFMA's lane maps (they differ from every other shape's C/D map):
//   A[i][k]: lane l holds i = l & 15, k = l >> 4;  B[k][n]: k = l >> 4, n = l & 15;
//   D[i][n]: register q of lane l is i = (l >> 4) + 4 q, n = l & 15.
#include "abc_accept_words.h"
#include "abc_column_ws.h"

namespace abc {
namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int WH_T = 256;      // 4 waves
constexpr int WH_ROWS = 64;    // candidates per block: one accept word

// rows row0 .. row0 + 15 of the row-major [nrows x S] matrix src into
// lds[16][KP + 2], zeros beyond its rows and columns (every thread calls it)
template <int KP>
__device__ __forceinline__ void stage16(const double* __restrict__ src, int64_t row0,
                                        int64_t nrows, int S, double* lds) {
  constexpr int LD = KP + 2;
  constexpr int N = 16 * KP;
#pragma unroll
  for (int e0 = 0; e0 < N; e0 += WH_T) {
    const int e = e0 + (int)threadIdx.x;
    if (N % WH_T != 0 && e >= N) break;
    const int r = e / KP, c = e % KP;
    double v = 0.0;
    if (c < S && row0 + r < nrows) v = src[(row0 + r) * S + c];
    lds[r * LD + c] = v;
  }
}

// The distances of the block's rows: dist[q] of lane l is the distance of row
// b0 + 16 wave + (l >> 4) + 4 q (every lane of the row's 16 holds it).  Every
// thread of the block calls it (barriers inside).  One definition: the norm
// and the accept tail get the same bits.
template <int KS>
__device__ __forceinline__ void whitened_rows(const double* __restrict__ x, int64_t B, int S,
                                              const double* __restrict__ x0,
                                              const double* __restrict__ W, int64_t b0,
                                              double* tile, double* x0s, double dist[4]) {
  constexpr int KP = 4 * KS, LD = KP + 2;
  constexpr int NA = KS >= 4 ? 4 : KS;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int lr = lane & 15, lk = lane >> 4;
  for (int c = t; c < KP; c += WH_T) x0s[c] = c < S ? x0[c] : 0.0;
  double a[KS];
#pragma unroll
  for (int w = 0; w < WH_T / 64; ++w) {
    __syncthreads();                       // x0s written; the previous rows read
    stage16<KP>(x, b0 + 16 * w, B, S, tile);
    __syncthreads();
    if (wave == w) {
#pragma unroll
      for (int kk = 0; kk < KS; ++kk) a[kk] = tile[lr * LD + 4 * kk + lk] - x0s[4 * kk + lk];
    }
  }
  double ss[4] = {0.0, 0.0, 0.0, 0.0};
  const int npanel = (S + 15) / 16;
#pragma unroll 1
  for (int pn = 0; pn < npanel; ++pn) {
    __syncthreads();                       // the previous panel read
    stage16<KP>(W, 16 * pn, S, S, tile);
    __syncthreads();
    f64x4 acc[NA];
#pragma unroll
    for (int c = 0; c < NA; ++c) acc[c] = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int kk = 0; kk < KS; ++kk)
      acc[kk % NA] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[kk], tile[lr * LD + 4 * kk + lk],
                                                          acc[kk % NA], 0, 0, 0);
    f64x4 y = acc[0];
    if (NA == 2) y = acc[0] + acc[1];
    if (NA == 4) y = (acc[0] + acc[1]) + (acc[2] + acc[3]);
    // output column 16 pn + lr: a padded one would turn an infinite
    // difference into inf * 0
    if (16 * pn + lr < S) {
#pragma unroll
      for (int q = 0; q < 4; ++q) ss[q] = __builtin_fma(y[q], y[q], ss[q]);
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) ss[q] += __shfl_xor(ss[q], o, 64);
    dist[q] = sqrt(ss[q]);
  }
}

template <int KS, bool ACCEPT>
__global__ __launch_bounds__(WH_T) void whitened_kernel(
    const double* __restrict__ x, int64_t B, int S, const double* __restrict__ x0,
    const double* __restrict__ W, double* __restrict__ d, double eps,
    const int32_t* __restrict__ att, int max_attempts, uint64_t* __restrict__ bits) {
  __shared__ double tile[16 * (4 * KS + 2)];
  __shared__ double x0s[4 * KS];
  __shared__ uint32_t tbits[WH_ROWS / 32];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t b0 = (int64_t)blockIdx.x * WH_ROWS;
  if (ACCEPT && t < WH_ROWS / 32) tbits[t] = 0u;   // (barriers follow in whitened_rows)
  double dist[4];
  whitened_rows<KS>(x, B, S, x0, W, b0, tile, x0s, dist);
  if ((lane & 15) == 0) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int loc = 16 * wave + (lane >> 4) + 4 * q;
      const int64_t b = b0 + loc;
      if (b < B) {
        if (!ACCEPT) {
          d[b] = dist[q];
        } else if (dist[q] <= eps && (att == nullptr || att[b] <= max_attempts)) {
          atomicOr(&tbits[loc >> 5], 1u << (loc & 31));
        }
      }
    }
  }
  if (ACCEPT) {
    __syncthreads();
    if (t == 0) bits[blockIdx.x] = (uint64_t)tbits[0] | ((uint64_t)tbits[1] << 32);
  }
}

// K steps per row: ceil(S / 4) rounded up to a power of two
using WhitenKS = std::integer_sequence<int, 1, 2, 4, 8, 16, 32, 64>;
constexpr int WHITEN_MAX_S = 256;
inline int whiten_ks(int S) {
  int ks = 1;
  while (4 * ks < S) ks *= 2;
  return ks;
}

template <bool ACCEPT>
int launch_whitened(const double* x, int64_t B, int S, const double* x0, const double* W,
                    double* d, double eps, const int32_t* att, int max_attempts, uint64_t* bits,
                    hipStream_t s) {
  const unsigned nb = (unsigned)ceil_div(B, WH_ROWS);
  dispatch_int(WhitenKS{}, whiten_ks(S), [&](auto KS) {
    hipLaunchKernelGGL((whitened_kernel<KS(), ACCEPT>), dim3(nb), dim3(WH_T), 0, s, x, B, S, x0,
                       W, d, eps, att, max_attempts, bits);
  });
  ABC_LAUNCHED();
  return ABC_OK;
}

// ---- centred Gram matrix ------------------------------------------------------
// A wave takes one row split of a 16 x 64 strip of G: the 16 columns i of the
// A operand against four 16-column tiles j, K = the split's rows in steps of
// 4 (A[i][k] = X[r0 + k][i] - mean[i], B[k][j] likewise), four independent
// accumulators.  G[i][j] and G[j][i] sum the same products in the same order.
constexpr int GR_NJ = 4;
__global__ __launch_bounds__(256) void gram_partial_kernel(const double* __restrict__ X,
                                                           int64_t R, int S,
                                                           const double* __restrict__ mean,
                                                           int nsplit, int64_t rps,
                                                           double* __restrict__ part) {
  const int lane = threadIdx.x & 63, lr = lane & 15, lk = lane >> 4;
  const int nti = (S + 15) / 16, ntg = (nti + GR_NJ - 1) / GR_NJ;
  const int64_t task = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (task >= (int64_t)nsplit * nti * ntg) return;        // whole wave
  const int tg = (int)(task % ntg), ti = (int)((task / ntg) % nti);
  const int sp = (int)(task / ((int64_t)ntg * nti));
  const int64_t r0 = sp * rps;
  const int64_t r1 = r0 + rps < R ? r0 + rps : R;
  const int i = 16 * ti + lr;
  const bool vi = i < S;
  const double mi = vi ? mean[i] : 0.0;
  int j[GR_NJ];
  bool vj[GR_NJ];
  double mj[GR_NJ];
  f64x4 acc[GR_NJ];
#pragma unroll
  for (int q = 0; q < GR_NJ; ++q) {
    j[q] = 16 * (tg * GR_NJ + q) + lr;
    vj[q] = j[q] < S;
    mj[q] = vj[q] ? mean[j[q]] : 0.0;
    acc[q] = f64x4{0.0, 0.0, 0.0, 0.0};
  }
#pragma unroll 4
  for (int64_t rb = r0; rb < r1; rb += 4) {
    const int64_t r = rb + lk;
    const bool vr = r < r1;
    const double av = (vr && vi) ? X[r * S + i] - mi : 0.0;
#pragma unroll
    for (int q = 0; q < GR_NJ; ++q) {
      if (tg * GR_NJ + q < nti) {                         // wave-uniform
        const double bv = (vr && vj[q]) ? X[r * S + j[q]] - mj[q] : 0.0;
        acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc[q], 0, 0, 0);
      }
    }
  }
  double* out = part + (int64_t)sp * S * S;
#pragma unroll
  for (int q = 0; q < GR_NJ; ++q) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int row = 16 * ti + lk + 4 * g;
      if (row < S && vj[q]) out[(int64_t)row * S + j[q]] = acc[q][g];
    }
  }
}

// the splits' blocks in split order; the means leave the workspace
__global__ __launch_bounds__(256) void gram_combine_kernel(const double* __restrict__ part,
                                                           int nsplit, int S,
                                                           const double* __restrict__ mean_ws,
                                                           double* __restrict__ mean,
                                                           double* __restrict__ G) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e < S) mean[e] = mean_ws[e];
  if (e >= S * S) return;
  double s = 0.0;
  for (int sp = 0; sp < nsplit; ++sp) s += part[(int64_t)sp * S * S + e];
  G[e] = s;
}

// out[c] = NaN for every column of X that holds one (out zeroed before; the
// blocks that find one all store the same value).  Thread t reads column
// t % CB of the rows sub + rpb i of its block's share, CB = min(S, 256)
// columns at a time: a block's threads read consecutive doubles, 8 rows in
// flight per thread (colsum_kernel's traversal).
constexpr int NAN_BLOCKS = 256, NAN_U = 8;
__global__ __launch_bounds__(256) void column_nan_kernel(const double* __restrict__ X, int64_t R,
                                                         int S, double* __restrict__ out) {
  const int CB = S < 256 ? S : 256;
  const int rpb = 256 / CB;
  const int cl = threadIdx.x % CB, sub = threadIdx.x / CB;
  if (sub >= rpb) return;
  const int64_t step = (int64_t)gridDim.x * rpb;
  for (int c = cl; c < S; c += CB) {
    bool found = false;
    int64_t r = (int64_t)blockIdx.x * rpb + sub;
    for (; r + (NAN_U - 1) * step < R; r += NAN_U * step) {
      double v[NAN_U];
#pragma unroll
      for (int u = 0; u < NAN_U; ++u) v[u] = X[(r + u * step) * S + c];
#pragma unroll
      for (int u = 0; u < NAN_U; ++u) found |= v[u] != v[u];
    }
    for (; r < R; r += step) {
      const double v = X[r * S + c];
      found |= v != v;
    }
    if (found) out[c] = NAN;
  }
}

// out[c] is NaN where the column holds one: the NaN stays
__global__ void quantile_finish_kernel(const double* __restrict__ val, int S,
                                       double* __restrict__ out) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < S) out[c] = out[c] != out[c] ? out[c] : val[c];
}

}  // namespace
}  // namespace abc

using namespace abc;

extern "C" int abc_whitened_norm(const double* x, int64_t B, int S, const double* x0,
                                 const double* W, double* d, void* stream) {
  ABC_CHECK_ARG(S >= 1 && S <= WHITEN_MAX_S, "whitened_norm: S outside 1..%d", WHITEN_MAX_S);
  ABC_CHECK_ARG(B >= 0 && ceil_div(B, WH_ROWS) < (1ll << 31), "whitened_norm: bad B");
  if (B == 0) return ABC_OK;
  ABC_CHECK_ARG(x && x0 && W && d, "whitened_norm: null pointer");
  return launch_whitened<false>(x, B, S, x0, W, d, 0.0, nullptr, 0, nullptr, as_stream(stream));
}

extern "C" int abc_whitened_accept(const double* x, int64_t B, int S, const double* x0,
                                   const double* W, double eps, const int32_t* attempts,
                                   int max_attempts, int64_t cap, int64_t* idx, int64_t* count,
                                   void* ws, size_t ws_bytes, void* stream) {
  ABC_CHECK_ARG(S >= 1 && S <= WHITEN_MAX_S, "whitened_accept: S outside 1..%d", WHITEN_MAX_S);
  ABC_CHECK_ARG(B >= 0 && cap >= 0, "whitened_accept: bad B/cap");
  ABC_CHECK_ARG(B < (1ll << 36), "whitened_accept: B too large");
  ABC_CHECK_ARG(count && (cap == 0 || idx), "whitened_accept: null pointer");
  AcceptWords w;
  if (!accept_words_carve(ws, ws_bytes, B, w))
    return set_error(ABC_ERR_WORKSPACE, "whitened_accept: workspace too small");
  hipStream_t s = as_stream(stream);
  if (B == 0) {
    ABC_HIP(hipMemsetAsync(count, 0, sizeof(int64_t), s));
    return ABC_OK;
  }
  ABC_CHECK_ARG(x && x0 && W && ws, "whitened_accept: null pointer");
  const int rc = launch_whitened<true>(x, B, S, x0, W, nullptr, eps, attempts, max_attempts,
                                       w.bits, s);
  if (rc) return rc;
  return accept_words_compact(w, B, cap, idx, count, s);
}

extern "C" int abc_column_gram(const double* X, int64_t R, int S, double* mean, double* G,
                               void* ws, size_t ws_bytes, void* stream) {
  ABC_CHECK_ARG(R >= 1 && R <= (1ll << 40), "column_gram: bad R");
  ABC_CHECK_ARG(S >= 1 && S <= WHITEN_MAX_S, "column_gram: S outside 1..%d", WHITEN_MAX_S);
  ABC_CHECK_ARG(X && mean && G && ws, "column_gram: null pointer");
  GramBufs k;
  ABC_CARVE(k, "column_gram", R, S);
  hipStream_t s = as_stream(stream);
  int rc = column_mean(X, R, S, k.sd, s);
  if (rc) return rc;
  const int nti = (S + 15) / 16, ntg = (nti + GR_NJ - 1) / GR_NJ;
  const int64_t rps = ceil_div(ceil_div(R, k.nsplit), 4) * 4;
  const int64_t tasks = (int64_t)k.nsplit * nti * ntg;
  hipLaunchKernelGGL(gram_partial_kernel, dim3((unsigned)ceil_div(tasks, 4)), dim3(256), 0, s, X, R,
                     S, (const double*)k.sd.mean, k.nsplit, rps, k.gpart);
  ABC_LAUNCHED();
  hipLaunchKernelGGL(gram_combine_kernel, dim3((unsigned)ceil_div((int64_t)S * S, 256)), dim3(256),
                     0, s, (const double*)k.gpart, k.nsplit, S, (const double*)k.sd.mean, mean, G);
  ABC_LAUNCHED();
  return ABC_OK;
}

extern "C" int abc_column_quantile(const double* X, int64_t R, int S, double q, double* out,
                                   void* ws, size_t ws_bytes, void* stream) {
  ABC_CHECK_ARG(R >= 1 && S >= 1, "column_quantile: bad R/S");
  ABC_CHECK_ARG(q >= 0.0 && q <= 1.0, "column_quantile: q outside [0, 1]");
  ABC_CHECK_ARG(X && out && ws, "column_quantile: null pointer");
  ColumnStatsWs k;
  ABC_CARVE(k, "column_quantile", R, S);
  hipStream_t s = as_stream(stream);
  ABC_HIP(hipMemsetAsync(out, 0, sizeof(double) * S, s));
  const int64_t rows_at_once = 256 / (S < 256 ? S : 256);
  const int64_t want = ceil_div(R, rows_at_once);
  hipLaunchKernelGGL(column_nan_kernel, dim3((unsigned)(want < NAN_BLOCKS ? want : NAN_BLOCKS)),
                     dim3(256), 0, s, X, R, S, out);
  ABC_LAUNCHED();
  int rc = column_quantile_select(X, R, S, q, k.sel.med, k.sel, s);
  if (rc) return rc;
  hipLaunchKernelGGL(quantile_finish_kernel, dim3((unsigned)ceil_div(S, 256)), dim3(256), 0, s,
                     (const double*)k.sel.med, S, out);
  ABC_LAUNCHED();
  return ABC_OK;
}
