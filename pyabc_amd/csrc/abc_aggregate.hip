// AggregatedDistance / AdaptiveAggregatedDistance on the device: the term
// matrix and the aggregated distance of stored rows (abc_aggregate_distance;
// device code in abc_aggregate.h) and the span scale of a term matrix
// (abc_column_span).  The accept tail abc_aggregate_accept sits beside
// abc_pnorm_accept in abc_fused.hip, whose accept-word machinery it shares.
//
// Reference: pyabc/distance/distance.py:434-461 (AggregatedDistance.__call__),
// distance.py:560-601 (AdaptiveAggregatedDistance._update, which evaluates
// every child on every recorded sum stat and hands the columns to the scale
// function), pyabc/distance/scale.py:138-141 (span).
#include "abc_aggregate.h"
#include "abc_column_ws.h"

namespace abc {
namespace {

// S <= 32: one thread per row (pnorm_row_kernel's shape)
__global__ __launch_bounds__(256) void aggregate_row_kernel(
    const double* __restrict__ x, int64_t B, int S, const double* __restrict__ x0,
    const double* __restrict__ wf, const AggTerms T, double* __restrict__ d,
    double* __restrict__ terms) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const double dist = agg_row(x + b * S, S, x0, wf, T, [&](int k, double t) {
    if (terms) terms[b * T.K + k] = t;
  });
  if (d) d[b] = dist;
}

// wide rows: PNORM_ROWS rows per wave, four waves per block (pnorm_wave_kernel's shape)
template <bool SIMPLE>
__global__ __launch_bounds__(256) void aggregate_wave_kernel(
    const double* __restrict__ x, int64_t B, int S, const double* __restrict__ x0,
    const double* __restrict__ wf, const AggTerms T, double* __restrict__ d,
    double* __restrict__ terms) {
  const int64_t b0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * PNORM_ROWS;
  if (b0 >= B) return;  // whole wave
  agg_wave_rows<SIMPLE>(
      x, b0, B, S, x0, wf, T,
      [&](int r, int k, double t) { if (terms) terms[(b0 + r) * T.K + k] = t; },
      [&](int r, double dist) { if (d) d[b0 + r] = dist; });
}

// ---- span (scale.py:138-141): max - min per column, exact -----------------
// min / max that keep a NaN (fmin / fmax drop it)
__device__ __forceinline__ double nan_min(double a, double b) {
  return (a != a || b != b) ? NAN : (b < a ? b : a);
}
__device__ __forceinline__ double nan_max(double a, double b) {
  return (a != a || b != b) ? NAN : (b > a ? b : a);
}

constexpr int SPAN_T = 256;      // threads per block; K <= SPAN_T
constexpr int SPAN_BLOCKS = CS_BLOCKS / 2;   // (min, max) per block in ColumnStdBufs::part

// Thread t < (SPAN_T / K) K reads column t % K of rows rpb i + t / K: the
// block's threads read consecutive doubles.  part[(2 blk) K + k] = the
// block's min of column k, part[(2 blk + 1) K + k] its max (the identities
// +inf / -inf for a block without rows).
__global__ __launch_bounds__(SPAN_T) void span_partial_kernel(const double* __restrict__ V,
                                                              int64_t R, int K,
                                                              double* __restrict__ part) {
  __shared__ double smin[SPAN_T], smax[SPAN_T];
  const int t = threadIdx.x;
  const int rpb = SPAN_T / K;            // rows per block and step
  double lo = INFINITY, hi = -INFINITY;
  if (t < rpb * K) {
    const int k = t % K;
    for (int64_t r = (int64_t)blockIdx.x * rpb + t / K; r < R; r += (int64_t)gridDim.x * rpb) {
      const double v = V[r * K + k];
      lo = nan_min(lo, v);
      hi = nan_max(hi, v);
    }
  }
  smin[t] = lo;
  smax[t] = hi;
  __syncthreads();
  if (t < K) {
    for (int j = 1; j < rpb; ++j) {
      lo = nan_min(lo, smin[j * K + t]);
      hi = nan_max(hi, smax[j * K + t]);
    }
    part[(int64_t)(2 * blockIdx.x) * K + t] = lo;
    part[(int64_t)(2 * blockIdx.x + 1) * K + t] = hi;
  }
}

__global__ __launch_bounds__(SPAN_T) void span_final_kernel(const double* __restrict__ part,
                                                            int nblocks, int K,
                                                            double* __restrict__ out) {
  const int k = threadIdx.x;
  if (k >= K) return;
  double lo = INFINITY, hi = -INFINITY;
  for (int b = 0; b < nblocks; ++b) {
    lo = nan_min(lo, part[(int64_t)(2 * b) * K + k]);
    hi = nan_max(hi, part[(int64_t)(2 * b + 1) * K + k]);
  }
  out[k] = hi - lo;
}

}  // namespace
}  // namespace abc

using namespace abc;

extern "C" int abc_aggregate_distance(const double* x, int64_t B, int S, const double* x0,
                                      const double* wf, const double* p, const double* c,
                                      int K, double* d, double* terms, void* stream) {
  AggTerms T;
  const int rc = agg_check_terms("aggregate_distance", S, p, c, K, T);
  if (rc != ABC_OK) return rc;
  ABC_CHECK_ARG(B >= 0, "aggregate_distance: B < 0");
  ABC_CHECK_ARG(d || terms, "aggregate_distance: both outputs null");
  if (B == 0) return ABC_OK;
  ABC_CHECK_ARG(x && x0 && wf, "aggregate_distance: null pointer");
  hipStream_t s = as_stream(stream);
  // the same row / wave split as abc_pnorm (the same bits per term)
  if (S <= 32) {
    ABC_CHECK_ARG(ceil_div(B, 256) < (1ll << 31), "aggregate_distance: B too large");
    hipLaunchKernelGGL(aggregate_row_kernel, dim3((unsigned)ceil_div(B, 256)), dim3(256), 0, s,
                       x, B, S, x0, wf, T, d, terms);
  } else {
    const int64_t nb = ceil_div(B, 4 * PNORM_ROWS);
    ABC_CHECK_ARG(nb < (1ll << 31), "aggregate_distance: B too large");
    if (agg_simple(T.p, K))
      hipLaunchKernelGGL(aggregate_wave_kernel<true>, dim3((unsigned)nb), dim3(256), 0, s, x, B,
                         S, x0, wf, T, d, terms);
    else
      hipLaunchKernelGGL(aggregate_wave_kernel<false>, dim3((unsigned)nb), dim3(256), 0, s, x, B,
                         S, x0, wf, T, d, terms);
  }
  ABC_LAUNCHED();
  return ABC_OK;
}

extern "C" int abc_column_span(const double* V, int64_t R, int K, double* out, void* ws,
                               size_t ws_bytes, void* stream) {
  ABC_CHECK_ARG(R >= 1 && R <= (1ll << 31), "column_span: bad R");
  ABC_CHECK_ARG(K >= 1 && K <= SPAN_T, "column_span: K outside 1..%d", SPAN_T);
  ABC_CHECK_ARG(V && out, "column_span: null pointer");
  ColumnStatsWs w;
  ABC_CARVE(w, "column_span", R, K);
  hipStream_t s = as_stream(stream);
  const int rpb = SPAN_T / K;
  const int64_t want = ceil_div(R, rpb);
  const int nb = (int)(want < SPAN_BLOCKS ? want : SPAN_BLOCKS);
  hipLaunchKernelGGL(span_partial_kernel, dim3((unsigned)nb), dim3(SPAN_T), 0, s, V, R, K,
                     w.sd.part);
  ABC_LAUNCHED();
  hipLaunchKernelGGL(span_final_kernel, dim3(1), dim3(SPAN_T), 0, s, w.sd.part, nb, K, out);
  ABC_LAUNCHED();
  return ABC_OK;
}
