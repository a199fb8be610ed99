// AggregatedDistance on stored rows: K PNormDistance terms read from the same
// row and their weighted sum.
//
// Reference: AggregatedDistance.__call__ (pyabc/distance/distance.py:434-461):
//   values = [distance(x, x_0, t) for distance in self.distances]
//   return np.dot(weights * factors, values)
// with every child a PNormDistance (distance.py:79-105).  Term k of row b is
// bit for bit what abc_pnorm writes for (wf + k S, p[k]): the narrow path
// calls pnorm_row itself; the wide path repeats pnorm_wave_rows' operations
// in its order (lane-strided partials over k, then the wave tree, then
// pnorm_finish) for up to AGG_TG terms per loaded value, through pterm,
// wave_sum / wave_pnorm_max and pnorm_finish<0> of abc_candidate.h.  Contraction is
// off, so no kernel fuses differently from another.
//
// The wide path keeps pnorm_wave_rows' PNORM_ROWS rows in flight per wave and
// AGG_TG accumulators per row (PNORM_ROWS x AGG_TG doubles = 64 VGPRs); a
// stack of K > AGG_TG terms takes ceil(K / AGG_TG) passes over the wave's
// rows, the later ones served by L2 (8 rows x S doubles per wave, read again
// by the wave that just read them).
#pragma once
#include "abc_candidate.h"

#pragma clang fp contract(off)

namespace abc {

constexpr int AGG_TG = 4;   // terms per pass of the wide path

// the term stack's host-side scalars, passed by value (wave-uniform reads)
struct AggTerms {
  double p[ABC_AGG_MAX_TERMS];
  double c[ABC_AGG_MAX_TERMS];
  int K;
};

// every p in {1, 2, inf}: the kernels instantiated without pow
inline bool agg_simple(const double* p, int K) {
  for (int k = 0; k < K; ++k)
    if (!(p[k] == 1.0 || p[k] == 2.0 || isinf(p[k]))) return false;
  return true;
}

// pnorm_finish<0> without pow when SIMPLE (the same operations as its p in
// {1, 2, inf} branches), else itself
template <bool SIMPLE>
__device__ __forceinline__ double agg_finish(double s, double p) {
#pragma clang fp contract(off)
  if constexpr (SIMPLE) return (isinf(p) || p == 1.0) ? s : sqrt(s);
  return pnorm_finish<0>(s, p);
}

// d = ((0 + c_0 t_0) + c_1 t_1) + ...: one more term
__device__ __forceinline__ double agg_combine(double d, double c, double t) {
#pragma clang fp contract(off)
  return d + c * t;
}

// Narrow rows (S <= 32): the K terms of one row by pnorm_row, in k order.
// term(k, t_k) is called per term; returns d.
template <class F>
__device__ __forceinline__ double agg_row(const double* xr, int S, const double* x0,
                                          const double* wf, const AggTerms& T, F&& term) {
  double d = 0.0;
  for (int k = 0; k < T.K; ++k) {
    const double t = pnorm_row(xr, S, x0, wf + (int64_t)k * S, T.p[k]);
    term(k, t);
    d = agg_combine(d, T.c[k], t);
  }
  return d;
}

// Wide rows: rows b0 .. b0 + PNORM_ROWS - 1 of x [B x S] by one wave (every
// lane calls it).  Lane 0 calls term(r, k, t) per row and term and then
// emit(r, d) per row (rows < B only).
template <bool SIMPLE, class FT, class FD>
__device__ __forceinline__ void agg_wave_rows(const double* x, int64_t b0, int64_t B, int S,
                                              const double* x0, const double* wf,
                                              const AggTerms& T, FT&& term, FD&& emit) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  // b0 is the same in every lane: as scalars, the row bases are too and the
  // loads of an iteration share one lane offset
  b0 = ((int64_t)__builtin_amdgcn_readfirstlane((int)(b0 >> 32)) << 32) |
       (uint32_t)__builtin_amdgcn_readfirstlane((int)b0);
  double dacc[PNORM_ROWS];
#pragma unroll
  for (int r = 0; r < PNORM_ROWS; ++r) dacc[r] = 0.0;
#pragma unroll 1
  for (int k0 = 0; k0 < T.K; k0 += AGG_TG) {
    const int nt = T.K - k0 < AGG_TG ? T.K - k0 : AGG_TG;
    double pt[AGG_TG];
    bool inf[AGG_TG];
#pragma unroll
    for (int t = 0; t < AGG_TG; ++t) {
      pt[t] = T.p[k0 + (t < nt ? t : 0)];
      inf[t] = isinf(pt[t]);
    }
    double s[PNORM_ROWS][AGG_TG];
#pragma unroll
    for (int r = 0; r < PNORM_ROWS; ++r)
#pragma unroll
      for (int t = 0; t < AGG_TG; ++t) s[r][t] = 0.0;
    // every load of an iteration is unconditional (one wait for all of
    // them): rows past B read row B - 1 and terms past nt term nt - 1; neither
    // is emitted
    const double* wg[AGG_TG];
#pragma unroll
    for (int t = 0; t < AGG_TG; ++t) wg[t] = wf + (int64_t)(k0 + (t < nt ? t : nt - 1)) * S;
    const double* xr[PNORM_ROWS];
#pragma unroll
    for (int r = 0; r < PNORM_ROWS; ++r) xr[r] = x + (b0 + r < B ? b0 + r : B - 1) * S;
#pragma unroll 1
    for (int k = lane; k < S; k += 64) {
      const double ck = x0[k];
      double v[PNORM_ROWS], wk[AGG_TG];
#pragma unroll
      for (int r = 0; r < PNORM_ROWS; ++r) v[r] = xr[r][k];
#pragma unroll
      for (int t = 0; t < AGG_TG; ++t) wk[t] = wg[t][k];
#pragma unroll
      for (int r = 0; r < PNORM_ROWS; ++r) v[r] = v[r] - ck;
      // pterm's cases as wave-uniform branches around the PNORM_ROWS rows
#pragma unroll
      for (int t = 0; t < AGG_TG; ++t) {
        if (t < nt) {
          double a[PNORM_ROWS];
#pragma unroll
          for (int r = 0; r < PNORM_ROWS; ++r) a[r] = fabs(wk[t] * v[r]);
          if (inf[t]) {
#pragma unroll
            for (int r = 0; r < PNORM_ROWS; ++r) s[r][t] = pnorm_max(s[r][t], a[r]);
          } else if (pt[t] == 1.0) {
#pragma unroll
            for (int r = 0; r < PNORM_ROWS; ++r) s[r][t] = s[r][t] + a[r];
          } else if (SIMPLE || pt[t] == 2.0) {
#pragma unroll
            for (int r = 0; r < PNORM_ROWS; ++r) s[r][t] = s[r][t] + a[r] * a[r];
          } else {
#pragma unroll
            for (int r = 0; r < PNORM_ROWS; ++r) s[r][t] = s[r][t] + pow(a[r], pt[t]);
          }
        }
      }
    }
#pragma unroll
    for (int t = 0; t < AGG_TG; ++t) {
      if (t < nt) {
#pragma unroll
        for (int r = 0; r < PNORM_ROWS; ++r) {
          const double w = inf[t] ? wave_pnorm_max(s[r][t]) : wave_sum(s[r][t]);
          if (lane == 0 && b0 + r < B) {
            const double tv = agg_finish<SIMPLE>(w, pt[t]);
            term(r, k0 + t, tv);
            dacc[r] = agg_combine(dacc[r], T.c[k0 + t], tv);
          }
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < PNORM_ROWS; ++r)
    if (lane == 0 && b0 + r < B) emit(r, dacc[r]);
}

// the checks every aggregate entry shares (host; before any device call)
inline int agg_check_terms(const char* entry, int S, const double* p, const double* c, int K,
                           AggTerms& T) {
  ABC_CHECK_ARG(S >= 1, "%s: S < 1", entry);
  ABC_CHECK_ARG(K >= 1 && K <= ABC_AGG_MAX_TERMS, "%s: K outside 1..%d", entry,
                ABC_AGG_MAX_TERMS);
  ABC_CHECK_ARG(p && c, "%s: null pointer", entry);
  for (int k = 0; k < K; ++k) ABC_CHECK_ARG(p[k] >= 1.0, "%s: p < 1", entry);
  T.K = K;
  for (int k = 0; k < ABC_AGG_MAX_TERMS; ++k) {
    T.p[k] = k < K ? p[k] : 1.0;
    T.c[k] = k < K ? c[k] : 0.0;
  }
  return ABC_OK;
}

}  // namespace abc
