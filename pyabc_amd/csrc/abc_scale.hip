// Per-column scale functions of AdaptivePNormDistance over the recorded
// [R x S] row-major fp64 sum-stat matrix, with the observation x0[S] on the
// device.
//
// Reference: pyabc/distance/scale.py:38-135 (per key: data = one column,
// x_0 = the observed value o of that key)
//   MAD             median|x - median x|          abc_select.hip, two passes
//   STD             np.std                        abc_column_std
//   MAD_TO_OBS      median|x - o|                 abc_select.hip, one pass
//   CMAD            MAD + MAD_TO_OBS              abc_select.hip, three passes
//   MEAN_AD         mean|x - mean x|              sum x; sum |x - mean|
//   BIAS            |mean x - o|                  sum x
//   RMSD            sqrt(bias^2 + std^2)          sum x; sum (x - mean)^2
//   MEAN_AD_TO_OBS  mean|x - o|                   sum |x - o|
//   CMEAN_AD        MEAN_AD + MEAN_AD_TO_OBS      sum x and sum |x - o|; sum |x - mean|
//   STD_TO_OBS      np.std(|x - o|)               sum |x - o|; sum (|x - o| - mean)^2
//
// The mean family is one streaming kernel, colred_kernel<TOBS, A, B>: per
// column it accumulates up to two of {sum t, sum |t - c|, sum (t - c)^2}
// with t = x or |x - o| and a per-column centre c (the previous pass's mean,
// or o itself: sum |x - o| is the second form with c = o).  Every kind reads
// X at most twice, and the second pass is always centred (np.std's two-pass
// form; never E[x^2] - mean^2).
//
// Layout: a block covers CB = min(S, 256) columns x RPI = 256 / CB rows per
// load (thread t: column t % CB of row t / CB, so a block's load is one
// contiguous RPI * S element piece of X when S <= 256), U such pieces in
// flight, pieces dealt to blocks round-robin.
//
// Determinism: which elements a thread adds, and in which order, is fixed by
// (R, S) alone: U accumulators per thread added in index order, the RPI row
// slots of a column added in slot order through LDS, one partial per block
// and column stored to scratch, and the partials of the fixed grid added in
// a fixed order by colred_final.  No floating-point atomics; the result does
// not depend on which blocks run first.
#include "abc_column_ws.h"

namespace abc {
namespace {

constexpr int RD_T = 256;       // threads per block
constexpr int RD_U = 8;         // loads in flight per thread
constexpr int RD_BLOCKS = 512;  // row-piece blocks per column tile (fixed: the sum order)
constexpr int FIN_C = 16;       // colred_final: columns per block x RD_T / FIN_C slices

enum { OP_NONE, OP_SUM, OP_ABSC, OP_SQC };
enum { FIN_MEAN, FIN_MEAN_ADD, FIN_BIAS, FIN_STD, FIN_RMSD };

template <int OP>
__device__ __forceinline__ double red_term(double t, double c) {
  if (OP == OP_SUM) return t;
  const double d = t - c;
  return OP == OP_ABSC ? fabs(d) : d * d;
}

// the block's RPI row slots of each column, added in slot order
__device__ __forceinline__ void block_store(double* lds, double v, int CB, int RPI, int c, int S,
                                            double* __restrict__ dst) {
  const int t = threadIdx.x;
  lds[t] = v;
  __syncthreads();
  if (t < CB && c < S) {
    double s = lds[t];
    for (int k = 1; k < RPI; ++k) s += lds[t + k * CB];
    dst[c] = s;
  }
  __syncthreads();
}

// At most 4 waves per SIMD (the grid gives each SIMD 2): the two-sum form
// keeps 16 accumulators beside RD_U loads in flight, which the default
// 8-wave register budget (64 VGPRs) does not hold -- the compiler then waits
// for every load before it issues the next (0.61 ms per pass at c4 instead
// of 0.24).
template <bool TOBS, int A, int B>
__global__ __launch_bounds__(RD_T) __attribute__((amdgpu_waves_per_eu(1, 4))) void colred_kernel(
    const double* __restrict__ X, int64_t R, int S, const double* __restrict__ obs,
    const double* __restrict__ ctr, double* __restrict__ part) {
  __shared__ double lds[RD_T];
  constexpr bool CENTRED = (A != OP_SUM) || (B != OP_NONE && B != OP_SUM);
  const int t = threadIdx.x;
  const int CB = S < RD_T ? S : RD_T;
  const int RPI = RD_T / CB;
  const int cl = t % CB, rsub = t / CB;
  const int c = blockIdx.y * CB + cl;
  const bool active = rsub < RPI && c < S;
  double a[RD_U], b[RD_U];
#pragma unroll
  for (int u = 0; u < RD_U; ++u) a[u] = b[u] = 0.0;
  if (active) {
    const double o = TOBS ? obs[c] : 0.0;
    const double m = CENTRED ? ctr[c] : 0.0;
    const double* __restrict__ xc = X + c;
    const int64_t stride = (int64_t)RPI * gridDim.x;  // rows between a thread's loads
    int64_t r = (int64_t)blockIdx.x * RPI + rsub;
    for (; r + (RD_U - 1) * stride < R; r += RD_U * stride) {
      double v[RD_U];
#pragma unroll
      for (int u = 0; u < RD_U; ++u) v[u] = xc[(r + u * stride) * S];
#pragma unroll
      for (int u = 0; u < RD_U; ++u) {
        const double tv = TOBS ? fabs(v[u] - o) : v[u];
        a[u] += red_term<A>(tv, m);
        if (B != OP_NONE) b[u] += red_term<B>(tv, m);
      }
    }
#pragma unroll
    for (int u = 0; u < RD_U; ++u) {
      const int64_t rr = r + u * stride;
      if (rr < R) {
        const double x = xc[rr * S];
        const double tv = TOBS ? fabs(x - o) : x;
        a[u] += red_term<A>(tv, m);
        if (B != OP_NONE) b[u] += red_term<B>(tv, m);
      }
    }
  }
  double sa = 0.0, sb = 0.0;
#pragma unroll
  for (int u = 0; u < RD_U; ++u) { sa += a[u]; sb += b[u]; }
  block_store(lds, sa, CB, RPI, c, S, part + (int64_t)blockIdx.x * S);
  if (B != OP_NONE)
    block_store(lds, sb, CB, RPI, c, S, part + ((int64_t)gridDim.x + blockIdx.x) * S);
}

// out[c] from the nblk block partials of column c, added in a fixed order:
// slice sl adds blocks sl, sl + NSL, ...; the slices are added in slice order
__global__ __launch_bounds__(RD_T) void colred_final(
    const double* __restrict__ part, int nblk, int S, int64_t R, int fin,
    const double* __restrict__ obs, const double* __restrict__ mean, double* __restrict__ out) {
#pragma clang fp contract(off)
  constexpr int NSL = RD_T / FIN_C;
  __shared__ double lds[NSL][FIN_C];
  const int cl = threadIdx.x % FIN_C, sl = threadIdx.x / FIN_C;
  const int c = blockIdx.x * FIN_C + cl;
  double s = 0.0;
  if (c < S)
    for (int b = sl; b < nblk; b += NSL) s += part[(int64_t)b * S + c];
  lds[sl][cl] = s;
  __syncthreads();
  if (sl != 0 || c >= S) return;
  double tot = lds[0][cl];
  for (int k = 1; k < NSL; ++k) tot += lds[k][cl];
  const double v = tot / (double)R;
  double r = v;
  if (fin == FIN_MEAN_ADD) {
    r = v + out[c];
  } else if (fin == FIN_BIAS) {
    r = fabs(v - obs[c]);
  } else if (fin == FIN_STD) {
    r = sqrt(v);
  } else if (fin == FIN_RMSD) {
    const double bs = fabs(mean[c] - obs[c]), sd = sqrt(v);
    r = sqrt(bs * bs + sd * sd);
  }
  out[c] = r;
}

struct RedBufs {
  double* part;  // [2][RD_BLOCKS][S]
  double* mean;  // [S]
  void carve(Carver& cv, int S) {
    part = cv.take<double>((size_t)2 * RD_BLOCKS * S);
    mean = cv.take<double>((size_t)S);
  }
};

struct RedGrid {
  int CB, RPI, ctiles, nblk;
};
RedGrid red_grid(int64_t R, int S) {
  RedGrid g;
  g.CB = S < RD_T ? S : RD_T;
  g.RPI = RD_T / g.CB;
  g.ctiles = (int)ceil_div(S, g.CB);
  const int64_t pieces = ceil_div(R, g.RPI);
  g.nblk = (int)(pieces < RD_BLOCKS ? pieces : RD_BLOCKS);
  return g;
}

template <bool TOBS, int A, int B>
int red_pass(const double* X, int64_t R, int S, const double* obs, const double* ctr,
             double* part, hipStream_t s) {
  const RedGrid g = red_grid(R, S);
  hipLaunchKernelGGL((colred_kernel<TOBS, A, B>), dim3((unsigned)g.nblk, (unsigned)g.ctiles),
                     dim3(RD_T), 0, s, X, R, S, obs, ctr, part);
  ABC_LAUNCHED();
  return ABC_OK;
}

// plane 0 or 1 of the partials -> out
int red_final(const double* part, int plane, int64_t R, int S, int fin, const double* obs,
              const double* mean, double* out, hipStream_t s) {
  const RedGrid g = red_grid(R, S);
  hipLaunchKernelGGL(colred_final, dim3((unsigned)ceil_div(S, FIN_C)), dim3(RD_T), 0, s,
                     part + (size_t)plane * g.nblk * S, g.nblk, S, R, fin, obs, mean, out);
  ABC_LAUNCHED();
  return ABC_OK;
}

#define ABC_TRY(call) do { int rc_ = (call); if (rc_) return rc_; } while (0)

int column_mean_family(int kind, const double* X, int64_t R, int S, const double* x0, double* out,
                       const RedBufs& b, hipStream_t s) {
  const double* none = nullptr;
  switch (kind) {
    case ABC_SCALE_BIAS:
      ABC_TRY((red_pass<false, OP_SUM, OP_NONE>(X, R, S, none, none, b.part, s)));
      return red_final(b.part, 0, R, S, FIN_BIAS, x0, none, out, s);
    case ABC_SCALE_MEAN_AD_TO_OBS:
      ABC_TRY((red_pass<false, OP_ABSC, OP_NONE>(X, R, S, none, x0, b.part, s)));
      return red_final(b.part, 0, R, S, FIN_MEAN, none, none, out, s);
    case ABC_SCALE_MEAN_AD:
      ABC_TRY((red_pass<false, OP_SUM, OP_NONE>(X, R, S, none, none, b.part, s)));
      ABC_TRY(red_final(b.part, 0, R, S, FIN_MEAN, none, none, b.mean, s));
      ABC_TRY((red_pass<false, OP_ABSC, OP_NONE>(X, R, S, none, b.mean, b.part, s)));
      return red_final(b.part, 0, R, S, FIN_MEAN, none, none, out, s);
    case ABC_SCALE_RMSD:
      ABC_TRY((red_pass<false, OP_SUM, OP_NONE>(X, R, S, none, none, b.part, s)));
      ABC_TRY(red_final(b.part, 0, R, S, FIN_MEAN, none, none, b.mean, s));
      ABC_TRY((red_pass<false, OP_SQC, OP_NONE>(X, R, S, none, b.mean, b.part, s)));
      return red_final(b.part, 0, R, S, FIN_RMSD, x0, b.mean, out, s);
    case ABC_SCALE_CMEAN_AD:
      // sum x and sum |x - o| in one read; then sum |x - mean|
      ABC_TRY((red_pass<false, OP_SUM, OP_ABSC>(X, R, S, none, x0, b.part, s)));
      ABC_TRY(red_final(b.part, 0, R, S, FIN_MEAN, none, none, b.mean, s));
      ABC_TRY(red_final(b.part, 1, R, S, FIN_MEAN, none, none, out, s));
      ABC_TRY((red_pass<false, OP_ABSC, OP_NONE>(X, R, S, none, b.mean, b.part, s)));
      return red_final(b.part, 0, R, S, FIN_MEAN_ADD, none, none, out, s);
    case ABC_SCALE_STD_TO_OBS:
      ABC_TRY((red_pass<false, OP_ABSC, OP_NONE>(X, R, S, none, x0, b.part, s)));
      ABC_TRY(red_final(b.part, 0, R, S, FIN_MEAN, none, none, b.mean, s));
      ABC_TRY((red_pass<true, OP_SQC, OP_NONE>(X, R, S, x0, b.mean, b.part, s)));
      return red_final(b.part, 0, R, S, FIN_STD, none, none, out, s);
  }
  return set_error(ABC_ERR_INVALID, "column_scale: unknown kind %d", kind);
}

bool scale_kind_known(int kind) { return kind >= ABC_SCALE_MAD && kind <= ABC_SCALE_STD_TO_OBS; }
bool scale_kind_reads_x0(int kind) {
  return kind != ABC_SCALE_MAD && kind != ABC_SCALE_MEAN_AD && kind != ABC_SCALE_STD;
}

// abc_column_scale's layout: that of the kind's kernels
struct ScaleWs {
  ColumnStatsWs stats; SelectBufs sel; CmadBufs cmad; RedBufs red;
  void carve(Carver& cv, int kind, int64_t R, int S) {
    switch (kind) {
      case ABC_SCALE_MAD:
      case ABC_SCALE_STD: stats.carve(cv, R, S); break;
      case ABC_SCALE_MAD_TO_OBS: sel.carve(cv, R, S); break;
      case ABC_SCALE_CMAD: cmad.carve(cv, R, S); break;
      default: red.carve(cv, S);
    }
  }
};

}  // namespace
}  // namespace abc

using namespace abc;

extern "C" size_t abc_column_scale_workspace(int kind, int64_t R, int S) {
  if (!scale_kind_known(kind) || R < 1 || S < 1) return 0;
  return measure<ScaleWs>(kind, R, S);
}

extern "C" int abc_column_scale(int kind, const double* X, int64_t R, int S, const double* x0,
                                double* out, void* ws, size_t ws_bytes, void* stream) {
  ABC_CHECK_ARG(scale_kind_known(kind), "column_scale: unknown kind %d", kind);
  ABC_CHECK_ARG(R >= 1 && S >= 1, "column_scale: bad R/S");
  ABC_CHECK_ARG(X && out && ws, "column_scale: null pointer");
  ABC_CHECK_ARG(x0 || !scale_kind_reads_x0(kind), "column_scale: kind %d needs x0", kind);
  ScaleWs w;
  ABC_CARVE(w, "column_scale", kind, R, S);
  hipStream_t s = as_stream(stream);
  switch (kind) {
    case ABC_SCALE_MAD:  // the same calls as abc_column_mad / abc_column_std, the same bits
      return column_mad_select(X, R, S, out, w.stats.sel, s);
    case ABC_SCALE_STD:
      return column_std(X, R, S, out, w.stats.sd, s);
    case ABC_SCALE_MAD_TO_OBS:
      return column_absdev_median_select(X, R, S, x0, out, w.sel, s);
    case ABC_SCALE_CMAD:
      return column_cmad_select(X, R, S, x0, out, w.cmad, s);
    default:
      return column_mean_family(kind, X, R, S, x0, out, w.red, s);
  }
}
