// One Gaussian KDE at G covariance scalings in one pass (GridSearchCV over
// MultivariateNormalTransition.scaling).
//
// Reference: pyabc/transition/model_selection.py:9-74 runs sklearn's grid
// search, whose default grid varies only `scaling`, and scaling multiplies
// the covariance (multivariatenormal.py:82).  All grid points of a fold then
// share one whitening U (U U^T = Sigma_1^-1 at scaling 1) and differ in the
// exponent's scale alone:
//
//   out[g][i] = log sum_j w_j exp(-|(x_i - X_j) U|^2 / (2 s_g)) + log_const[g]
//
// The arithmetic follows mvn_lse_kernel<double> (abc_mvn.hip): the cross term
// on v_mfma_f64_16x16x4_f64, population rows the A operand and points the B
// operand (a lane owns one point and four rows of every 16x16 tile), operand
// images packed once per call, (m, l) partials per population chunk and a
// combine.  The weight cannot ride in the GEMM here (the quadratic form is
// scaled per g, log2 w_j is not), so
//
//   A = [y_j, -log2e |y_j|^2 / 2],  B = [log2e z_i, 1],  C = -log2e |z_i|^2 / 2
//
// and the MFMA emits a_ij = -log2e |z_i - y_j|^2 / 2 (<= 0 up to rounding),
// once for all g.  Per g the exponent is a_ij / s_g + log2 w_j - m_g[i] in
// fp64, rounded to f32 for v_exp_f32, summed in fp64.  m_g is a running
// reference per (point, g): it moves (per lane, plain VALU -- a_ij does not
// depend on it) when a tile's largest exponent exceeds 2 or when nothing
// has been accumulated and the largest is below -2, so every sum is
// dominated by terms whose f32 exponent has |d| <= 4 (half an ulp 1.2e-7
// there; a term 2^-k below the largest weighs 2^-k in the sum).  A held-out
// point many kernel widths from every train row is then finite wherever the
// fp64 value is.
#include "abc_density.h"

namespace abc {
namespace {

constexpr float THR_HI = 2.f;     // move m_g if an exponent exceeds this (log2)
constexpr float THR_LO = -2.f;    // ... or if nothing accumulated and below
// ln 2^-1075: below it every term w_j pdf_j of the reference's fp64 sum has
// rounded to zero and np.log gives -inf
constexpr double LOG_F64_UNDERFLOW = -745.13321910194110842;
constexpr int GCAP = 8;           // grid points per launch (registers, below)
constexpr int CT = 2;             // 16-point tiles per wave
constexpr int GMAX = 64;

typedef double f64x4 __attribute__((ext_vector_type(4)));

struct Scales { double inv[GCAP]; };
struct Consts { double c[GMAX]; };

// A image (operand_at); column r holds -log2e |y|^2 / 2.  lw[t][lane >> 4][v]
// = log2 w of row 16t + (lane >> 4) + 4v, the row of the f64 MFMA's result v
// in that lane (-inf for w = 0 and for the padding rows).
__global__ void scaled_pack_population(const double* __restrict__ X,
                                       const double* __restrict__ w, int64_t N,
                                       int d, const double* __restrict__ mu,
                                       const double* __restrict__ U, int r,
                                       int KB, double* __restrict__ packed,
                                       double* __restrict__ lw, int64_t NT) {
  const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= NT * 16) return;
  const int K = 4 * KB;
  double yv[64];
  double aug = 0.0, l2w = -INFINITY;
  for (int k = 0; k < r; ++k) yv[k] = 0.0;
  if (row < N) {
    double y2 = 0.0;
    for (int k = 0; k < r; ++k) {
      const double acc = whiten_row(X + row * d, mu, U, d, r, k);
      yv[k] = acc;
      y2 += acc * acc;
    }
    aug = -0.5 * LOG2E * y2;
    const double wj = w[row];
    if (wj > 0.0) l2w = log2(wj);
  }
  const int64_t t = row >> 4;
  const int rl = (int)(row & 15);
  for (int k = 0; k < K; ++k)
    packed[operand_at(t, rl, k, KB)] = (k < r) ? yv[k] : (k == r ? aug : 0.0);
  lw[t * 16 + (rl & 3) * 4 + (rl >> 2)] = l2w;
}

// B image of the points and z0 = -|u|^2 log2e / 2 of the point u = b / log2e
// the operand represents (the accumulator's start)
__global__ void scaled_pack_points(const double* __restrict__ x, int64_t M, int d,
                                   const double* __restrict__ mu,
                                   const double* __restrict__ U, int r, int KB,
                                   double* __restrict__ packed,
                                   double* __restrict__ z0, int64_t MT) {
  const int64_t col = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (col >= MT * 16) return;
  const int K = 4 * KB;
  double bv[64];
  double b2 = 0.0;
  for (int k = 0; k < r; ++k) bv[k] = 0.0;
  if (col < M) {
    for (int k = 0; k < r; ++k) {
      const double bt = whiten_row(x + col * d, mu, U, d, r, k) * LOG2E;
      bv[k] = bt;
      b2 += bt * bt;
    }
  }
  z0[col] = -0.5 * b2 / LOG2E;
  for (int k = 0; k < K; ++k)
    packed[operand_at(col >> 4, (int)(col & 15), k, KB)] =
        (k < r) ? bv[k] : (k == r ? 1.0 : 0.0);
}

// One wave = CT point tiles x one population chunk x GT grid points; block =
// 4 waves.  Registers (doubles per lane): b CT KB, a and its prefetch 2 KB,
// (m, l) 2 CT GT, the tile's log2 w 8.  Compiled: 164 VGPRs at KB = 3,
// GT = 5, 256 + 78 AGPRs at KB = 15, GT = 8 (one wave per SIMD), no scratch.  Partials: part[g][chunk][Mpad].
template <int KB, int GT>
__global__ __launch_bounds__(256) void mvn_scaled_kernel(
    const double* __restrict__ A, const double* __restrict__ lw,
    const double* __restrict__ Bp, const double* __restrict__ z0, int64_t MT,
    int64_t NT, int nchunk, int64_t tiles_per_chunk, Scales sc, int greal,
    double* __restrict__ part_m, double* __restrict__ part_l, int64_t Mpad) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int chunk = (int)(blockIdx.x % (unsigned)nchunk);
  const int64_t group = blockIdx.x / (unsigned)nchunk;
  const int64_t ct0 = (group * 4 + wave) * CT;

  double b[CT][KB];
  double zc[CT];
  double m[CT][GT], l[CT][GT];
#pragma unroll
  for (int c = 0; c < CT; ++c) {
    const int64_t ct = ct0 + c;
    const bool live = ct < MT;
#pragma unroll
    for (int kb = 0; kb < KB; ++kb)
      b[c][kb] = live ? Bp[operand_lane_at(ct, lane, kb, KB)] : 0.0;
    zc[c] = live ? z0[ct * 16 + (lane & 15)] : 0.0;
#pragma unroll
    for (int g = 0; g < GT; ++g) { m[c][g] = 0.0; l[c][g] = 0.0; }
  }

  const int64_t t_begin = (int64_t)chunk * tiles_per_chunk;
  const int64_t t_end = t_begin + tiles_per_chunk < NT ? t_begin + tiles_per_chunk : NT;

  double a[KB], an[KB];
  double wl[4], wn[4];
  if (t_begin < t_end) {
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) a[kb] = A[operand_lane_at(t_begin, lane, kb, KB)];
#pragma unroll
    for (int v = 0; v < 4; ++v) wl[v] = lw[t_begin * 16 + (lane >> 4) * 4 + v];
  }
  for (int64_t t = t_begin; t < t_end; ++t) {
    const int64_t tn = (t + 1 < t_end) ? t + 1 : t;
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) an[kb] = A[operand_lane_at(tn, lane, kb, KB)];
#pragma unroll
    for (int v = 0; v < 4; ++v) wn[v] = lw[tn * 16 + (lane >> 4) * 4 + v];
#pragma unroll
    for (int c = 0; c < CT; ++c) {
      f64x4 acc = {zc[c], zc[c], zc[c], zc[c]};
#pragma unroll
      for (int kb = 0; kb < KB; ++kb)
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[kb], b[c][kb], acc, 0, 0, 0);
#pragma unroll
      for (int g = 0; g < GT; ++g) {
        const double s = sc.inv[g];
        double e0 = __builtin_fma(acc[0], s, wl[0]) - m[c][g];
        double e1 = __builtin_fma(acc[1], s, wl[1]) - m[c][g];
        double e2 = __builtin_fma(acc[2], s, wl[2]) - m[c][g];
        double e3 = __builtin_fma(acc[3], s, wl[3]) - m[c][g];
        float d0 = (float)e0, d1 = (float)e1, d2 = (float)e2, d3 = (float)e3;
        const float tmax = fmaxf(fmaxf(d0, d1), fmaxf(d2, d3));
        const bool need = (tmax > THR_HI) ||
                          (l[c][g] == 0.0 && tmax < THR_LO && tmax > -INFINITY);
        if (__builtin_expect(need, 0)) {
          // nothing accumulated yet: only m moves (0 * exp2(huge) is NaN)
          const double sh = (double)tmax;
          if (l[c][g] > 0.0) l[c][g] *= exp2(-sh);
          m[c][g] += sh;
          d0 = (float)(e0 - sh); d1 = (float)(e1 - sh);
          d2 = (float)(e2 - sh); d3 = (float)(e3 - sh);
        }
        const float e = (__builtin_amdgcn_exp2f(d0) + __builtin_amdgcn_exp2f(d1)) +
                        (__builtin_amdgcn_exp2f(d2) + __builtin_amdgcn_exp2f(d3));
        l[c][g] += (double)e;
      }
    }
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) a[kb] = an[kb];
#pragma unroll
    for (int v = 0; v < 4; ++v) wl[v] = wn[v];
  }

  // Combine the four lane groups (lanes l, l^16, l^32, l^48 hold the same
  // point) and store one (m, l) partial per point, chunk and grid point.
#pragma unroll
  for (int c = 0; c < CT; ++c) {
#pragma unroll
    for (int g = 0; g < GT; ++g) {
      double mm = m[c][g], ll = l[c][g];
#pragma unroll
      for (int o = 16; o < 64; o <<= 1) {
        const double mo = __shfl_xor(mm, o, 64), lo = __shfl_xor(ll, o, 64);
        lse_merge_live<Base2>(mm, ll, mo, lo);
      }
      const int64_t ct = ct0 + c;
      if (lane < 16 && ct < MT && g < greal) {
        const int64_t at = ((int64_t)g * nchunk + chunk) * Mpad + ct * 16 + lane;
        part_m[at] = mm;
        part_l[at] = ll;
      }
    }
  }
}

// out[g][i] over grid (ceil(M / 256), G)
__global__ void scaled_combine_kernel(const double* __restrict__ part_m,
                                      const double* __restrict__ part_l,
                                      int nchunk, int64_t M, int64_t Mpad,
                                      Consts lc, double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int g = blockIdx.y;
  if (i >= M) return;
  const int64_t at = (int64_t)g * nchunk * Mpad;
  const LsePair p = lse_combine<Base2>(part_m + at, part_l + at, Mpad, nchunk, i);
  double v = -INFINITY;
  if (p.m > -INFINITY) {
    v = LN2 * (p.m + log2(p.l)) + lc.c[g];
    if (v < LOG_F64_UNDERFLOW) v = -INFINITY;
  }
  out[(int64_t)g * M + i] = v;
}

// score[g] = sum_i wt[i] out[g][i]: one block per g, each thread its strided
// rows in order, then a fixed tree in LDS (the same bits every run).  The
// product is plain IEEE: 0 * -inf is NaN, as (np.log(dens) * w).sum() has it.
__global__ __launch_bounds__(256) void scaled_score_kernel(
    const double* __restrict__ out, const double* __restrict__ wt, int64_t M,
    double* __restrict__ score) {
  __shared__ double sh[256];
  const int g = blockIdx.x;
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < M; i += 256) s += wt[i] * out[(int64_t)g * M + i];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) score[g] = sh[0];
}

// K blocks the kernel is instantiated for (r + 1 columns padded up with zero
// columns to the next entry) and grid points per launch (padded up by
// repeating the last scaling; the padding's partials are not stored)
using ScaledKBs = std::integer_sequence<int, 1, 2, 3, 4, 6, 8, 11, 15>;
using ScaledGTs = std::integer_sequence<int, 1, 2, 3, 4, 5, 8>;

int round_up_to(const int* list, int n, int v) {
  for (int i = 0; i < n; ++i)
    if (list[i] >= v) return list[i];
  return -1;
}
int scaled_kb(int r) {
  static const int kbs[] = {1, 2, 3, 4, 6, 8, 11, 15};
  return round_up_to(kbs, 8, (int)ceil_div(r + 1, 4));
}
int scaled_gt(int g) {
  static const int gts[] = {1, 2, 3, 4, 5, 8};
  return round_up_to(gts, 6, g);
}

// The decomposition depends on (M, N, r) only, never on G: a grid point's
// result is the same bits whichever launch carries it.
struct SPlan : TilePlan {
  int KB, nchunk, G;
  int64_t tiles_per_chunk;
};

SPlan make_splan(int64_t M, int64_t N, int r, int G) {
  SPlan p;
  static_cast<TilePlan&>(p) = tile_plan(M, N, CT);
  p.KB = scaled_kb(r);
  p.G = G;
  p.tiles_per_chunk = ceil_div(p.NT, p.nc);
  p.nchunk = (int)ceil_div(p.NT, p.tiles_per_chunk);   // no empty chunk
  return p;
}

struct SPlanWs {
  double *A, *lw, *Bp, *z0, *pm, *pl;
  void carve(Carver& cv, const SPlan& p) {
    A = cv.take<double>((size_t)p.NT * 64 * p.KB);
    lw = cv.take<double>((size_t)p.NT * 16);
    Bp = cv.take<double>((size_t)p.MTpad * 64 * p.KB);
    z0 = cv.take<double>((size_t)p.Mpad);
    pm = cv.take<double>((size_t)p.G * p.nchunk * p.Mpad);
    pl = cv.take<double>((size_t)p.G * p.nchunk * p.Mpad);
  }
};

template <int KB, int GT>
void launch_scaled(const SPlan& p, const SPlanWs& k, const Scales& sc, int greal,
                   int g0, hipStream_t s) {
  const int64_t off = (int64_t)g0 * p.nchunk * p.Mpad;
  hipLaunchKernelGGL((mvn_scaled_kernel<KB, GT>), dim3((unsigned)(p.groups * p.nchunk)),
                     dim3(256), 0, s, k.A, k.lw, k.Bp, k.z0, p.MT, p.NT, p.nchunk,
                     p.tiles_per_chunk, sc, greal, k.pm + off, k.pl + off, p.Mpad);
}

}  // namespace
}  // namespace abc

using namespace abc;

static bool scaled_shape_ok(int64_t M, int64_t N, int r, int G) {
  return M >= 0 && N >= 1 && r >= 1 && r <= 59 && G >= 1 && G <= GMAX;
}

extern "C" size_t abc_mvn_logpdf_scaled_bytes(int64_t M, int64_t N, int r, int G) {
  if (!scaled_shape_ok(M, N, r, G)) return 0;
  return measure<SPlanWs>(make_splan(M, N, r, G));
}

extern "C" int abc_mvn_logpdf_scaled(const double* x, int64_t M, int d,
                                     const double* X, const double* w, int64_t N,
                                     const double* mu, const double* U, int r,
                                     const double* inv_scaling, int G,
                                     const double* log_const, double* out,
                                     const double* wt, double* score, void* ws,
                                     size_t ws_bytes, void* stream) {
  ABC_CHECK_ARG(G >= 1 && G <= GMAX, "logpdf_scaled: G=%d outside [1, %d]", G, GMAX);
  ABC_CHECK_ARG(r == d, "logpdf_scaled: rank r=%d is not d=%d (full rank only)", r, d);
  ABC_CHECK_ARG(r >= 1 && r <= 59, "logpdf_scaled: rank r=%d outside [1, 59]", r);
  ABC_CHECK_ARG(M >= 0 && N >= 1, "logpdf_scaled: bad M/N");
  ABC_CHECK_ARG(inv_scaling && log_const, "logpdf_scaled: null scaling arrays");
  ABC_CHECK_ARG(wt || !score, "logpdf_scaled: score without test weights wt");
  ABC_CHECK_ARG(M == 0 || (x && X && w && mu && U && out), "logpdf_scaled: null pointer");
  for (int g = 0; g < G; ++g)
    ABC_CHECK_ARG(inv_scaling[g] > 0.0 && inv_scaling[g] < INFINITY,
                  "logpdf_scaled: inv_scaling[%d] is not positive and finite", g);
  const SPlan p = make_splan(M, N, r, G);
  ABC_CHECK_ARG(ws_bytes >= measure<SPlanWs>(p) && (ws || M == 0),
                "logpdf_scaled: workspace too small (%zu bytes)", ws_bytes);
  hipStream_t s = as_stream(stream);
  if (M == 0) {
    if (score) ABC_HIP(hipMemsetAsync(score, 0, sizeof(double) * G, s));
    return ABC_OK;
  }
  SPlanWs k;
  ABC_CARVE(k, "logpdf_scaled", p);
  hipLaunchKernelGGL(scaled_pack_population, dim3((unsigned)ceil_div(p.NT * 16, 128)),
                     dim3(128), 0, s, X, w, N, d, mu, U, r, p.KB, k.A, k.lw, p.NT);
  ABC_LAUNCHED();
  hipLaunchKernelGGL(scaled_pack_points, dim3((unsigned)ceil_div(p.MTpad * 16, 128)),
                     dim3(128), 0, s, x, M, d, mu, U, r, p.KB, k.Bp, k.z0, p.MTpad);
  ABC_LAUNCHED();
  Consts lc;
  for (int g = 0; g < GMAX; ++g) lc.c[g] = g < G ? log_const[g] : 0.0;
  for (int g0 = 0; g0 < G; g0 += GCAP) {
    const int greal = G - g0 < GCAP ? G - g0 : GCAP;
    const int GTv = scaled_gt(greal);
    Scales sc;
    for (int g = 0; g < GCAP; ++g)
      sc.inv[g] = inv_scaling[g0 + (g < greal ? g : greal - 1)];
    const bool ok = dispatch_int(ScaledKBs{}, p.KB, [&](auto KB) {
      dispatch_int(ScaledGTs{}, GTv, [&](auto GT) {
        launch_scaled<decltype(KB)::value, decltype(GT)::value>(p, k, sc, greal, g0, s);
      });
    });
    if (!ok) return set_error(ABC_ERR_UNSUPPORTED, "logpdf_scaled: r=%d too large", r);
    ABC_LAUNCHED();
  }
  hipLaunchKernelGGL(scaled_combine_kernel, dim3((unsigned)ceil_div(M, 256), (unsigned)G),
                     dim3(256), 0, s, k.pm, k.pl, p.nchunk, M, p.Mpad, lc, out);
  ABC_LAUNCHED();
  if (score) {
    hipLaunchKernelGGL(scaled_score_kernel, dim3((unsigned)G), dim3(256), 0, s, out, wt,
                       M, score);
    ABC_LAUNCHED();
  }
  return ABC_OK;
}
