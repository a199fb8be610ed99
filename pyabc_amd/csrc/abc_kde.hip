// Marginal Gaussian KDEs of one population on their plot grids, all panels of
// a KDE matrix in one launch sequence.
//
// Reference: pyabc/visualization/kde.py:19-74 (kde_1d) and :174-248 (kde_2d)
// fit a MultivariateNormalTransition to one or two columns and evaluate its
// pdf (transition/multivariatenormal.py:99-113) on a linspace / meshgrid grid,
// one panel at a time: at d = 10 and 50 x 50 grids, 113 000 grid points
// against every particle.  Every panel shares the population, the weights and
// the effective sample size, and every panel's covariance is a sub-block of
// one d x d covariance, so the host plans all panels from one moments pass and
// this file evaluates them together:
//
//   z_j = (X_j[cols] - c) U',  z_g = (g - c) U',  U' = U sqrt(log2e / 2)
//   out_g = ln2 log2 sum_j 2^(log2 w_j - |z_g - z_j|^2) + log_const
//
// Plan.  A tile is 512 consecutive grid points of one panel (tiles never span
// panels; the last tile of a panel is masked).  The population is cut into
// nchunk chunks of whole 256-row stages.  Block (tile, chunk): thread t owns
// points t and t + 256 of the tile in registers (whitened coordinates and an
// (m, l) pair each); per stage the block whitens 256 rows for its panel --
// X is read row-wise, the panel's one or two columns of each row, no gathered
// copy -- into LDS as (z0, z1, log2 w), and every lane then reads the rows
// from the same address (broadcast).  The partial pairs go to
// part[chunk][point]; kde_finish_kernel combines a point's chunks in ascending
// order (lse_combine).  Rows are summed in ascending order within a chunk, so
// the order of every sum is a function of the shapes alone.
//
// Arithmetic.  Differences are taken after centring, in fp64, as are the
// quadratic form and the exponent t = s - m against the point's running
// reference m.  2^t is ldexp(exp2f(frac), int) with t split in fp64, so the
// fp32 exp2 sees an argument in [-1/2, 1/2] and its error does not grow with
// |t| (mvn_lse_kernel<double> converts t itself).  The first row of a chunk
// sets m, and m moves (lse_add) when a term exceeds it by more than 2; between
// moves the terms are added to l in fp64, l >= 1.  Terms 2^-126 below the
// reference are dropped (fp32 range), each below the last bit of l.  Since m
// follows the terms, a sum never underflows: far from the population the log
// density is a large negative number, and -inf only where no row has weight.
#include <vector>
#include "abc_density.h"

namespace abc {
namespace {

constexpr int KDE_THREADS = 256;
constexpr int KDE_GP = 2;                          // grid points per thread
constexpr int KDE_TILE = KDE_THREADS * KDE_GP;     // grid points per tile
constexpr int KDE_STAGE = 256;                     // rows whitened per stage
constexpr int64_t KDE_PART_BUDGET = (int64_t)1 << 22;   // partial pairs kept
constexpr double KDE_T_HI = 2.0;         // a term this far above m moves m
// log2 w of a row of weight 0: finite, so that no difference is inf - inf, and
// so far down that 2^(it - anything) is 0; a sum that holds nothing else ends
// with its reference here and is reported as -inf
constexpr double KDE_LW_ZERO = -1e300;

struct KdePanelDev {
  int col0, col1, nx, ny;
  int64_t ax, ay, out;
  double cx, cy;
  double u00, u01, u10, u11;   // U sqrt(log2e / 2)
  double log_const;
};
struct KdeTile { int panel; int start; };

// 2^t for finite t <= KDE_T_HI: the fraction through the fp32 exp2.  Below
// 2^-149 the result is 0 (KDE_LW_ZERO too: its fraction is 0); NaN stays NaN.
__device__ __forceinline__ double exp2_split(double t) {
  const double ti = __builtin_rint(t);
  const float e = __builtin_amdgcn_exp2f((float)(t - ti));
  return (double)__builtin_ldexpf(e, (int)fmax(ti, -1100.0));
}

// One term 2^s onto the pair (m, l), which starts at (-inf, 0): the first term
// sets the reference, so l >= 1 from then on and a term dropped by the fp32
// range is below 2^-126 of the sum.  s is finite or NaN (never -inf: a row of
// weight 0 carries KDE_LW_ZERO).
__device__ __forceinline__ void kde_term(double s, double& m, double& l) {
  const double t = s - m;
  if (__builtin_expect(t > KDE_T_HI, 0)) lse_add<Base2>(s, m, l);
  else l += exp2_split(t);
}

template <int DIM>
__device__ __forceinline__ void kde_rows(const double* __restrict__ sh, int rows,
                                         const double (&g0)[KDE_GP],
                                         const double (&g1)[KDE_GP],
                                         double (&m)[KDE_GP], double (&l)[KDE_GP]) {
#pragma unroll 4
  for (int r = 0; r < rows; ++r) {
    const double z0 = sh[4 * r], z1 = sh[4 * r + 1], lw = sh[4 * r + 2];
#pragma unroll
    for (int k = 0; k < KDE_GP; ++k) {
      const double d0 = g0[k] - z0;
      double q = d0 * d0;
      if (DIM == 2) {
        const double d1 = g1[k] - z1;
        q = __builtin_fma(d1, d1, q);
      }
      kde_term(lw - q, m[k], l[k]);
    }
  }
}

__global__ __launch_bounds__(KDE_THREADS) void kde_panels_kernel(
    const double* __restrict__ X, const double* __restrict__ w, int64_t N, int d,
    const KdePanelDev* __restrict__ panels, const KdeTile* __restrict__ tiles,
    const double* __restrict__ coords, int64_t chunk_rows, int64_t G_total,
    double* __restrict__ part_m, double* __restrict__ part_l) {
  __shared__ double sh[4 * KDE_STAGE];       // (z0, z1, log2 w, -) per row
  const KdeTile tl = tiles[blockIdx.x];
  const KdePanelDev p = panels[tl.panel];
  const int tid = threadIdx.x;
  const int chunk = blockIdx.y;
  const int64_t G = (int64_t)p.nx * p.ny;
  const bool two = p.col1 >= 0;

  double g0[KDE_GP], g1[KDE_GP], m[KDE_GP], l[KDE_GP];
#pragma unroll
  for (int k = 0; k < KDE_GP; ++k) {
    int64_t g = (int64_t)tl.start + tid + k * KDE_THREADS;
    if (g >= G) g = G - 1;                   // masked at the store
    const int ix = (int)(g % p.nx), iy = (int)(g / p.nx);
    const double ex = coords[p.ax + ix] - p.cx;
    const double ey = two ? coords[p.ay + iy] - p.cy : 0.0;
    g0[k] = two ? __builtin_fma(ey, p.u10, ex * p.u00) : ex * p.u00;
    g1[k] = two ? __builtin_fma(ey, p.u11, ex * p.u01) : 0.0;
    m[k] = -INFINITY;
    l[k] = 0.0;
  }

  const int64_t j_begin = (int64_t)chunk * chunk_rows;
  const int64_t j_end = j_begin + chunk_rows < N ? j_begin + chunk_rows : N;
  for (int64_t base = j_begin; base < j_end; base += KDE_STAGE) {
    __syncthreads();                         // the last stage has been read
    {
      const int64_t j = base + tid;
      double z0 = 0.0, z1 = 0.0, lw = KDE_LW_ZERO;   // rows past the end: not read
      if (j < j_end) {
        const double wj = w[j];
        lw = (wj == 0.0) ? KDE_LW_ZERO : log2(wj);
        const double ex = X[j * d + p.col0] - p.cx;
        if (two) {
          const double ey = X[j * d + p.col1] - p.cy;
          z0 = __builtin_fma(ey, p.u10, ex * p.u00);
          z1 = __builtin_fma(ey, p.u11, ex * p.u01);
        } else {
          z0 = ex * p.u00;
        }
      }
      sh[4 * tid] = z0; sh[4 * tid + 1] = z1; sh[4 * tid + 2] = lw;
    }
    __syncthreads();
    const int rows = (int)(j_end - base < KDE_STAGE ? j_end - base : KDE_STAGE);
    if (two) kde_rows<2>(sh, rows, g0, g1, m, l);
    else kde_rows<1>(sh, rows, g0, g1, m, l);
  }

#pragma unroll
  for (int k = 0; k < KDE_GP; ++k) {
    const int64_t g = (int64_t)tl.start + tid + k * KDE_THREADS;
    if (g < G) {
      // a NaN sum (NaN row or weight) as a live pair of reference NaN:
      // lse_combine skips a pair whose l is not positive
      const bool bad = l[k] != l[k];
      part_m[(int64_t)chunk * G_total + p.out + g] = bad ? l[k] : m[k];
      part_l[(int64_t)chunk * G_total + p.out + g] = bad ? 1.0 : l[k];
    }
  }
}

__global__ __launch_bounds__(KDE_THREADS) void kde_finish_kernel(
    const KdePanelDev* __restrict__ panels, const KdeTile* __restrict__ tiles,
    const double* __restrict__ part_m, const double* __restrict__ part_l,
    int nchunk, int64_t G_total, double* __restrict__ out) {
  const KdeTile tl = tiles[blockIdx.x];
  const KdePanelDev& p = panels[tl.panel];
  const int64_t G = (int64_t)p.nx * p.ny;
#pragma unroll
  for (int k = 0; k < KDE_GP; ++k) {
    const int64_t g = (int64_t)tl.start + threadIdx.x + k * KDE_THREADS;
    if (g >= G) continue;
    const int64_t i = p.out + g;
    const LsePair s = lse_combine<Base2>(part_m, part_l, G_total, nchunk, i);
    if (s.l > 0.0)
      out[i] = s.m > 0.5 * KDE_LW_ZERO ? LN2 * (s.m + log2(s.l)) + p.log_const : -INFINITY;
    else
      out[i] = s.l == 0.0 ? -INFINITY : s.l;               // NaN stays NaN
  }
}

// The chunk plan: a function of N and G_total alone.  As many chunks as the
// population has stages of 1024 rows, at most 64, and no more than keep the
// partial pairs within KDE_PART_BUDGET (one chunk beyond it).
struct KdePlan {
  int64_t max_tiles, part, chunk_rows;
  int nchunk;
};
KdePlan kde_plan(int64_t N, int P, int64_t G_total) {
  KdePlan k;
  k.max_tiles = ceil_div(G_total, KDE_TILE) + P;
  int64_t maxc = ceil_div(N, 1024);
  maxc = maxc < 1 ? 1 : (maxc > 64 ? 64 : maxc);
  int64_t nc;
  if (maxc * G_total <= KDE_PART_BUDGET) {
    nc = maxc;
    k.part = maxc * G_total;
  } else {
    nc = KDE_PART_BUDGET / G_total;
    nc = nc < 1 ? 1 : nc;
    k.part = G_total > KDE_PART_BUDGET ? G_total : KDE_PART_BUDGET;
  }
  k.chunk_rows = ceil_div(ceil_div(N, nc), KDE_STAGE) * KDE_STAGE;
  k.nchunk = (int)ceil_div(N, k.chunk_rows);     // no empty chunk
  return k;
}

bool kde_shape_ok(int64_t N, int d, int P, int64_t G_total) {
  return N >= 1 && d >= 1 && d <= 64 && P >= 1 && P <= ABC_KDE_MAX_PANELS &&
         G_total >= 1 && G_total <= ABC_KDE_MAX_POINTS;
}

}  // namespace
}  // namespace abc

using namespace abc;

struct KdeWs {
  KdePanelDev* panels;
  KdeTile* tiles;
  double* pm;
  double* pl;
  void carve(Carver& c, const KdePlan& k, int P) {
    panels = c.take<KdePanelDev>((size_t)P);
    tiles = c.take<KdeTile>((size_t)k.max_tiles);
    pm = c.take<double>((size_t)k.part);
    pl = c.take<double>((size_t)k.part);
  }
};

extern "C" size_t abc_kde_panels_bytes(int64_t N, int d, int P, int64_t G_total) {
  if (!kde_shape_ok(N, d, P, G_total)) return 0;
  return measure<KdeWs>(kde_plan(N, P, G_total), P);
}

extern "C" int abc_kde_panels(const double* X, const double* w, int64_t N, int d,
                              const abc_kde_panel* panels, int P,
                              const double* coords, int64_t n_coords, double* out,
                              int64_t G_total, void* ws, size_t ws_bytes,
                              void* stream) {
  ABC_CHECK_ARG(N >= 1 && d >= 1 && P >= 1 && G_total >= 1 && n_coords >= 1,
                "kde_panels: N, d, P, G_total, n_coords must be >= 1");
  if (!kde_shape_ok(N, d, P, G_total))
    return set_error(ABC_ERR_UNSUPPORTED,
                     "kde_panels: beyond d <= 64, P <= %d, G_total <= 2^24",
                     ABC_KDE_MAX_PANELS);
  ABC_CHECK_ARG(X && w && panels && coords && out && ws, "kde_panels: null pointer");
  const KdePlan k = kde_plan(N, P, G_total);
  std::vector<KdePanelDev> dev((size_t)P);
  std::vector<KdeTile> tiles;
  tiles.reserve((size_t)k.max_tiles);
  const double c = sqrt(0.5 * LOG2E);
  int64_t off = 0;
  for (int i = 0; i < P; ++i) {
    const abc_kde_panel& s = panels[i];
    const bool two = s.col[1] >= 0;
    ABC_CHECK_ARG(s.col[0] >= 0 && s.col[0] < d && s.col[1] >= -1 && s.col[1] < d,
                  "kde_panels: panel %d: column outside [0, d)", i);
    if (s.num[0] > ABC_KDE_MAX_AXIS || s.num[1] > ABC_KDE_MAX_AXIS)
      return set_error(ABC_ERR_UNSUPPORTED, "kde_panels: panel %d: axis beyond %d points",
                       i, ABC_KDE_MAX_AXIS);
    ABC_CHECK_ARG(s.num[0] >= 1 && s.num[1] >= 1 && (two || s.num[1] == 1),
                  "kde_panels: panel %d: bad grid shape %d x %d", i, s.num[0], s.num[1]);
    ABC_CHECK_ARG(s.axis[0] >= 0 && s.axis[0] + s.num[0] <= n_coords &&
                  (!two || (s.axis[1] >= 0 && s.axis[1] + s.num[1] <= n_coords)),
                  "kde_panels: panel %d: axis outside the coordinates", i);
    bool fin = isfinite(s.centre[0]) && isfinite(s.U[0]) && isfinite(s.log_const);
    if (two)
      fin = fin && isfinite(s.centre[1]) && isfinite(s.U[1]) && isfinite(s.U[2]) &&
            isfinite(s.U[3]);
    ABC_CHECK_ARG(fin, "kde_panels: panel %d: centre, U or log_const not finite", i);
    ABC_CHECK_ARG(s.out == off, "kde_panels: panel %d: out %lld, expected %lld "
                  "(panels lie back to back)", i, (long long)s.out, (long long)off);
    const int64_t G = (int64_t)s.num[0] * s.num[1];
    KdePanelDev& q = dev[(size_t)i];
    q.col0 = s.col[0]; q.col1 = two ? s.col[1] : -1;
    q.nx = s.num[0]; q.ny = s.num[1];
    q.ax = s.axis[0]; q.ay = two ? s.axis[1] : 0; q.out = off;
    q.cx = s.centre[0]; q.cy = two ? s.centre[1] : 0.0;
    q.u00 = s.U[0] * c;
    q.u01 = two ? s.U[1] * c : 0.0;
    q.u10 = two ? s.U[2] * c : 0.0;
    q.u11 = two ? s.U[3] * c : 0.0;
    q.log_const = s.log_const;
    for (int64_t st = 0; st < G; st += KDE_TILE) tiles.push_back(KdeTile{i, (int)st});
    off += G;
    ABC_CHECK_ARG(off <= G_total, "kde_panels: the panels hold more than G_total points");
  }
  ABC_CHECK_ARG(off == G_total, "kde_panels: the panels hold %lld points, G_total is %lld",
                (long long)off, (long long)G_total);
  KdeWs wk;
  ABC_CARVE(wk, "kde_panels", k, P);
  hipStream_t s = as_stream(stream);
  ABC_HIP(hipMemcpyAsync(wk.panels, dev.data(), dev.size() * sizeof(KdePanelDev),
                         hipMemcpyHostToDevice, s));
  ABC_HIP(hipMemcpyAsync(wk.tiles, tiles.data(), tiles.size() * sizeof(KdeTile),
                         hipMemcpyHostToDevice, s));
  ABC_HIP(hipStreamSynchronize(s));          // dev / tiles are locals
  const unsigned nt = (unsigned)tiles.size();
  hipLaunchKernelGGL(kde_panels_kernel, dim3(nt, (unsigned)k.nchunk), dim3(KDE_THREADS),
                     0, s, X, w, N, d, wk.panels, wk.tiles, coords, k.chunk_rows,
                     G_total, wk.pm, wk.pl);
  ABC_LAUNCHED();
  hipLaunchKernelGGL(kde_finish_kernel, dim3(nt), dim3(KDE_THREADS), 0, s, wk.panels,
                     wk.tiles, wk.pm, wk.pl, k.nchunk, G_total, out);
  ABC_LAUNCHED();
  return ABC_OK;
}
