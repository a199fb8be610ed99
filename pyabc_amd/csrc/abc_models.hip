// Model selection on the batched path: candidates of a generation with
// several competing models.
//
// Reference per-candidate closure with several models (pyabc/smc.py:610-662,
// _generate_valid_proposal):
//   t == 0:  m ~ model_prior, theta ~ prior_m                 (smc.py:624-626)
//   t  > 0:  m ~ p(t - 1) over the alive models, m' ~ K(. | m)
//            (random_variables.py:455-538), again while m' is dead
//            (smc.py:641-649); theta ~ T_m'.rvs(); the WHOLE attempt -- the
//            model included -- again while model_prior(m') prior_m'(theta)
//            is 0 (smc.py:654-656)
// The three model steps are one categorical draw from q~(m') ~ sum_m p_m
// K(m' | m) restricted to the alive models of positive prior mass; the host
// passes its inclusive scan (model_cdf).  Every attempt draws its model from
// the attempt's own Philox slot (SLOT_MODEL) and then runs the single-model
// attempt (propose_attempt, abc_candidate.h) in that model, so with one model
// the candidates are abc_propose's bit for bit.
#include "abc_candidate.h"

namespace abc {
namespace {

constexpr int MODELS_MAX = 16;        // models per generation
constexpr int MODELS_DMAX = 64;       // parameters per model
constexpr int MODELS_LDIM = LT_DMAX;  // L staged in LDS for d <= 16

struct ModelDev {
  const double* X;
  const double* cdf;
  const int32_t* guide;
  int64_t N;
  const double* L;
  const int32_t* kind;
  const double* params;
  const double* box;   // nullable: bisected by the block
  int d;
};

struct ModelsArgs {
  ModelDev m[MODELS_MAX];
  double cdf[MODELS_MAX];   // inclusive scan of the model masses
  int M;                    // descriptors
  int Mdraw;                // 1 + the last model of positive mass
  int dmax;
  int max_attempts;
  uint64_t seed;
  uint32_t gen;
};

// Per-block constants: every model's factor, support box and population
// total, read per lane (the lanes of a wave hold different models).
struct ModelsShared {
  float bmt[BM_TAB_SIZE];
  double L[MODELS_MAX * MODELS_LDIM * MODELS_LDIM];   // model m: [d x d] row-major
  double box[MODELS_MAX * 2 * MODELS_DMAX];
  double total[MODELS_MAX];
  double cdf[MODELS_MAX];
  ModelDev m[MODELS_MAX];
};

// propose_attempt's constants for one lane's model
struct LaneConsts {
  const float* bmt;
  const double* LT;    // (never read: no dimension is staged at D = 0)
  const double* box;
  double inv_step;     // (never read: no ancestor table)
};

template <int MODE>
__global__ __launch_bounds__(256) void models_propose_kernel(
    ModelsArgs G, int64_t idx0, int64_t B, int32_t* __restrict__ model_out,
    double* __restrict__ theta, int64_t* __restrict__ anc_out, int32_t* __restrict__ att_out) {
  __shared__ ModelsShared S;
  const int t = threadIdx.x, nt = blockDim.x;
  for (int k = t; k < BM_TAB_SIZE; k += nt) S.bmt[k] = BM_TAB[k];
  if (t < G.M) {
    S.m[t] = G.m[t];
    S.cdf[t] = G.cdf[t];
  }
  for (int m = 0; m < G.M; ++m) {
    const ModelDev& D = G.m[m];
    if (MODE == PROP_MVN && D.X != nullptr) {
      if (D.d <= MODELS_LDIM)
        for (int e = t; e < D.d * D.d; e += nt)
          S.L[m * MODELS_LDIM * MODELS_LDIM + e] = D.L[e];
      if (t == 0) S.total[m] = D.cdf[D.N - 1];
    } else if (t == 0) {
      S.total[m] = 0.0;
    }
    if (D.box != nullptr)
      for (int k = t; k < 2 * D.d; k += nt) S.box[m * 2 * MODELS_DMAX + k] = D.box[k];
  }
  // one wave per (model, dimension) without a precomputed box
  for (int e = t >> 6; e < G.M * MODELS_DMAX; e += nt >> 6) {
    const int m = e / MODELS_DMAX, k = e % MODELS_DMAX;
    const ModelDev& D = G.m[m];
    if (D.box == nullptr && k < D.d)
      support_bounds_wave(D.kind[k], D.params + 4 * k, S.box + m * 2 * MODELS_DMAX + 2 * k);
  }
  __syncthreads();
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const uint64_t g = (uint64_t)(idx0 + b);
  const double mtotal = S.cdf[G.Mdraw - 1];
  double th[MODELS_DMAX];
  int64_t j = -1;
  int m = 0, used = G.max_attempts + 1;
  for (int att = 0; att < G.max_attempts; ++att) {
    const u32x4 rm = philox(g, (uint32_t)att * SLOTS_PER_ATTEMPT + SLOT_MODEL, G.gen, G.seed);
    m = (int)upper_bound(S.cdf, G.Mdraw, uniform53(rm.x, rm.y) * mtotal);
    const ModelDev& D = S.m[m];
    ProposalArgs A{D.X, D.cdf, D.guide, D.N,
                   D.d <= MODELS_LDIM ? S.L + m * MODELS_LDIM * MODELS_LDIM : D.L,
                   D.kind, D.params, D.d, G.max_attempts, G.seed, G.gen};
    const LaneConsts C{S.bmt, nullptr, S.box + m * 2 * MODELS_DMAX, 0.0};
    if (propose_attempt<0, MODE>(A, C, S.total[m], g, att, th, j)) {
      used = att + 1;
      break;
    }
  }
  const int d = S.m[m].d;
  for (int k = 0; k < G.dmax; ++k) theta[b * G.dmax + k] = k < d ? th[k] : NAN;
  model_out[b] = m;
  anc_out[b] = MODE == PROP_PRIOR ? -1 : j;
  att_out[b] = used;
}

// abc_simulate_linear_gaussian's kernel with the row's model choosing its
// (src, a, sigma) table: the same expression and noise stream per statistic
__global__ __launch_bounds__(256) void models_simulate_lg_kernel(
    const double* __restrict__ theta, const int32_t* __restrict__ model, int64_t B, int dmax,
    int M, int S, const int32_t* __restrict__ src, const double* __restrict__ a,
    const double* __restrict__ sigma, uint64_t seed, uint32_t gen, int64_t idx0,
    double* __restrict__ x) {
  __shared__ float sbmt[BM_TAB_SIZE];
  stage_bm_tab(sbmt);
  const int G = (S + 3) >> 2;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= B * G) return;
  const int64_t b = e / G;
  const int q = (int)(e % G) * 4;
  const int m = model[b];
  if (m < 0 || m >= M) {   // no table to read: the row is NaN
    for (int t = 0; t < 4 && q + t < S; ++t) x[b * S + q + t] = NAN;
    return;
  }
  double n4[4];
  normals4((uint64_t)(idx0 + b), SLOT_SIM + (uint32_t)(q >> 2), gen, seed, n4, 4, sbmt);
  const int64_t o = (int64_t)m * S;
  for (int t = 0; t < 4 && q + t < S; ++t) {
    const int k = q + t;
    x[b * S + k] = a[o + k] * theta[b * dmax + src[o + k]] + sigma[o + k] * n4[t];
  }
}

// ---- stable partition by model id --------------------------------------------
// Tiles of PT_TILE positions: per tile the number of rows of every model
// (count), one block scans the [M x tiles] table in model-major order
// (scan), and every tile writes its rows of model m, in position order, from
// its offset (scatter).  Counts travel through the block scan four models at
// a time, 16 bits each (a tile holds 2048 rows), so the order comes from the
// scans alone.
constexpr int PT_T = 256, PT_I = 8, PT_TILE = PT_T * PT_I;

__device__ __forceinline__ int64_t pt_pack(const int32_t* id, int64_t base, int64_t B, int M,
                                           int grp, int* bad) {
  int64_t v = 0;
  for (int k = 0; k < PT_I; ++k) {
    if (base + k >= B) break;
    const int m = id[base + k];
    if (m < 0 || m >= M) { *bad = 1; continue; }
    if ((m >> 2) == grp) v += (int64_t)1 << (16 * (m & 3));
  }
  return v;
}

__global__ __launch_bounds__(PT_T) void partition_count_kernel(
    const int32_t* __restrict__ id, int64_t B, int M, int64_t nt, int64_t* __restrict__ tiles,
    int32_t* __restrict__ flag) {
  __shared__ int64_t sh[PT_T];
  const int64_t base = (int64_t)blockIdx.x * PT_TILE + threadIdx.x * PT_I;
  int bad = 0;
  for (int grp = 0; grp < (M + 3) / 4; ++grp) {
    int64_t tot;
    block_exscan<int64_t, PT_T>(pt_pack(id, base, B, M, grp, &bad), sh, tot);
    if (threadIdx.x < 4 && 4 * grp + threadIdx.x < M)
      tiles[(int64_t)(4 * grp + threadIdx.x) * nt + blockIdx.x] = (tot >> (16 * threadIdx.x)) & 0xFFFF;
  }
  if (bad) *flag = 1;   // (every writer stores the same value)
}

__global__ __launch_bounds__(PT_T) void partition_scan_kernel(
    int64_t* __restrict__ tiles, int64_t nt, int M, int64_t* __restrict__ counts) {
  __shared__ int64_t sh[PT_T];
  __shared__ int64_t start[MODELS_MAX + 1];
  const int64_t n = nt * M;
  const int64_t per = (n + PT_T - 1) / PT_T;
  const int64_t b0 = threadIdx.x * per;
  int64_t s = 0;
  for (int64_t k = 0; k < per; ++k)
    if (b0 + k < n) s += tiles[b0 + k];
  int64_t tot;
  int64_t off = block_exscan<int64_t, PT_T>(s, sh, tot);
  for (int64_t k = 0; k < per; ++k)
    if (b0 + k < n) {
      const int64_t v = tiles[b0 + k];
      tiles[b0 + k] = off;
      if ((b0 + k) % nt == 0) start[(b0 + k) / nt] = off;
      off += v;
    }
  if (threadIdx.x == 0) start[M] = tot;
  __syncthreads();
  if (threadIdx.x < M) counts[threadIdx.x] = start[threadIdx.x + 1] - start[threadIdx.x];
}

__global__ __launch_bounds__(PT_T) void partition_scatter_kernel(
    const int32_t* __restrict__ id, int64_t B, int M, int64_t nt,
    const int64_t* __restrict__ tile_off, int64_t* __restrict__ perm) {
  __shared__ int64_t sh[PT_T];
  const int64_t base = (int64_t)blockIdx.x * PT_TILE + threadIdx.x * PT_I;
  int bad = 0;
  for (int grp = 0; grp < (M + 3) / 4; ++grp) {
    int64_t tot;
    const int64_t ex = block_exscan<int64_t, PT_T>(pt_pack(id, base, B, M, grp, &bad), sh, tot);
    int64_t pos[4];
    for (int c = 0; c < 4; ++c)
      pos[c] = 4 * grp + c < M
                   ? tile_off[(int64_t)(4 * grp + c) * nt + blockIdx.x] + ((ex >> (16 * c)) & 0xFFFF)
                   : 0;
    for (int k = 0; k < PT_I; ++k) {
      if (base + k >= B) break;
      const int m = id[base + k];
      if (m < 0 || m >= M || (m >> 2) != grp) continue;
      // (pos[] indexed by compile-time constants: no scratch array)
      int64_t p;
      switch (m & 3) {
        case 0: p = pos[0]++; break;
        case 1: p = pos[1]++; break;
        case 2: p = pos[2]++; break;
        default: p = pos[3]++; break;
      }
      // an invalid id elsewhere shortens the groups: p < B always holds (the
      // counts sum to the valid rows), checked all the same
      if (p >= 0 && p < B) perm[p] = base + k;
    }
  }
}

struct PartitionWs {
  int64_t* tiles;   // [M x tiles] counts, then their exclusive scan
  int32_t* flag;    // an id outside [0, M)
  void carve(Carver& c, int64_t B, int M) {
    tiles = c.take<int64_t>((size_t)ceil_div(B > 0 ? B : 1, PT_TILE) * (size_t)(M > 0 ? M : 1));
    flag = c.take<int32_t>(1);
  }
};

}  // namespace
}  // namespace abc

using namespace abc;

extern "C" int abc_models_propose(const abc_model_desc* models, int M, const double* model_cdf,
                                  uint64_t seed, uint32_t generation, int64_t idx0, int64_t B,
                                  int max_attempts, int32_t* model, double* theta,
                                  int64_t* ancestor, int32_t* attempts, void* stream) {
  ABC_CHECK_ARG(models && model_cdf && M >= 1 && M <= MODELS_MAX, "models_propose: 1 <= M <= 16");
  ABC_CHECK_ARG(B >= 0 && max_attempts >= 1 && max_attempts < (1 << 15),
                "models_propose: bad B / max_attempts");
  ModelsArgs G{};
  G.M = M;
  G.max_attempts = max_attempts;
  G.seed = seed;
  G.gen = generation;
  int n_prior = 0;
  for (int m = 0; m < M; ++m) n_prior += models[m].X == nullptr;
  // (X == NULL in every descriptor: the prior draw; in no descriptor of
  // positive mass: the transitions)
  double prev = 0.0;
  for (int m = 0; m < M; ++m) {
    const abc_model_desc& s = models[m];
    ABC_CHECK_ARG(s.d >= 1 && s.d <= MODELS_DMAX, "models_propose: 1 <= d <= 64");
    ABC_CHECK_ARG(s.prior_kind && s.prior_params, "models_propose: null prior");
    ABC_CHECK_ARG(model_cdf[m] >= prev && model_cdf[m] < INFINITY,
                  "models_propose: model_cdf is not a finite non-decreasing scan");
    const bool mass = model_cdf[m] > prev;
    prev = model_cdf[m];
    if (mass) G.Mdraw = m + 1;
    if (n_prior < M) {
      ABC_CHECK_ARG(!mass || (s.X && s.cdf && s.L && s.N >= 1),
                    "models_propose: a model of positive mass needs X, cdf, L, N");
      ABC_CHECK_ARG(s.N < (1ll << 31), "models_propose: N too large");
    }
    G.m[m] = ModelDev{s.X, s.cdf, s.guide, s.X ? s.N : 0, s.L, s.prior_kind, s.prior_params,
                      s.support_box, s.d};
    G.cdf[m] = model_cdf[m];
    G.dmax = s.d > G.dmax ? s.d : G.dmax;
  }
  ABC_CHECK_ARG(G.Mdraw >= 1, "models_propose: no model of positive mass");
  if (B == 0) return ABC_OK;
  ABC_CHECK_ARG(model && theta && ancestor && attempts, "models_propose: null output");
  const dim3 grid((unsigned)ceil_div(B, 256));
  if (n_prior == M)
    hipLaunchKernelGGL((models_propose_kernel<PROP_PRIOR>), grid, dim3(256), 0, as_stream(stream),
                       G, idx0, B, model, theta, ancestor, attempts);
  else
    hipLaunchKernelGGL((models_propose_kernel<PROP_MVN>), grid, dim3(256), 0, as_stream(stream),
                       G, idx0, B, model, theta, ancestor, attempts);
  ABC_LAUNCHED();
  return ABC_OK;
}

extern "C" int abc_models_simulate_linear_gaussian(const double* theta, const int32_t* model,
                                                   int64_t B, int d_max, int M, int S,
                                                   const int32_t* src, const double* a,
                                                   const double* sigma, uint64_t seed,
                                                   uint32_t generation, int64_t idx0, double* x,
                                                   void* stream) {
  ABC_CHECK_ARG(d_max >= 1 && S >= 1 && B >= 0 && M >= 1 && M <= MODELS_MAX,
                "models_simulate: bad d_max/S/B/M");
  if (B == 0) return ABC_OK;
  ABC_CHECK_ARG(theta && model && src && a && sigma && x, "models_simulate: null pointer");
  const int64_t n = B * ((S + 3) / 4);
  hipLaunchKernelGGL(models_simulate_lg_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0,
                     as_stream(stream), theta, model, B, d_max, M, S, src, a, sigma, seed,
                     generation, idx0, x);
  ABC_LAUNCHED();
  return ABC_OK;
}

extern "C" size_t abc_models_partition_bytes(int64_t B, int M) {
  return measure<PartitionWs>(B, M);
}

extern "C" int abc_models_partition(const int32_t* model, int64_t B, int M, int64_t* perm,
                                    int64_t* counts, void* ws, size_t ws_bytes, void* stream) {
  ABC_CHECK_ARG(B >= 0 && M >= 1 && M <= MODELS_MAX, "models_partition: bad B / M");
  ABC_CHECK_ARG(counts && ws, "models_partition: null pointer");
  PartitionWs w;
  ABC_CARVE(w, "models_partition", B, M);
  hipStream_t s = as_stream(stream);
  if (B == 0) {
    ABC_HIP(hipMemsetAsync(counts, 0, sizeof(int64_t) * M, s));
    return ABC_OK;
  }
  ABC_CHECK_ARG(model && perm, "models_partition: null pointer");
  const int64_t nt = ceil_div(B, PT_TILE);
  ABC_HIP(hipMemsetAsync(w.flag, 0, sizeof(int32_t), s));
  hipLaunchKernelGGL(partition_count_kernel, dim3((unsigned)nt), dim3(PT_T), 0, s, model, B, M,
                     nt, w.tiles, w.flag);
  ABC_LAUNCHED();
  hipLaunchKernelGGL(partition_scan_kernel, dim3(1), dim3(PT_T), 0, s, w.tiles, nt, M, counts);
  ABC_LAUNCHED();
  hipLaunchKernelGGL(partition_scatter_kernel, dim3((unsigned)nt), dim3(PT_T), 0, s, model, B,
                     M, nt, w.tiles, perm);
  ABC_LAUNCHED();
  int32_t bad = 0;
  ABC_HIP(hipMemcpyAsync(&bad, w.flag, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  ABC_HIP(hipStreamSynchronize(s));
  ABC_CHECK_ARG(bad == 0, "models_partition: a model id outside [0, M)");
  return ABC_OK;
}
