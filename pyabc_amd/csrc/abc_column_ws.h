// Workspace layouts of the column statistics, shared by the files that carve
// them: abc_select.hip (median / MAD by radix select), abc_sort.hip
// (abc_column_std, abc_column_mad), abc_scale.hip (abc_column_scale) and
// abc_whiten.hip (abc_column_gram, abc_column_quantile).
#pragma once
#include "abc_common.h"

namespace abc {

// the buffers of one select pass
struct SelectBufs {
  uint64_t* scratch;         // window keys (worst case: all)
  uint64_t* win;             // windows [lo, hi]
  unsigned long long* cnt;   // in-window / below counts
  double* med;               // medians
  void carve(Carver& cv, int64_t R, int S) {
    scratch = cv.take<uint64_t>((size_t)R * S);
    win = cv.take<uint64_t>((size_t)2 * S);
    cnt = cv.take<unsigned long long>((size_t)2 * S);
    med = cv.take<double>((size_t)S);
  }
};

// CMAD: the select's buffers and the MAD beside the MAD to x0
struct CmadBufs {
  SelectBufs sel; double* mad;
  void carve(Carver& cv, int64_t R, int S) {
    sel.carve(cv, R, S);
    mad = cv.take<double>((size_t)S);
  }
};

constexpr int CS_BLOCKS = 256;   // colsum_kernel's fixed grid
struct ColumnStdBufs {
  double* part; double* mean;
  void carve(Carver& cv, int S) {
    part = cv.take<double>((size_t)CS_BLOCKS * S);
    mean = cv.take<double>((size_t)S);
  }
};

// abc_column_stats_workspace: one buffer for abc_column_std or abc_column_mad,
// the regions of both from the same start, as large as the larger
struct ColumnStatsWs {
  ColumnStdBufs sd; SelectBufs sel;
  void carve(Carver& cv, int64_t R, int S) {
    Carver other = cv;
    sd.carve(cv, S);
    sel.carve(other, R, S);
    if (other.off > cv.off) cv = other;
  }
};

// abc_column_gram in an abc_column_stats_workspace(R, S) buffer: the mean
// pass's buffers, then the row splits' partial [S x S] blocks -- behind the
// means as many as the buffer holds (it holds 8 R S bytes), else in place of
// the mean pass's partial sums, which are spent once the means are final
// (2048 S bytes: 256 / S blocks, one at S = 256).
constexpr int GRAM_SPLITS = 64;  // row splits at most
struct GramBufs {
  ColumnStdBufs sd; double* gpart; int nsplit;
  void carve(Carver& cv, int64_t R, int S) {
    const size_t end = measure<ColumnStatsWs>(R, S) - Carver::SLACK;  // every caller's buffer
    sd.carve(cv, S);
    const size_t blk = (size_t)S * S * sizeof(double);
    const size_t start = align_up(cv.off, 256);
    const size_t behind = end > start ? (end - start) / blk : 0;
    const size_t inplace = (size_t)CS_BLOCKS / S;
    const size_t most = (size_t)ceil_div(R, 64) < (size_t)GRAM_SPLITS ? (size_t)ceil_div(R, 64)
                                                                    : (size_t)GRAM_SPLITS;
    if (behind >= inplace) {
      nsplit = (int)(behind < most ? behind : most);
      gpart = cv.take<double>((size_t)nsplit * S * S);
    } else {
      nsplit = (int)(inplace < most ? inplace : most);
      gpart = sd.part;
    }
  }
};

// abc_select.hip
// out[c] = median_c(|X[:, c] - median_c(X[:, c])|)
int column_mad_select(const double* X, int64_t R, int S, double* out, const SelectBufs& b,
                      hipStream_t s);
// out[c] = median_c(|X[:, c] - centre[c]|): one of the MAD's two passes
int column_absdev_median_select(const double* X, int64_t R, int S, const double* centre,
                                double* out, const SelectBufs& b, hipStream_t s);
// out[c] = MAD_c + median_c(|X[:, c] - x0[c]|): three select passes, one add
int column_cmad_select(const double* X, int64_t R, int S, const double* x0, double* out,
                       const CmadBufs& b, hipStream_t s);
// out[c] = numpy's default ("linear") percentile 100 q of X[:, c]: one pass
int column_quantile_select(const double* X, int64_t R, int S, double q, double* out,
                           const SelectBufs& b, hipStream_t s);
// abc_sort.hip: b.mean[c] = mean_r X[r, c] (column_std's first pass)
int column_mean(const double* X, int64_t R, int S, const ColumnStdBufs& b, hipStream_t s);
// abc_sort.hip: np.std, two-pass
int column_std(const double* X, int64_t R, int S, double* out, const ColumnStdBufs& b,
               hipStream_t s);

}  // namespace abc
