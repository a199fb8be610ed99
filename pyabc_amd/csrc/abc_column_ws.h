// Workspace layouts of the column statistics, shared by the files that carve
// them: abc_select.hip (median / MAD by radix select), abc_sort.hip
// (abc_column_std, abc_column_mad) and abc_scale.hip (abc_column_scale).
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
// abc_sort.hip: np.std, two-pass
int column_std(const double* X, int64_t R, int S, double* out, const ColumnStdBufs& b,
               hipStream_t s);

}  // namespace abc
