"""Record a library's workspace query values in tests/golden/workspace_sizes.json.

Run against the library of the commit BEFORE a change to the workspace
layouts (built in a scratch worktree); tests/test_workspace_sizes.py then
holds the changed library to those values.  Pure host: no GPU.

    ABCGPU_LIB=<parent worktree>/pyabc_amd/libabcgpu.so \
      python tests/golden/make_golden_workspace.py

Rows are [query, [arguments], bytes]: per query the degenerate shape, one
shape on each side of every branch of its layout, and the c3 / c4 / c5 shapes.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from pyabc_amd import _native as nat  # noqa: E402

KN_MIN_N = 2048          # abc_local_knn.h
X3_NEST_CAP = 16384      # abc_mvn_x3.hip
WQ_ONE_MAX = 1 << 20     # abc_quantile.hip
C3_N, C3_B = 10 ** 6, 4_600_000
C4_R, C4_S = 670_000, 256
C5_N = 10 ** 5


def shapes():
    rows = []

    def add(q, *args):
        rows.append((q, list(args)))

    sizes = (0, 1, 1000, 70_001, C5_N, C3_N)
    for n in sizes + (C3_B,):
        for q in ("abc_scan_workspace", "abc_normalize_weights_workspace",
                  "abc_compact_workspace", "abc_candidates_workspace",
                  "abc_bootstrap_cv_workspace"):
            add(q, n)
    add("abc_candidates_propose_workspace")
    add("abc_temper_workspace")
    for n in sizes:
        add("abc_sort_pairs_workspace", n)
        add("abc_weighted_quantile_sorted_workspace", n)
    for n in sizes + (WQ_ONE_MAX - 1, WQ_ONE_MAX, WQ_ONE_MAX + 1, 1 << 24):
        add("abc_weighted_quantile_workspace", n)
    for n in (0, 1, 1000, C3_N):
        for d in (1, 2, 10, 16, 64, 65, 80):     # d > 64: the wide kernels
            add("abc_weighted_moments_workspace", n, d)
    # column statistics: R below / above the std layout's 256 blocks
    for R, S in ((1, 1), (100, 12), (255, 3), (257, 3), (4097, 3), (C4_R, C4_S)):
        add("abc_column_stats_workspace", R, S)
        for kind in range(10):
            add("abc_column_scale_workspace", kind, R, S)
    for kind in (-1, 10):
        add("abc_column_scale_workspace", kind, 100, 12)
    add("abc_column_scale_workspace", nat.ABC_SCALE_BIAS, 0, 12)
    # mvn density: every precision, M on both sides of the nested pass's cap
    for prec in (nat.ABC_PREC_F64, nat.ABC_PREC_F32, nat.ABC_PREC_X3):
        for M, N, r in ((0, 1, 1), (1, 1, 1), (4096, 4096, 10), (200, 3000, 10),
                        (X3_NEST_CAP - 1, 4096, 10), (X3_NEST_CAP, 4096, 10),
                        (X3_NEST_CAP + 1, 4096, 10), (100_000, 100_000, 2),
                        (C3_N, C3_N, 10), (C3_B, C3_N, 10)):
            add("abc_mvn_logpdf_workspace", M, N, r, prec)
    # local fit: every d at which a path or a constant changes, N around the
    # k-NN threshold
    for d in (1, 2, 5, 6, 8, 9, 16, 17, 64, 65, 80):
        for n in (1, 300, KN_MIN_N - 1, KN_MIN_N, KN_MIN_N + 1, C5_N):
            add("abc_local_fit_workspace", n, d)
    add("abc_local_fit_workspace", 0, 5)
    for d in (1, 2, 5, 6, 8, 9, 16, 17, 80):
        for M, N in ((0, 1), (1, 1), (300, 300), (5000, 2049), (C5_N, C5_N)):
            add("abc_local_logpdf_workspace", M, N, d)
    return rows


def main():
    rows = [[q, args, nat.query(q, *args)] for q, args in shapes()]
    path = os.path.join(HERE, "workspace_sizes.json")
    with open(path, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")
    print("workspace_sizes", len(rows), "rows from", nat.LIB_PATH)


if __name__ == "__main__":
    main()
