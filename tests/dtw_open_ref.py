"""The open-end DTW (include/whisper_hip.h, wh_dtw_open) restated in numpy: the cost
recurrence, the score, the end row and the backtrace, without the oracle's code.  Also the
planted matrices the tests use.  Shared by test_forced_align_host.py and
test_gpu_forced_align.py."""
import numpy as np


def dtw_tables_cellwise(x):
    """(cost [N+1][M+1] float32, trace [N+1][M+1]) cell by cell, as the definition reads."""
    x = np.asarray(x, dtype=np.float32)
    N, M = x.shape
    cost = np.full((N + 1, M + 1), np.inf, dtype=np.float32)
    trace = np.zeros((N + 1, M + 1), dtype=np.int8)
    cost[0, 0] = 0
    trace[0, :] = 2
    trace[:, 0] = 1
    for i in range(1, N + 1):
        for j in range(1, M + 1):
            c0, c1, c2 = cost[i - 1, j - 1], cost[i - 1, j], cost[i, j - 1]
            if c0 < c1 and c0 < c2:
                c, t = c0, 0
            elif c1 < c0 and c1 < c2:
                c, t = c1, 1
            else:
                c, t = c2, 2
            cost[i, j] = np.float32(np.float64(x[i - 1, j - 1]) + np.float64(c))
            trace[i, j] = t
    return cost, trace


def dtw_tables(x):
    """The same tables, one anti-diagonal at a time (cell (i, j) reads diagonals i + j - 1
    and i + j - 2 only), which keeps every cell's arithmetic and comparisons and makes the
    1500-column cases quick."""
    x = np.asarray(x, dtype=np.float32)
    N, M = x.shape
    cost = np.full((N + 1, M + 1), np.inf, dtype=np.float32)
    trace = np.zeros((N + 1, M + 1), dtype=np.int8)
    cost[0, 0] = 0
    trace[0, :] = 2
    trace[:, 0] = 1
    for d in range(2, N + M + 1):
        i = np.arange(max(1, d - M), min(N, d - 1) + 1)
        j = d - i
        c0, c1, c2 = cost[i - 1, j - 1], cost[i - 1, j], cost[i, j - 1]
        first = (c0 < c1) & (c0 < c2)
        second = ~first & (c1 < c0) & (c1 < c2)
        c = np.where(first, c0, np.where(second, c1, c2))
        cost[i, j] = (x[i - 1, j - 1].astype(np.float64) + c.astype(np.float64)).astype(np.float32)
        trace[i, j] = np.where(first, 0, np.where(second, 1, 2))
    return cost, trace


def dtw_open_ref(x, min_rows, row_penalty, tables=None):
    """(path [2][L] int32, end_row, scores [N] float32) of cost matrix ``x [N][M]``.
    ``min_rows == 0`` is the closed form: end_row = N.  ``tables``: ``dtw_tables(x)`` when the
    caller already has them (they do not depend on min_rows or the penalty)."""
    x = np.asarray(x, dtype=np.float32)
    N, M = x.shape
    assert N >= 1 and M >= 1 and 0 <= min_rows <= N
    pen = np.float64(np.float32(row_penalty))  # the ABI takes an fp32 penalty
    assert np.isfinite(pen) and pen >= 0
    cost, trace = dtw_tables(x) if tables is None else tables
    scores = np.array([np.float32(np.float64(cost[i, M]) + pen * i) for i in range(1, N + 1)], dtype=np.float32)
    e = N
    if min_rows > 0:
        e = min_rows
        for i in range(min_rows + 1, N + 1):
            if scores[i - 1] < scores[e - 1]:  # fp32 compare; the smallest i keeps a tie
                e = i
    a, b = e, M
    text, time = [], []
    while a > 0 or b > 0:
        text.append(a - 1)
        time.append(b - 1)
        t = trace[a, b]
        if t == 0:
            a, b = a - 1, b - 1
        elif t == 1:
            a -= 1
        else:
            b -= 1
    return np.array([text[::-1], time[::-1]], dtype=np.int32), e, scores


def planted_matrix(n_rows, n_cols, spoken_rows, noise, seed, min_frames=3):
    """A z-normalised attention-like matrix [n_rows][n_cols] (rows are tokens): the first
    ``spoken_rows`` rows own consecutive stretches of at least ``min_frames`` frames that
    cover all the columns (weight 1 there), the other rows own nothing; uniform noise of
    amplitude ``noise`` is added and every column is z-normalised over the rows, as
    find_alignment's matrix is.  Returns (x = -matrix as float32, bounds): row r owns frames
    ``bounds[r] .. bounds[r + 1] - 1``.  The planted end row of x is ``spoken_rows``."""
    rng = np.random.default_rng(seed)
    assert 1 <= spoken_rows <= n_rows and spoken_rows * min_frames <= n_cols
    extra = n_cols - spoken_rows * min_frames
    cuts = np.sort(rng.integers(0, extra + 1, spoken_rows - 1))
    sizes = np.diff(np.concatenate(([0], cuts, [extra]))) + min_frames
    bounds = np.concatenate(([0], np.cumsum(sizes))).astype(int)
    w = np.zeros((n_rows, n_cols))
    for r in range(spoken_rows):
        w[r, bounds[r]:bounds[r + 1]] = 1.0
    w += noise * rng.random((n_rows, n_cols))
    sd = w.std(axis=0, keepdims=True)
    w = (w - w.mean(axis=0, keepdims=True)) / np.where(sd > 0, sd, 1.0)  # one row: nothing to normalise
    return (-w).astype(np.float32), bounds
