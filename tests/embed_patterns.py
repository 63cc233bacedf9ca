"""TEST INFRASTRUCTURE ONLY.  Designed inputs for the bag-linear kernels.

csrc/embed.hip's bag_linear_kernel appends a row's nonzeros, 64 columns at a
time, to a CAP-entry list and flushes it early when the next 64 columns would
not fit; it loads the row SCAN * 64 columns per round.  bag_dw_kernel cuts V
into (row range, DW_ROWS-row chunk, DW_KB-column block) lists and walks each
through a two-buffer pipeline of DW_U-entry batches whose branches turn on
the list's total against 16, 32 and 48.  Bag-of-characters rows (11 nonzeros)
and fully dense blocks meet none of those edges; the builders here place
them, and the censuses count them from the arrays and the kernels' geometry
alone.  numpy only.
"""
from __future__ import annotations

import numpy as np

# embed.hip: CAP, 64 * SCAN, DW_KB, DW_ROWS, DW_U, DW_PART_BUDGET
CAP, SCAN_COLS, DW_KB, DW_ROWS, DW_U, DW_PART_BUDGET = 512, 24 * 64, 16, 256, 16, 1 << 30

FWD_K = (1535, 1536, 1537, 4369)
FWD_COUNTS = (0, 1, 511, 512, 513, 1024, 1025)
NEG_ZERO_NNZ = 600


def _values(rng, n, exact):
    """n nonzero values: small integers (exact data) or normals."""
    if exact:
        return (rng.integers(1, 4, n) * rng.choice([-1, 1], n)).astype(np.float32)
    v = rng.standard_normal(n).astype(np.float32)
    v[v == 0.0] = 1.0
    return v


def forward_rows(K: int, seed: int, exact: bool):
    """(V [M, K], rows): the designed rows of the forward, rows = name -> index.
      n<count>       `count` nonzeros at random columns (FWD_COUNTS, and n<K>: all)
      full512        exactly columns 0..511: the list exactly full, the next chunk empty
      full512_last   columns 0..511 plus column K - 1: one entry over
      at1535 / at1536 / at_last   a single nonzero at the last column of the first
                     scan round, the first of the second (where K has them), at K - 1
      dense_a, zero_mid, dense_b   an all-zero row between two dense rows
      neg_zero       NEG_ZERO_NNZ nonzeros and -0.0 everywhere else (skipped)"""
    rng, vrng = np.random.default_rng(seed), np.random.default_rng(seed + 1)  # positions; values
    rows, data = {}, []

    def add(name, cols, fill=0.0):
        cols = np.asarray(cols, dtype=np.int64)
        v = np.full(K, fill, dtype=np.float32)
        v[cols] = _values(vrng, cols.size, exact)
        rows[name] = len(data)
        data.append(v)

    for n in FWD_COUNTS + (K,):
        add(f"n{n}", rng.choice(K, n, replace=False))
    add("full512", np.arange(512))
    add("full512_last", np.r_[0:512, K - 1])
    if K > 1535:
        add("at1535", [1535])
    if K > 1536:
        add("at1536", [1536])
    add("at_last", [K - 1])
    add("dense_a", np.arange(K)), add("zero_mid", []), add("dense_b", np.arange(K))
    add("neg_zero", rng.choice(K, NEG_ZERO_NNZ, replace=False), fill=-0.0)
    return np.stack(data), rows


def forward_census(v) -> dict:
    """One row's walk as bag_linear_kernel cuts it: 64 columns at a time, the
    list flushed first when cnt + n > CAP.  nnz, overflow flushes, and how
    often the list was exactly full."""
    nz = np.asarray(v) != 0.0  # -0.0 != 0.0 is false: skipped, as in the kernel
    cnt = overflows = full = 0
    for k0 in range(0, nz.size, 64):
        n = int(nz[k0:k0 + 64].sum())
        if n == 0:
            continue
        if cnt + n > CAP:
            overflows += 1
            cnt = 0
        cnt += n
        full += cnt == CAP
    return {"nnz": int(nz.sum()), "overflows": overflows, "exactly_full": full}


# ------------------------------------------------------------------ weight gradient
DW_TOTALS = (0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 4096)
# the runs (entries per column, columns ascending) that make up each total: 17 and 48 have a run that ends
# exactly on a 16-entry batch boundary with another behind it, 31 / 33 / 47 / 49 a run that spans one
DW_RUNS = {0: (), 1: (1,), 15: (15,), 16: (7, 9), 17: (16, 1), 31: (31,), 32: (16, 16), 33: (10, 23), 47: (20, 27),
           48: (16, 32), 49: (48, 1), 4096: (DW_ROWS,) * DW_KB}
DW_LAST_ROW_COLUMN = 12 * DW_KB + 3  # a column whose only nonzero is its range's last row
DW_SPRINKLE_FROM = 13 * DW_KB        # columns from here on: two random nonzeros a row


def dw_splits(M: int, Keff: int, C: int):
    """(ranges, rows per range): bag_dw_splits' rule and the launcher's ceil_div (embed.hip)."""
    by_mem = max(1, DW_PART_BUDGET // max(1, Keff * C * 4))
    S = max(1, min(128, by_mem, -(-M // 512)))
    rps = -(-M // S)
    return -(-M // rps), rps


def dw_matrix(M: int, K: int, seed: int, exact: bool):
    """V [M, K] for the weight gradient.  Column block b < 12 of the chunk c
    of row range y holds DW_TOTALS[(b + y + 5 c) % 12] entries in the runs of
    DW_RUNS (where the chunk is high enough), except that a range's chunk 1
    stays EMPTY when the range has three chunks (an empty chunk between two
    populated ones).  K <= 12 * DW_KB keeps only the blocks that fit."""
    rng, vrng = np.random.default_rng(seed), np.random.default_rng(seed + 1)  # positions; values
    V = np.zeros((M, K), dtype=np.float32)
    ranges, rps = dw_splits(M, K + 1, 1)
    for y in range(ranges):
        r_lo, r_hi = y * rps, min(M, (y + 1) * rps)
        chunks = -(-(r_hi - r_lo) // DW_ROWS)
        for c in range(chunks):
            r0 = r_lo + c * DW_ROWS
            h = min(DW_ROWS, r_hi - r0)
            if chunks >= 3 and c == 1:
                continue
            for b in range(min(12, K // DW_KB)):
                runs = DW_RUNS[DW_TOTALS[(b + y + 5 * c) % 12]]
                if not runs or max(runs) > h:
                    continue
                cols = np.sort(rng.choice(DW_KB, len(runs), replace=False)) + b * DW_KB
                for col, n in zip(cols, runs):
                    V[r0 + np.sort(rng.choice(h, n, replace=False)), col] = _values(vrng, n, exact)
    if K > DW_LAST_ROW_COLUMN:
        V[min(M, 2 * rps) - 1, DW_LAST_ROW_COLUMN] = _values(vrng, 1, exact)[0]
    if K > DW_SPRINKLE_FROM:
        for _ in range(2):
            cols = rng.integers(DW_SPRINKLE_FROM, K, M)
            V[np.arange(M), cols] = _values(vrng, M, exact)
    return V


def dw_census(V, want_db: bool, C: int) -> dict:
    """The (range, chunk, block) lists of bag_dw_kernel over V (and the db
    column of ones behind it): how often each total occurs, and the run
    conditions of the pipeline."""
    M, K = V.shape
    Keff = K + (1 if want_db else 0)
    nz = np.concatenate([np.asarray(V) != 0.0, np.ones((M, Keff - K), dtype=bool)], axis=1)
    ranges, rps = dw_splits(M, K + 1, C)
    blocks = -(-Keff // DW_KB)
    c = {"ranges": ranges, "rows_per_range": rps, "blocks": blocks, "totals": {}, "run_spans_batch_boundary": 0,
         "run_ends_on_batch_boundary": 0, "empty_chunk_between_populated": 0, "partial_chunks": 0,
         "column_only_nonzero_is_range_last_row": 0, "db_column_opens_a_block": int(want_db and K % DW_KB == 0),
         "db_column_closes_a_block": int(want_db and Keff % DW_KB == 0)}
    for y in range(ranges):
        r_lo, r_hi = y * rps, min(M, (y + 1) * rps)
        per_chunk = []
        for r0 in range(r_lo, r_hi, DW_ROWS):
            c["partial_chunks"] += r_hi - r0 < DW_ROWS
            cols = nz[r0:min(r0 + DW_ROWS, r_hi)].sum(0)
            per_chunk.append(cols)
            for b in range(blocks):
                runs = cols[b * DW_KB:(b + 1) * DW_KB]
                runs = runs[runs > 0]
                total = int(runs.sum())
                c["totals"][total] = c["totals"].get(total, 0) + 1
                ends = np.cumsum(runs)
                begins = ends - runs
                c["run_spans_batch_boundary"] += int(((ends - 1) // DW_U > begins // DW_U).sum())
                c["run_ends_on_batch_boundary"] += int(((ends % DW_U == 0) & (ends < total)).sum())
        per_chunk = np.array(per_chunk)  # [chunks, Keff]
        for b in range(blocks):
            pop = per_chunk[:, b * DW_KB:(b + 1) * DW_KB].sum(1) > 0
            if pop.any():
                lo, hi = np.nonzero(pop)[0][[0, -1]]
                c["empty_chunk_between_populated"] += int((~pop[lo:hi]).sum())
        only_last = (nz[r_lo:r_hi, :K].sum(0) == 1) & nz[r_hi - 1, :K]
        c["column_only_nonzero_is_range_last_row"] += int(only_last.sum())
    return c
