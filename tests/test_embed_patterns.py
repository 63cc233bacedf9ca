"""CPU: the designed inputs of tests/embed_patterns.py are what
tests/test_gpu_embed_structure.py needs them to be, checked before anything
runs on a GPU -- the forward's rows have the nonzero counts they are named
for and meet every flush condition of bag_linear_kernel's list, and the
weight gradient's (range, chunk, block) lists, cut with bag_dw_kernel's
geometry, have every total its pipeline branches on."""
import numpy as np
import pytest

import embed_patterns as ep

DW_CASES = [(3100, 303), (1537, 304), (70_000, 47)]  # tests/test_gpu_embed_structure.py: DW_CASES' (M, K)


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("K", ep.FWD_K)
def test_forward_rows_meet_every_flush_condition(K, exact):
    V, rows = ep.forward_rows(K, K, exact)
    assert V.shape == (len(rows), K) and V.dtype == np.float32
    c = {name: ep.forward_census(V[i]) for name, i in rows.items()}
    for n in ep.FWD_COUNTS + (K,):
        assert c[f"n{n}"]["nnz"] == n, f"nonzero count of row n{n}: {c[f'n{n}']}"
    want = {"full512": 512, "full512_last": 513, "at_last": 1, "dense_a": K, "zero_mid": 0, "dense_b": K,
            "neg_zero": ep.NEG_ZERO_NNZ}
    for name, n in want.items():
        assert c[name]["nnz"] == n, f"nonzero count of row {name}: {c[name]}"
    assert rows["zero_mid"] == rows["dense_a"] + 1 == rows["dense_b"] - 1
    assert np.signbit(V[rows["neg_zero"]]).sum() >= K - ep.NEG_ZERO_NNZ  # every other entry is -0.0
    assert np.count_nonzero(V[rows["full512"]]) == 512 and not V[rows["full512"], 512:].any()
    assert V[rows["full512_last"], K - 1] != 0 and V[rows["at_last"], K - 1] != 0
    assert ("at1535" in rows) == (K > 1535) and ("at1536" in rows) == (K > 1536)
    for name, col in (("at1535", ep.SCAN_COLS - 1), ("at1536", ep.SCAN_COLS)):  # the scan-round boundary
        if name in rows:
            assert np.nonzero(V[rows[name]])[0].tolist() == [col], name
    # the list's conditions, each named
    assert c["full512"] == {"nnz": 512, "overflows": 0, "exactly_full": 1}, "exactly full, then empty chunks"
    assert c["n512"]["overflows"] == 0 and c["n512"]["exactly_full"] == 1, "exactly full at the row's end"
    assert c["n511"]["overflows"] == 0 and c["n511"]["exactly_full"] == 0, "one short of full"
    assert c["full512_last"]["overflows"] == 1 and c["full512_last"]["exactly_full"] == 1, "full, then one entry"
    assert c["n513"]["overflows"] == 1, "the list overflows once"
    assert c["n1024"]["overflows"] >= 2 and c["n1025"]["overflows"] >= 2, "the list overflows several times"
    assert c[f"n{K}"]["overflows"] == (K - 1) // ep.CAP and c[f"n{K}"]["exactly_full"] == K // ep.CAP, "dense row"
    assert all(c[name]["overflows"] == 0 for name in ("n0", "n1", "at_last", "zero_mid"))
    assert c["neg_zero"]["overflows"] == 1, "-0.0 entries are not list entries"


@pytest.mark.parametrize("want_db", [True, False])
@pytest.mark.parametrize("M,K", DW_CASES)
def test_weight_gradient_lists_have_every_total(M, K, want_db):
    V = ep.dw_matrix(M, K, M + K, True)
    assert np.array_equal(V != 0, ep.dw_matrix(M, K, M + K, False) != 0)  # exact and real data: one pattern
    c = ep.dw_census(V, want_db, 256)
    for C in (1, 257, 512):  # the geometry does not depend on C at these sizes
        assert ep.dw_splits(M, K + 1, C) == (c["ranges"], c["rows_per_range"])
    tot = c["totals"]
    if M == 70_000:  # 128 ranges of 547 rows: chunks of 256, 256 and 35 rows, the middle one empty
        assert (c["ranges"], c["rows_per_range"]) == (128, 547)
        assert c["empty_chunk_between_populated"] >= 1, "empty_chunk_between_populated"
        assert c["db_column_closes_a_block"] == int(want_db)
        if want_db:  # the db column alone in its block's list: the chunk's height
            assert tot.get(256, 0) >= 256 and tot.get(35, 0) >= 127
        return
    # at most two chunks a range below 65536 rows (ranges hold at most 512), so no empty chunk between two
    assert c["empty_chunk_between_populated"] == 0 and c["rows_per_range"] <= 512
    assert (c["ranges"], c["rows_per_range"]) == {3100: (7, 443), 1537: (4, 385)}[M]
    assert c["rows_per_range"] % ep.DW_ROWS != 0 and c["partial_chunks"] == c["ranges"]
    for t in ep.DW_TOTALS:
        assert tot.get(t, 0) >= 1, f"no (chunk, block) list with total {t}: {sorted(tot)}"
    assert sum(n for t, n in tot.items() if 17 <= t <= 32) >= 3 and sum(n for t, n in tot.items() if 33 <= t <= 48) >= 3
    assert c["run_spans_batch_boundary"] >= 1, "run_spans_batch_boundary"
    assert c["run_ends_on_batch_boundary"] >= 1, "run_ends_on_batch_boundary"
    assert c["column_only_nonzero_is_range_last_row"] >= 1, "column_only_nonzero_is_range_last_row"
    assert V[2 * c["rows_per_range"] - 1, ep.DW_LAST_ROW_COLUMN] != 0
    assert c["db_column_closes_a_block"] == int(want_db and K == 303), "db_column_closes_a_block"
    assert c["db_column_opens_a_block"] == int(want_db and K == 304), "db_column_opens_a_block"
