"""CPU: the designed graphs of tests/graph_patterns.py are what
tests/test_gpu_graphconv_structure.py needs them to be, checked before
anything runs on a GPU: well formed, no heavy row in P or in its transpose
(else the one-kernel path is silently not taken), and every condition of the
gather role's index logic present at least once for every (N, L) and DropEdge
variant the GPU tests use."""
import functools

import numpy as np
import pytest

import graph_patterns as gp

SEED, SHAPES, VARIANTS = gp.SEED, gp.SHAPES_NL, gp.VARIANTS

STRUCTURE = ("total_zero", "total_multiple_of_64", "row_end_on_fetch_boundary", "total_over_64",
             "total_2048_or_more", "seven_leading_empty_rows", "seven_trailing_empty_rows",
             "groups_with_one_valid_row", "empty_tiles")


@functools.lru_cache(maxsize=None)
def _graph(N, L):
    return gp.pattern_graph(N, L, SEED)


def _well_formed(rowptr, colidx, N, L):
    assert rowptr.dtype == np.int32 and colidx.dtype == np.int32
    assert rowptr.size == N * L + 1 and rowptr[0] == 0 and rowptr[-1] == colidx.size
    assert np.all(np.diff(rowptr) >= 0)
    assert colidx.min() >= 0 and colidx.max() < N
    seg = np.repeat(np.arange(N * L), np.diff(rowptr))
    same = seg[1:] == seg[:-1]
    assert np.all(colidx[1:][same] > colidx[:-1][same])  # sorted and unique within a segment


@pytest.mark.parametrize("N,L", SHAPES)
def test_pattern_graph_is_well_formed_and_never_heavy(N, L):
    rowptr, colidx, c = _graph(N, L)
    _well_formed(rowptr, colidx, N, L)
    rpt, cit = gp.transpose_host(rowptr, colidx, L, N)
    assert rpt[-1] == rowptr[-1]
    # (a transposed segment lists source rows in ascending order, each once: well formed in the same sense)
    _well_formed(rpt, cit, N, L)
    ct = gp.census(rpt, cit, L, N)
    assert c["max_row_degree"] == gp.HEAVY and c["max_in_degree"] <= gp.HEAVY  # the largest row that is not heavy
    assert ct["max_row_degree"] == c["max_in_degree"] and ct["max_in_degree"] == c["max_row_degree"]


@pytest.mark.parametrize("N,L", SHAPES)
def test_transpose_host_is_a_stable_involution(N, L):
    rowptr, colidx, _ = _graph(N, L)
    rpt, cit, eid = gp.transpose_host(rowptr, colidx, L, N, return_eid=True)
    back = gp.transpose_host(rpt, cit, L, N)
    assert np.array_equal(back[0], rowptr) and np.array_equal(back[1], colidx)
    # entry e' of the transpose is forward entry eid[e']: (n, t, m) became (m, t, n)
    seg = np.repeat(np.arange(N * L), np.diff(rowptr))
    segt = np.repeat(np.arange(N * L), np.diff(rpt))
    assert np.array_equal(colidx[eid], segt // L) and np.array_equal(seg[eid] // L, cit)
    assert np.array_equal(seg[eid] % L, segt % L)
    same = segt[1:] == segt[:-1]
    assert np.all(eid[1:][same] > eid[:-1][same])  # stable: forward-CSR order within a segment


@pytest.mark.parametrize("N,L", SHAPES)
def test_every_structural_condition_occurs(N, L):
    rowptr, colidx, c = _graph(N, L)
    assert c == gp.census(rowptr, colidx, L, N)
    for name in STRUCTURE:
        assert c[name] >= 1, (name, c)
    # a group of the last tile without a valid row exists unless the last tile's 8 groups all have one:
    # N % 64 = 57 is 7 full groups and one row, so there the count is 0 by geometry (S1b's point is the
    # other remainder: the one-row group is the tile's LAST wave, not its first)
    assert c["groups_without_valid_row"] == (7 if N % 64 == 1 else 0)
    assert N % 8 == 1 and c["groups_with_one_valid_row"] == 1
    # the named placements are there: the patterns' own lists, at every position class
    at = gp.placements(N)
    deg = np.diff(rowptr).reshape(N, L)
    for g in at["P0"]:
        assert deg[g * 8:(g + 1) * 8].sum() == 0
    assert deg[(gp.EMPTY_TILE + 1) * 64].sum() > 0
    for g in at["P1"]:
        assert deg[g * 8:g * 8 + 7].sum() == 0 and deg[g * 8 + 7].tolist() == [1] + [0] * (L - 1)
    for g in at["P2"]:
        assert deg[g * 8 + 1:(g + 1) * 8].sum() == 0 and deg[g * 8].tolist() == [0] * (L - 1) + [70]
    for g in at["P3"]:
        d = deg[g * 8:(g + 1) * 8]
        assert d[:, 0].tolist() == [64, 1, 0, 0, 0, 0, 0, 0] and d[:, 1].tolist() == [0] * 7 + [63]
        assert d[:, 2].tolist() == [128, 0, 0, 1, 0, 0, 0, 0] and d[:, 3:].sum() == 0
    for g in at["P4"]:
        d = deg[g * 8:(g + 1) * 8]
        assert np.all(d[:, 0] == 8) and np.all(d[:, 1] == 16) and d[:, 2:].sum() == 0
    for g, r in zip(at["P5"], at["P5_rows"]):
        assert deg[g * 8:(g + 1) * 8].sum() == 2048 and deg[r].max() == 2048
    for g, r in zip(at["P6"], at["P6_rows"]):
        d = deg[g * 8:(g + 1) * 8]
        assert deg[r].sum() == 2048 and deg[r].max() - deg[r].min() <= 1
        assert np.all(d.sum(1) <= 2048) and np.all(np.delete(d, r - g * 8, 0) >= 280)
    for g in at["P7"]:
        d = deg[g * 8:(g + 1) * 8]
        assert np.all(d[1::2] == 1) and d[0::2].sum() == 0
    for g in at["P8"]:
        for r in range(g * 8, (g + 1) * 8):
            assert deg[r].tolist() == [1, 1, 1] + [0] * (L - 3)
            assert colidx[rowptr[r * L]:rowptr[r * L + 3]].tolist() == [0, N - 1, r]
    q0 = gp.QUIET_GROUP * 8
    assert not np.any((colidx >= q0) & (colidx < q0 + 8))
    assert deg[N - 1].max() == 65 == deg[N - 1].sum()
    # ... so the transpose has an all-empty group (the quiet ids) and rows of in-degree 2048
    rpt, cit = gp.transpose_host(rowptr, colidx, L, N)
    assert rpt[q0 * L] == rpt[(q0 + 8) * L]


@pytest.mark.parametrize("N,L", SHAPES)
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_every_dropedge_condition_occurs(N, L, variant):
    """Which DropEdge conditions a variant can meet: p = 1 keeps nothing, so
    every populated list is all dropped and nothing else can happen; a fetch
    block without a kept entry (64 drops in a row) needs the high p, which is
    what that variant is for; 0 < p < 1 must show the other two."""
    rowptr, colidx, _ = _graph(N, L)
    p, seed, call, _ = VARIANTS[variant]
    c = gp.census(rowptr, colidx, L, N, (p, seed, call))
    populated = c["lists"] - c["total_zero"] - c["groups_without_valid_row"] * L
    if p == 1.0:
        assert c["list_all_dropped"] == populated
        assert c["row_all_dropped_between_kept_rows"] == 0 and c["empty_fetch_block_then_kept_entry"] == 0
        return
    assert 1 <= c["list_all_dropped"] < populated
    assert c["row_all_dropped_between_kept_rows"] >= 1
    if variant == "high_p":
        assert c["empty_fetch_block_then_kept_entry"] >= 1
        # and in a 2048-entry list, as designed (not only in P6's neighbours)
        from oracle import hash as ohash

        at = gp.placements(N)
        hit = 0
        for i, r in enumerate(at["P5_rows"]):
            e0, e1 = rowptr[r * L + i % L], rowptr[r * L + i % L + 1]
            assert e1 - e0 == 2048
            k = ohash.dropedge_keep(p, seed, call, np.arange(e0, e1, dtype=np.uint64)).reshape(32, 64).sum(1)
            live = np.nonzero(k)[0]
            hit += int((k[:live[-1]] == 0).sum()) if live.size else 0
        assert hit >= 1
