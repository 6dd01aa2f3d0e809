"""GPU: the plan kernels of the semi-global router (wfa_amd/csrc/wfa_wide_plan.hpp: count per tile, scan of the tile counts, scatter)
through Aligner.debug_wide_plan, against a numpy classifier written here from wide_class_bounds().  Lengths only, no alignment."""
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_SEQ_LEN = (1 << 29) - 1  # WFAHIP_MAX_SEQ_LEN


def _kernel_constants():
    """WP_BLOCK, WP_ITEMS of the plan kernels, from their header: a tile is their product, and the scan kernel takes the tile counts
    WP_BLOCK at a time"""
    src = open(os.path.join(ROOT, "wfa_amd", "csrc", "wfa_wide_plan.hpp")).read()
    m = re.search(r"WP_BLOCK = (\d+), WP_ITEMS = (\d+), WP_TILE = WP_BLOCK \* WP_ITEMS;", src)
    assert m, "the plan kernels' tile constants"
    return int(m.group(1)), int(m.group(2))


def _classify(bounds, q_len, t_len):
    """(lists, counts, longest, ladder): what the plan must give"""
    q, t = q_len.astype(np.int64), t_len.astype(np.int64)
    valid = (q > 0) & (t > 0) & (q <= MAX_SEQ_LEN) & (t <= MAX_SEQ_LEN)
    longer = np.maximum(q, t)
    ladder = valid & (longer > bounds[-1])
    cls = np.searchsorted(np.array(bounds), longer, side="left")  # the first class whose bound is >= the longer read
    cls = np.where(valid, cls, 0)
    lists, counts, longest = [], [], []
    for c in range(len(bounds)):
        ids = np.nonzero(~ladder & (cls == c))[0]
        lists.append(ids.astype(np.uint32)), counts.append(len(ids))
        ok = ids[valid[ids]]
        longest.append(int(longer[ok].max()) if len(ok) else 0)
    return lists, counts, longest, np.nonzero(ladder)[0].astype(np.uint32)


def _edge_lengths(bounds):
    vals = [0, 1, 2047, 2048, MAX_SEQ_LEN, MAX_SEQ_LEN + 1, 9000, 100000]
    for b in bounds:
        vals += [b - 1, b, b + 1]
    return vals


def _lengths(bounds, n, seed):
    """n pairs: every edge length against every other in the first pairs (query long with target short and the reverse among
    them), then a random mix of classes, edge values, long reads, empty and over-long sequences"""
    rng = np.random.default_rng(seed)
    edges = np.array(_edge_lengths(bounds), dtype=np.uint64)
    grid_q, grid_t = [a.ravel() for a in np.meshgrid(edges, edges)]
    q = rng.integers(1, bounds[-1] + 600, n).astype(np.uint64)
    t = np.clip(q.astype(np.int64) + rng.integers(-40, 41, n), 0, None).astype(np.uint64)
    pick = rng.random(n)
    q = np.where(pick < 0.15, edges[rng.integers(0, len(edges), n)], q)
    t = np.where((pick > 0.1) & (pick < 0.25), edges[rng.integers(0, len(edges), n)], t)
    k = min(n, len(grid_q))
    at = rng.permutation(n)[:k]  # (scattered over the batch: every tile, wave and round sees some)
    q[at], t[at] = grid_q[:k], grid_t[:k]
    return q.astype(np.uint32), t.astype(np.uint32)


def _check(al, bounds, q_len, t_len, what):
    lists, counts, longest, ladder = al.debug_wide_plan(q_len, t_len)
    w_lists, w_counts, w_longest, w_ladder = _classify(bounds, q_len, t_len)
    assert counts == w_counts and len(ladder) == len(w_ladder), (what, counts, w_counts, len(ladder), len(w_ladder))
    assert longest == w_longest, (what, longest, w_longest)
    for c in range(len(bounds)):
        assert np.array_equal(lists[c], w_lists[c]), (what, c)
        assert np.all(np.diff(lists[c].astype(np.int64)) > 0), (what, c)
    assert np.array_equal(ladder, w_ladder) and np.all(np.diff(ladder.astype(np.int64)) > 0), what
    everything = np.concatenate(lists + [ladder])
    assert np.array_equal(np.sort(everything), np.arange(len(q_len), dtype=np.uint32)), what  # a partition of range(n)


def test_plan_against_numpy(built):
    import wfa_amd as w
    bounds = w.wide_class_bounds()
    block, items = _kernel_constants()
    tile = block * items
    al = w.New(w.DefaultPenalties, w.Options(GlobalAlignment=False), device=0)
    # one block minus one pair; three blocks plus seven; more tiles than the scan kernel takes in one round (twice its width, and a
    # partial tile); and a few sizes around a wave and a tile
    sizes = [tile - 1, 3 * tile + 7, (2 * block + 1) * tile + 13, 1, 63, 64, 65, tile, tile + 1]
    for j, n in enumerate(sizes):
        q_len, t_len = _lengths(bounds, n, 1000 + j)
        _check(al, bounds, q_len, t_len, f"n={n}")
    # the edge grid alone, in order: every bound at b - 1, b, b + 1, 0, 1, 2 047 / 2 048, the longest valid length and one over it
    edges = np.array(_edge_lengths(bounds), dtype=np.uint32)
    gq, gt = [a.ravel() for a in np.meshgrid(edges, edges)]
    _check(al, bounds, gq, gt, "edge grid")
    # one class only, the ladder only, invalid pairs only
    n = 2 * tile + 5
    _check(al, bounds, np.full(n, bounds[0], np.uint32), np.full(n, 1, np.uint32), "smallest class only")
    _check(al, bounds, np.full(n, 2048, np.uint32), np.full(n, 3, np.uint32), "ladder only")
    _check(al, bounds, np.zeros(n, np.uint32), np.full(n, 2048, np.uint32), "empty queries only")
    al.close()
