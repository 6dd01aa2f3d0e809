"""GPU: wfahip_score_matrix (every query against every target, score only) returns, cell for cell, what the oracle and
wfahip_score_batch give on the expanded pairs -- global and semi-global, wf-adaptive on and off, edge sequences, the max_score
bound, a penalty shape without an instance, tiles that split rows and columns, strided output -- and the matrix kernels, not
the full path, do the work."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = [(g, a) for g in (True, False) for a in ((10, 50, 1), None)]


def _aligner(glob, adaptive, pen=(4, 6, 2)):
    import wfa_amd
    al = wfa_amd.New(wfa_amd.Penalties(*pen), wfa_amd.Options(GlobalAlignment=glob), device=0)
    if adaptive is not None:
        assert al.AdaptiveReduction(wfa_amd.AdaptiveReductionOption(*adaptive)) is None
    return al


def _mutate(rng, s, rate):
    out = bytearray()
    for c in s:
        r = rng.random()
        if r < rate / 3:
            out.append(b"ACGT"[rng.integers(4)])  # substitution
        elif r < 2 * rate / 3:
            continue  # deletion
        elif r < rate:
            out += bytes([c, b"ACGT"[rng.integers(4)]])  # insertion
        else:
            out.append(c)
    return bytes(out)


def _families(seed, n_fam, k, length, rate):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_fam):
        anc = bytes(rng.choice(list(b"ACGT"), length).astype(np.uint8))
        out += [_mutate(rng, anc, rate) for _ in range(k)]
    return out


def _mixed(seed, n):
    """n sequences of 1 .. 700 bases: members of a few families (prefixes of varying length) and unrelated ones."""
    rng = np.random.default_rng(seed)
    anc = [bytes(rng.choice(list(b"ACGT"), 700).astype(np.uint8)) for _ in range(3)]
    out = []
    for i in range(n):
        ln = int(rng.integers(1, 701))
        if i % 3 == 2:
            out.append(bytes(rng.choice(list(b"ACGT"), ln).astype(np.uint8)))
        else:
            out.append(_mutate(rng, anc[i % 3][:ln], 0.05) or b"A")
    return out


def _expand(qs, ts):
    import wfa_amd
    return wfa_amd.make_blob([q for q in qs for _ in ts], [t for _ in qs for t in ts])


def _want_batch(al, qs, ts, max_score=0):
    st, sc = al.score_arrays(*_expand(qs, ts), max_score=max_score)
    return st.reshape(len(qs), len(ts)), sc.reshape(len(qs), len(ts))


@pytest.mark.parametrize("glob,adaptive", MODES)
def test_small_sets_match_oracle(glob, adaptive):
    qs, ts = _mixed(1, 24), _mixed(2, 31)
    al = _aligner(glob, adaptive)
    st, sc = al.ScoreMatrix(qs, ts)
    want = O.align_batch(O.make_params(4, 6, 2, global_alignment=glob, adaptive=adaptive), *_expand(qs, ts), n_threads=16, want_ops=False)
    assert np.array_equal(st.ravel(), want.status)
    assert np.array_equal(sc.ravel(), np.where(want.status == 0, want.score, 0).astype(np.uint32))
    assert al.last_timing().main_kernel_kind == (21 if glob else 22)


@pytest.mark.parametrize("glob,adaptive", MODES)
def test_matrix_kernels_do_the_work(glob, adaptive):
    seqs = _families(14, 1, 40, 300, 0.05)  # (one family: an unrelated pair's band outgrows wfa_score_kernel's 248 diagonals without wf-adaptive)
    al = _aligner(glob, adaptive)
    st, sc = al.ScoreMatrix(seqs[:17], seqs[17:])
    t = al.last_timing()
    assert t.main_kernel_kind == (21 if glob else 22) and t.n_retried_pairs == 0 and t.arena_bytes == 0
    wst, wsc = _want_batch(al, seqs[:17], seqs[17:])
    assert np.array_equal(st, wst) and np.array_equal(sc, wsc)
    if adaptive is not None:
        # launch accounting: 8 x 8 sequences of 1 kbp in tiles of 16 cells are four tiles -- a launch each on wfa_score_kernel, two on
        # the wide kernel under wf-adaptive (its two phases count as one main launch)
        kbp = _families(16, 1, 16, 1000, 0.05)
        al.set_option("matrix_tile_cells", 16)
        al.ScoreMatrix(kbp[:8], kbp[8:])
        t = al.last_timing()
        print("launches", glob, "retried", t.n_retried_pairs, (t.main_kernel_kind, t.n_launches, t.n_main_launches))
        assert t.n_retried_pairs == 0
        assert (t.main_kernel_kind, t.n_launches, t.n_main_launches) == ((21, 4, 4) if glob else (22, 8, 4))


@pytest.mark.parametrize("glob", [True, False])
def test_edge_sequences(glob):
    import wfa_amd
    rng = np.random.default_rng(3)
    long_read = bytes(rng.choice(list(b"ACGT"), 2300).astype(np.uint8))
    base = _mixed(4, 6)
    qs = base[:3] + [b"", b"ACGTNACGTACGT", long_read, b"acgtACGTACGTAAAC"]
    ts = base[3:] + [long_read[:2000] + b"ACGTAC", b"ACGTACGTNN", b"", b"ACGTACGTACGTAAAC"]
    odd_q = {4, 5, 6}  # non-ACGT bytes or longer than the kernels take
    odd_t = {4}
    al = _aligner(glob, (10, 50, 1))
    st, sc = al.ScoreMatrix(qs, ts)
    wst, wsc = _want_batch(al, qs, ts)
    assert np.array_equal(st, wst) and np.array_equal(sc, wsc)
    assert (st[3, :] == wfa_amd._lib.PAIR_EMPTY).all() and (st[:, 5] == wfa_amd._lib.PAIR_EMPTY).all()
    batch_retried = al.last_timing().n_retried_pairs  # (the same cells: the same kernels' decisions, pair by pair)
    st, sc = al.ScoreMatrix(qs, ts)
    empty_q, empty_t = 3, 5
    odd = sum(1 for i in range(len(qs)) for j in range(len(ts)) if i != empty_q and j != empty_t and (i in odd_q or j in odd_t))
    assert al.last_timing().n_retried_pairs == batch_retried >= odd
    # family members of 300 bases and odd copies of them: exactly the non-empty cells of an odd sequence go to the full path
    fam = _families(15, 1, 8, 300, 0.05)
    qs2 = fam[:3] + [fam[3][:100] + b"N" + fam[3][101:], fam[4].lower(), long_read]
    ts2 = fam[5:8] + [fam[3][:50] + b"NN" + fam[3][52:], b""]
    st, sc = al.ScoreMatrix(qs2, ts2)
    assert al.last_timing().n_retried_pairs == 3 * 4 + 3 * 1
    wst, wsc = _want_batch(al, qs2, ts2)
    assert np.array_equal(st, wst) and np.array_equal(sc, wsc)


@pytest.mark.parametrize("glob", [True, False])
def test_max_score_bound(glob):
    import wfa_amd
    qs, ts = _mixed(5, 12), _mixed(6, 9)
    al = _aligner(glob, (10, 50, 1))
    _, sc0 = al.ScoreMatrix(qs, ts)
    live = sc0[sc0 > 0]
    for bound in (1, int(np.min(live)), int(np.median(live)), int(np.max(live)), int(np.max(live)) + 1):
        st, sc = al.ScoreMatrix(qs, ts, max_score=bound)
        wst, wsc = _want_batch(al, qs, ts, max_score=bound)
        assert np.array_equal(st, wst) and np.array_equal(sc, wsc), bound
        assert ((st == wfa_amd._lib.PAIR_OVER_MAX) == (sc0 > bound)).all()


@pytest.mark.parametrize("glob", [True, False])
def test_shape_without_instance_takes_full_path(glob):
    qs, ts = _mixed(7, 5), _mixed(8, 7)
    al = _aligner(glob, (10, 50, 1), pen=(3, 5, 2))
    st, sc = al.ScoreMatrix(qs, ts)
    t = al.last_timing()
    wst, wsc = _want_batch(al, qs, ts)
    assert np.array_equal(st, wst) and np.array_equal(sc, wsc)
    assert t.n_retried_pairs == len(qs) * len(ts) and t.main_kernel_kind not in (21, 22)


@pytest.mark.parametrize("glob", [True, False])
def test_tiles_stride_and_thin_shapes(glob):
    qs, ts = _mixed(9, 13), _mixed(10, 17)
    al = _aligner(glob, (10, 50, 1))
    wst, wsc = _want_batch(al, qs, ts)
    al.set_option("matrix_tile_cells", 5)  # tiles of 1 x 5: every row and every column split
    st, sc = al.ScoreMatrix(qs, ts)
    assert np.array_equal(st, wst) and np.array_equal(sc, wsc)
    assert al.last_timing().n_main_launches == len(qs) * 4
    # a window of a larger sentinel-filled matrix
    big_st, big_sc = np.full((20, 40), -5, np.int32), np.full((20, 40), 0xDEADBEEF, np.uint32)
    import wfa_amd
    blob, off, ln, _, _ = wfa_amd.make_blob(qs + ts, [b""] * (len(qs) + len(ts)))
    al.score_matrix_arrays(blob, off[:13], ln[:13], off[13:], ln[13:], out=(big_st[3:16, 7:24], big_sc[3:16, 7:24]))
    assert np.array_equal(big_st[3:16, 7:24], wst) and np.array_equal(big_sc[3:16, 7:24], wsc)
    mask = np.ones((20, 40), bool)
    mask[3:16, 7:24] = False
    assert (big_st[mask] == -5).all() and (big_sc[mask] == 0xDEADBEEF).all()
    al.set_option("matrix_tile_cells", 0)
    for qq, tt in (([qs[0]], ts), (qs, [ts[0]])):
        st, sc = al.ScoreMatrix(qq, tt)
        w1, w2 = _want_batch(al, qq, tt)
        assert st.shape == (len(qq), len(tt)) and np.array_equal(st, w1) and np.array_equal(sc, w2)


@pytest.mark.parametrize("glob", [True, False])
def test_all_against_all(glob):
    qs = _families(11, 4, 6, 400, 0.05) + _mixed(12, 6)
    al = _aligner(glob, (10, 50, 1))
    st, sc = al.ScoreMatrix(qs)
    st2, sc2 = al.ScoreMatrix(qs, qs)
    assert np.array_equal(st, st2) and np.array_equal(sc, sc2)
    dst, dsc = al.ScoreBatch(qs, qs)
    assert np.array_equal(np.diag(st), dst) and np.array_equal(np.diag(sc), dsc)


@pytest.mark.parametrize("glob", [True, False])
def test_larger_set_matches_score_batch(glob):
    seqs = _families(13, 14, 50, 1000, 0.05)
    qs, ts = seqs[:300], seqs[300:700]
    al = _aligner(glob, (10, 50, 1))
    st, sc = al.ScoreMatrix(qs, ts)
    t = al.last_timing()
    assert t.main_kernel_kind == (21 if glob else 22)
    wst, wsc = _want_batch(al, qs, ts)
    assert al.last_timing().n_retried_pairs == t.n_retried_pairs
    assert np.array_equal(st, wst) and np.array_equal(sc, wsc)


def test_cli_score_matrix(tmp_path):
    pairs = [(b"ACCATACTCG", b"AGGATGCTCG"), (b"ACGTACGTAC", b"ACGTACGTAC"), (b"TTTTACGT", b"ACGTTTTT")]
    f = tmp_path / "pairs.txt"
    f.write_bytes(b"".join(b">" + q + b"\n<" + t + b"\n" for q, t in pairs))
    r = subprocess.run([sys.executable, "-m", "wfa_amd.cli", "-S", "-i", str(f)], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    al = _aligner(True, (10, 50, 1))
    _, want = _want_batch(al, [p[0] for p in pairs], [p[1] for p in pairs])
    assert r.stdout == "".join("\t".join(str(int(v)) for v in row) + "\n" for row in want)
    assert r.stdout.splitlines()[0].split("\t")[0] == "12"  # the README pair
