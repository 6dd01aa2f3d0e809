"""GPU: wfa_duo_kernel's packed rings (16-bit pairs, the default) against its 32-bit-ring reference wfa_duo32_kernel
(debug option duo_pk = 0).  The same batch through both: every arena word of every pair the kernel finished (absent
cells included; _canon() says what may differ between any two runs), every record field and every CIGAR op; and a sample
against the oracle."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FIELDS = ("score", "tbegin", "tend", "qbegin", "qend", "align_len", "matches", "gaps", "gap_regions", "ops_len")
# one penalty set of every shape wfa_duo_kernel is instantiated for (x/g : (o+e)/g, e == g; KERNELS.md 4e)
SHAPES = ((4, 6, 2), (2, 4, 2), (1, 1, 1), (4, 4, 2), (4, 2, 2), (6, 4, 2))


def _aligner(pen, ad, pk):
    import wfa_amd as w
    al = w.New(w.Penalties(*pen), w.Options(GlobalAlignment=True), device=0)
    if ad is not None:
        assert al.AdaptiveReduction(w.AdaptiveReductionOption(*ad)) is None
    al.set_option("duo", 2)
    al.set_option("arena_poison", 1)  # (words a kernel did not write compare equal only if both start from the same pattern)
    al.set_option("duo_pk", pk)
    return al


def _ragged(length, err, n, seed):
    import wfa_amd as w
    blob, q_off, q_len, t_off, t_len = w.generate_pairs(seed=seed, n_pairs=n, length=length, error_rate=err, n_threads=8)
    rng = np.random.default_rng(seed)
    cut = rng.integers(0, 3, n) == 0  # a third of the pairs lose a piece of one sequence: overhangs, early sequence ends
    q_len = np.where(cut & (np.arange(n) % 2 == 0), np.maximum(1, q_len - rng.integers(1, 60, n)), q_len).astype(np.uint32)
    t_len = np.where(cut & (np.arange(n) % 2 == 1), np.maximum(1, t_len - rng.integers(1, 60, n)), t_len).astype(np.uint32)
    return blob, q_off, q_len, t_off, t_len


def _run(pen, ad, pk, data, sample):
    al = _aligner(pen, ad, pk)
    got = al.align_arrays(*data)
    assert al.last_timing().main_kernel_kind == 8
    slots = {}
    from wfa_amd._lib import WfaHipError
    for i in sample:
        try:
            words, f, meta = al.debug_compact_arena(int(i))
        except WfaHipError:  # (a batch of several chunks: only the last chunk's arena is kept)
            continue
        assert f == 10
        slots[int(i)] = (words, meta)
    al.close()
    return got, slots


def _assert_same(got, ref, what):
    assert np.array_equal(got.status, ref.status), what
    for f in FIELDS:
        a, b = getattr(got, f), getattr(ref, f)
        assert np.array_equal(a, b), f"{what}: field {f} differs at pairs {np.nonzero(a != b)[0][:5]}"
    for i in range(len(got.status)):
        assert np.array_equal(got.pair_ops(i), ref.pair_ops(i)), f"{what}: CIGAR differs at pair {i}"


def _canon(words):
    """The arena words as the backtrace reads them.  Which pairs share a wave depends on the order the waves claim the queue,
    and a wave steps WF_NEXT's exact path (rejections near a sequence end) when any of its pairs needs it: the two paths write
    the same offsets and decisions but differ in two bits the backtrace never reads -- fromI next to a set fromX (the exact path
    clears it), and an absent cell (3 on the rejection-free path, 1 on the exact one).  Two runs of the same kernel differ the
    same way; everything else must match byte for byte."""
    w = words.view(np.uint16)
    w = np.where(w == 3, 1, w).astype(np.uint16)
    return np.where((w & 2) != 0, w & ~np.uint16(1), w).astype(np.uint16)


def _compare(pen, ad, data, sample, what):
    ref, ref_slots = _run(pen, ad, 0, data, sample)
    got, got_slots = _run(pen, ad, 1, data, sample)
    _assert_same(got, ref, what)
    assert got_slots.keys() == ref_slots.keys() and len(ref_slots) > 0, what
    done = 0
    for i in ref_slots:
        (w1, m1), (w0, m0) = got_slots[i], ref_slots[i]
        assert m1 == m0, (what, i, m1, m0)
        if m0[0] != 0:  # handed on to another kernel: not the kernel's final state
            continue
        assert len(w1) == len(w0) and np.array_equal(_canon(w1), _canon(w0)), f"{what}: arena of pair {i} differs"
        done += 1
    # (wf-adaptive off: most bands outgrow a whole row and are handed on to the 256-diagonal rung)
    assert done >= (len(ref_slots) // 2 if ad is not None else 0), (what, done, len(ref_slots))
    return got


def _oracle_sample(got, pen, ad, data, idx, what):
    from oracle import oracle as O
    blob, q_off, q_len, t_off, t_len = data
    want = O.align_batch(O.make_params(*pen, global_alignment=True, adaptive=ad), blob, q_off[idx], q_len[idx], t_off[idx],
                         t_len[idx], n_threads=8)
    assert np.array_equal(got.status[idx], want.status), what
    for f in FIELDS:
        assert np.array_equal(getattr(got, f)[idx], getattr(want, f)), (what, f)
    for j, i in enumerate(idx):
        assert np.array_equal(got.pair_ops(int(i)), want.pair_ops(j)), (what, int(i))


@pytest.mark.parametrize("ad", [(10, 50, 1), None])
@pytest.mark.parametrize("pen", SHAPES)
@pytest.mark.parametrize("length,err", [(260, 0.06), (1000, 0.05), (1950, 0.03)])
def test_duo_packed_matches_32bit(built, length, err, pen, ad):
    n = 700
    data = _ragged(length, err, n, seed=length + 31 * pen[0] + 7 * pen[1] + (0 if ad else 1))
    what = f"L={length} pen={pen} ad={ad}"
    got = _compare(pen, ad, data, np.arange(n), what)
    _oracle_sample(got, pen, ad, data, np.arange(0, n, 23), what)


def test_duo_packed_large_batch(built):
    """2e5 pairs: every wave parks, resumes, widens and narrows many times.  Records and CIGARs of all pairs, the arena
    of a sample, the oracle on part of it."""
    n, pen, ad = 200000, (4, 6, 2), (10, 50, 1)
    data = _ragged(1000, 0.05, n, seed=77)
    sample = np.unique(np.concatenate([np.arange(0, n, 97), np.arange(n - 2000, n)]))  # (the arena kept is the last chunk's)
    got = _compare(pen, ad, data, sample, "2e5 x 1 kbp")
    _oracle_sample(got, pen, ad, data, sample[::8], "2e5 x 1 kbp")
