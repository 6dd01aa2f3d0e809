"""GPU: the byte-input packing pass alone (wfa_prepack_kernel in wfa_blk.hpp, through wfahip_debug_prepack), its slots word for word
against a NumPy packer written here, and end to end through wfahip_align_batch_device against the oracle.

A slot is {q_len, t_len, status, 0, SW query words, SW text words}: 16 bases a word, the first base in the low bits, code
(byte >> 1) & 3, 0 behind a sequence's end.  Status: 0xFFFFFFFF (to be aligned), 1 (an empty sequence), 102 (a sequence plus its pad
word does not fit SW words), 100 (a byte outside ACGT).  Only slots of status 0xFFFFFFFF and 100 hold words; the debug entry fills the
buffer with 0xA5 first, so a word the kernel must not store -- or fails to store -- reads 0xA5A5A5A5.  The reference is checked on
the CPU against wfa_amd.pack_pairs.

How the kernel maps words to lanes decides the shapes: lane l takes query word l and text word l of a round of 64 words; a remainder
of at most 32 words per sequence shares one fetch; a slot of at most 16 words per sequence puts two pairs side by side in a wave.  So:
SW 63 .. 67 with lengths either side of 1 008 and 1 024 bases (word 63 and word 64 appear), SW = 126 (two full rounds), SW = 11 (two
pairs a wave, odd pair counts), every alignment class of the blob offsets (16-byte, 4-byte, none) for query and text independently,
bytes outside ACGT in the first, the last and a word past 64, and pairs the kernel must leave alone between pairs it packs.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ST_PENDING, ST_EMPTY, ST_REDO_BYTES, ST_REDO_LDS = 0xFFFFFFFF, 1, 100, 102
POISON = 0xA5A5A5A5
LENGTHS = (1, 15, 16, 17, 1007, 1008, 1009, 1023, 1024, 1025, 1040)
FIELDS = ("score", "tbegin", "tend", "qbegin", "qend", "align_len", "matches", "gaps", "gap_regions", "ops_len")
AD = (10, 50, 1)


def _pack_seq(seq, words):
    """`words` packed words of a byte sequence"""
    codes = np.zeros(16 * words, dtype=np.uint64)
    codes[:len(seq)] = (seq.astype(np.uint64) >> 1) & 3
    return (codes.reshape(words, 16) << (2 * np.arange(16, dtype=np.uint64))).sum(axis=1).astype(np.uint32)


def ref_slots(blob, q_off, q_len, t_off, t_len, sw, work=None):
    """the NumPy packer: uint32 [n, 4 + 2 sw]"""
    ids = np.arange(len(q_len)) if work is None else np.asarray(work)
    out = np.full((len(ids), 4 + 2 * sw), POISON, dtype=np.uint32)
    acgt = np.zeros(256, dtype=bool)
    acgt[list(b"ACGT")] = True
    for s, p in enumerate(ids):
        n, m = int(q_len[p]), int(t_len[p])
        q, t = blob[int(q_off[p]):int(q_off[p]) + n], blob[int(t_off[p]):int(t_off[p]) + m]
        status = ST_PENDING
        if n == 0 or m == 0:
            status = ST_EMPTY
        elif (max(n, m) + 15) // 16 + 1 > sw:
            status = ST_REDO_LDS
        else:
            out[s, 4:4 + sw], out[s, 4 + sw:] = _pack_seq(q, sw), _pack_seq(t, sw)
            if not (acgt[q].all() and acgt[t].all()):
                status = ST_REDO_BYTES
        out[s, :4] = (n, m, status, 0)
    return out


def _layout(rng, lens, align=lambda k: 0, fill=b"ACGT"):
    """a blob with the sequences of `lens` (query, text, query, ...) one after the other, sequence k starting at a byte offset that is
    align(k) modulo 16; the last sequence ends on the blob's last byte.  Bytes between sequences are 'N'."""
    offs, pos = [], 0
    for k, n in enumerate(lens):
        pos += (align(k) - pos) % 16
        offs.append(pos)
        pos += n
    blob = np.full(pos, ord("N"), dtype=np.uint8)
    for o, n in zip(offs, lens):
        blob[o:o + n] = rng.choice(np.frombuffer(fill, dtype=np.uint8), n)
    off, ln = np.array(offs, dtype=np.uint64), np.array(lens, dtype=np.uint32)
    return blob, off[0::2].copy(), ln[0::2].copy(), off[1::2].copy(), ln[1::2].copy()


@functools.lru_cache(maxsize=None)
def _grid_batch():
    """every (query, text) combination of LENGTHS: shorter, equal and longer queries"""
    lens = [x for n in LENGTHS for m in LENGTHS for x in (n, m)]
    return _layout(np.random.default_rng(1400), lens)


@functools.lru_cache(maxsize=None)
def _batch_of(n_pairs, length, seed=1401):
    rng = np.random.default_rng(seed + n_pairs)
    lens = [int(x) for x in rng.integers(length - 6, length + 7, 2 * n_pairs)]
    return _layout(rng, lens)


def _to_dev(data):
    import torch
    blob, q_off, q_len, t_off, t_len = data
    t = lambda a, d: torch.from_numpy(np.ascontiguousarray(a).view(d).copy()).to("cuda:0")
    return t(blob, np.uint8), t(q_off, np.int64), t(q_len, np.int32), t(t_off, np.int64), t(t_len, np.int32)


@pytest.fixture(scope="module")
def al(built):
    import wfa_amd
    a = wfa_amd.New(wfa_amd.Penalties(4, 6, 2), wfa_amd.Options(GlobalAlignment=True), device=0)
    assert a.AdaptiveReduction(wfa_amd.AdaptiveReductionOption(*AD)) is None
    yield a
    a.close()


def _check(al, data, sw, ppw, work=None, what=""):
    import torch
    want = ref_slots(*data, sw, work)
    w = None if work is None else torch.from_numpy(np.asarray(work, dtype=np.int32)).to("cuda:0")
    got = al.debug_prepack(*_to_dev(data), sw, ppw, w)
    assert got.shape == want.shape
    bad = np.nonzero((got != want).any(axis=1))[0]
    if len(bad):
        s = int(bad[0])
        c = np.nonzero(got[s] != want[s])[0]
        raise AssertionError(f"{what} SW={sw} ppw={ppw}: {len(bad)} slots differ, first slot {s} header {got[s, :4]} / {want[s, :4]}, "
                             f"words {c[:8]} got {got[s, c[:8]]} want {want[s, c[:8]]}")
    return want


def test_reference_packer_against_pack_pairs(built):
    """pure-ACGT input: the NumPy packer's words are wfa_amd.pack_pairs' (ceil(len / 16) words and a pad word per sequence)"""
    import wfa_amd
    data = _grid_batch()
    blob, q_off, q_len, t_off, t_len = data
    packed, q_woff, t_woff = wfa_amd.pack_pairs(*data)
    sw = (max(LENGTHS) + 15) // 16 + 1
    want = ref_slots(*data, sw)
    assert (want[:, 2] == ST_PENDING).all()
    for i in range(len(q_len)):
        for woff, ln, base in ((q_woff, q_len, 4), (t_woff, t_len, 4 + sw)):
            nw = (int(ln[i]) + 15) // 16
            assert np.array_equal(want[i, base:base + nw], packed[int(woff[i]):int(woff[i]) + nw]), i
            assert not want[i, base + nw:base + sw].any()


@pytest.mark.parametrize("ppw", [1, 4])
@pytest.mark.parametrize("sw", [63, 64, 65, 66, 67])
def test_lengths_either_side_of_a_fetch(al, sw, ppw):
    """121 pairs, every combination of LENGTHS: at SW 63 .. 67 the words 63, 64 and 65 exist or not, in one sequence or both, and the
    pairs that do not fit the slot (status 102) lie between pairs that do"""
    want = _check(al, _grid_batch(), sw, ppw)
    assert (want[:, 2] == ST_REDO_LDS).sum() == sum((max(n, m) + 15) // 16 + 1 > sw for n in LENGTHS for m in LENGTHS)
    if sw >= 66:
        assert (want[:, 2] == ST_PENDING).sum() >= 100


@pytest.mark.parametrize("ppw", [1, 4])
def test_two_full_rounds(al, ppw):
    """1 985 and 2 000 bases at SW = 126: two rounds of 64 and 62 words per sequence"""
    lens = [x for n in (1985, 2000) for m in (1985, 2000) for x in (n, m)]
    want = _check(al, _layout(np.random.default_rng(1402), lens), 126, ppw)
    assert (want[:, 2] == ST_PENDING).all()


@pytest.mark.parametrize("ppw", [1, 4])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 17, 16 * 64 + 1])
def test_short_slots_two_pairs_a_wave(al, n, ppw):
    """150-base pairs at SW = 11: two pairs side by side in a wave; odd counts leave the last wave one pair on one side"""
    want = _check(al, _batch_of(n, 150), 11, ppw)
    assert (want[:, 2] == ST_PENDING).all()


@pytest.mark.parametrize("ppw", [1, 4])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 17, 16 * 64 + 1])
def test_pair_counts(al, n, ppw):
    """1 kbp pairs at SW = 66 (texts a few bases either side of the queries): the last wave holds one to four pairs"""
    want = _check(al, _batch_of(n, 1000), 66, ppw)
    assert (want[:, 2] == ST_PENDING).all()


@pytest.mark.parametrize("sw,length", [(66, 1000), (67, 1034), (11, 150), (24, 300)])
def test_work_list_in_shuffled_order(al, sw, length):
    """slot i is pair work[i]: a shuffled list, and one that names some pairs twice and others not at all"""
    data = _batch_of(41, length)
    rng = np.random.default_rng(1403)
    for work in (rng.permutation(41), rng.integers(0, 41, 23)):
        for ppw in (1, 4):
            _check(al, data, sw, ppw, work.astype(np.int32), "work list")


@pytest.mark.parametrize("sw,length", [(66, 1000), (67, 1034), (11, 150), (24, 300)])
def test_blob_offsets(al, sw, length):
    """offsets with off & 15 in {0, 1, 3, 4, 8, 15} for query and text independently (36 pairs, then four aligned ones, so that a wave
    of four pairs is aligned throughout, mixed, and unaligned throughout); the last sequence ends on the blob's last byte"""
    cls = (0, 1, 3, 4, 8, 15)
    rng = np.random.default_rng(1404 + sw)
    al_of = [a for q in cls for t in cls for a in (q, t)] + [0] * 8
    lens = [int(x) for x in rng.integers(length - 6, length + 7, len(al_of))]
    data = _layout(rng, lens, lambda k: al_of[k])
    assert int(data[3][-1]) + int(data[4][-1]) == len(data[0])
    for ppw in (1, 4):
        want = _check(al, data, sw, ppw, what="offsets")
        assert (want[:, 2] == ST_PENDING).all()
    # ... and an unaligned last sequence that ends there
    al_of[-1] = 5
    data = _layout(rng, lens, lambda k: al_of[k])
    assert int(data[3][-1]) + int(data[4][-1]) == len(data[0]) and int(data[3][-1]) % 16 == 5
    _check(al, data, sw, 4, what="offsets")


@pytest.mark.parametrize("ppw", [1, 4])
@pytest.mark.parametrize("sw,length", [(66, 1040), (67, 1040), (11, 150)])
def test_bytes_outside_acgt(al, sw, length, ppw):
    """'N', a lowercase base and 0x00 as the first base, as the last base and -- at 1 040 bases -- in word 64 of the query or of the
    text: status 100 for exactly those pairs (every third pair of the batch), and the words as packed from the bytes"""
    rng = np.random.default_rng(1405)
    spots = [("q", 0), ("q", -1), ("t", 0), ("t", -1)] + ([("q", 1030), ("t", 1027), ("q", 1024), ("t", 1039)] if length > 1024 else [])
    cases = [(s, p, b) for (s, p) in spots for b in (ord("N"), ord("a"), 0)]
    n = 3 * len(cases) + 2
    data = _layout(rng, [length] * (2 * n), lambda k: (k % 5) if length < 200 else 0)
    blob, q_off, q_len, t_off, t_len = data
    hit = set()
    for c, (s, p, b) in enumerate(cases):
        i = 3 * c + 1
        off, ln = (q_off, q_len) if s == "q" else (t_off, t_len)
        blob[int(off[i]) + (p if p >= 0 else int(ln[i]) - 1)] = b
        hit.add(i)
    want = _check(al, data, sw, ppw, what="bytes")
    assert {int(i) for i in np.nonzero(want[:, 2] == ST_REDO_BYTES)[0]} == hit
    assert (want[:, 2] == ST_PENDING).sum() == n - len(hit)


@pytest.mark.parametrize("ppw", [1, 4])
@pytest.mark.parametrize("sw,length", [(66, 1000), (11, 150)])
def test_pairs_the_kernel_leaves_alone(al, sw, length, ppw):
    """an empty query, an empty text and a pair too long for the slot in the middle of a wave's four pairs (and side by side in a wave
    of short slots): their status and lengths are stored, their words are not, and their neighbours are packed"""
    rng = np.random.default_rng(1406)
    too_long = 16 * (sw - 1) + 1
    lens = []
    for k in range(13):
        n, m = (length, length + k % 3)
        if k % 4 == 1:
            n, m = [(0, length), (length, 0), (too_long, length)][(k // 4) % 3]
        elif k % 4 == 2:
            n, m = [(length, too_long), (0, 0), (length, 0)][(k // 4) % 3]
        lens += [n, m]
    want = _check(al, _layout(rng, lens), sw, ppw, what="left alone")
    st = want[:, 2]
    assert (st == ST_EMPTY).sum() == 4 and (st == ST_REDO_LDS).sum() == 2 and (st == ST_PENDING).sum() == 7
    assert (want[st != ST_PENDING, 4:] == POISON).all()


def test_refused_without_the_environment_switch(al):
    """a debug entry like the debug options: WFAHIP_ERR_UNSUPPORTED unless WFAHIP_DEBUG=1 is in the environment"""
    import os
    from wfa_amd._lib import WfaHipError
    dev = _to_dev(_batch_of(3, 150))
    saved = os.environ.pop("WFAHIP_DEBUG", None)
    try:
        with pytest.raises(WfaHipError):
            al.debug_prepack(*dev, 11, 4)
        os.environ["WFAHIP_DEBUG"] = "1"
        al.debug_prepack(*dev, 11, 4)
    finally:
        if saved is None:
            os.environ.pop("WFAHIP_DEBUG", None)
        else:
            os.environ["WFAHIP_DEBUG"] = saved


# ---- end to end: the consumers see the same slots

@functools.lru_cache(maxsize=None)
def _e2e(kind):
    """1k: 66 pairs whose queries have the lengths of LENGTHS from 1 007 on, texts at 3 % error; short: 33 pairs of 150 bases"""
    import wfa_amd
    if kind == "short":
        data = wfa_amd.generate_pairs(seed=1407, n_pairs=33, length=150, error_rate=0.04, n_threads=2)
    else:
        parts = [wfa_amd.generate_pairs(seed=1408 + L, n_pairs=6, length=L, error_rate=0.03, n_threads=2) for L in LENGTHS if L > 1000]
        base = np.concatenate([[0], np.cumsum([len(p[0]) for p in parts])]).astype(np.uint64)
        data = (np.concatenate([p[0] for p in parts]),) + tuple(
            np.concatenate([p[j] + (base[k] if j in (1, 3) else 0) for k, p in enumerate(parts)]).astype(parts[0][j].dtype) for j in (1, 2, 3, 4))
    from oracle import oracle as O
    want = O.align_batch(O.make_params(4, 6, 2, global_alignment=True, adaptive=AD), *data, n_threads=4)
    return data, want


@pytest.mark.parametrize("kind", ["1k", "short"])
def test_end_to_end_device_entry(al, kind):
    """wfahip_align_batch_device on bytes, wfa_duo_kernel forced on the small batch (option duo = 2; short reads: duo_short = 2): records
    and CIGAR ops of every pair are the oracle's"""
    data, want = _e2e(kind)
    blob = np.concatenate([data[0], np.zeros(64, dtype=np.uint8)])
    al.set_option("duo", 2)
    al.set_option("duo_short", 2 if kind == "short" else 0)
    try:
        rec, ops = al.align_tensors(*_to_dev((blob,) + tuple(data[1:])))
        assert al.last_timing().main_kernel_kind == 8
    finally:
        al.set_option("duo", 1)
        al.set_option("duo_short", 0)
    rec, ops = rec.cpu().numpy().view(np.uint32), ops.cpu().numpy().view(np.uint64)
    assert np.array_equal(rec[:, 0].astype(np.int64), want.status.astype(np.int64)) and not want.status.any()
    for c, f in enumerate(FIELDS):
        a, b = rec[:, 1 + c].view(np.int32).astype(np.int64), np.asarray(getattr(want, f)).astype(np.int64)
        assert np.array_equal(a, b), f"field {f} differs at pairs {np.nonzero(a != b)[0][:8]}"
    for i in range(len(want.status)):
        o = int(rec[i, 11]) | (int(rec[i, 12]) << 32)
        assert np.array_equal(ops[o:o + int(rec[i, 10])], np.asarray(want.pair_ops(i), dtype=np.uint64)), i
