"""CPU: what the long-read score path adds without a device -- the timing struct keeps its size, the header documents
main_kernel_kind 23 / 24 and the DEBUG keys, and the host-side list of long pairs (wfahip_debug_score_long_list: the words and
the table wfahip_score_batch hands wfa_score_long_kernel) agrees with wfahip_pack_pairs."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCORE_MAX_LEN = 2047


def test_timing_size_and_header_text(built):
    from wfa_amd import _lib
    assert C.sizeof(_lib.Timing) == 72
    assert _lib.lib().wfahip_version() == 400
    hdr = open(os.path.join(ROOT, "include", "wfa_hip.h")).read()
    assert re.search(r"23 = wfa_score_long_kernel", hdr) and re.search(r"24 = wfa_score_long_kernel<MATRIX>", hdr)
    assert '"score_long_min"' in hdr and '"score_long_window_words"' in hdr
    assert "wfahip_debug_score_long_list" in _lib.EXPORTS


def _long_list(arrays):
    from wfa_amd import _lib
    blob, q_off, q_len, t_off, t_len = [np.ascontiguousarray(a) for a in arrays]
    words, table = C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint32)()
    n_words, n_listed = C.c_uint64(), C.c_uint64()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    L = _lib.lib()
    rc = L.wfahip_debug_score_long_list(vp(blob), vp(q_off), vp(q_len), vp(t_off), vp(t_len), len(q_len), C.byref(words), C.byref(n_words),
                                        C.byref(table), C.byref(n_listed))
    assert rc == _lib.OK
    w = np.ctypeslib.as_array(words, shape=(max(n_words.value, 1),))[:n_words.value].copy()
    t = np.ctypeslib.as_array(table, shape=(max(n_listed.value, 1), 8))[:n_listed.value].copy()
    L.wfahip_free(words), L.wfahip_free(table)
    return w, t


def test_long_list_agrees_with_pack_pairs(built):
    import wfa_amd
    rng = np.random.default_rng(21)
    lens = [(2047, 2047), (2048, 100), (100, 2048), (2049, 2049), (2047, 2048), (4096, 4096), (4112, 3000), (16, 2064), (5000, 1500),
            (1500, 5000), (1000, 1000), (2046, 17), (3001, 3007), (32, 32), (6400, 6399)]
    lens += [(int(rng.integers(1, 9000)), int(rng.integers(1, 9000))) for _ in range(40)]
    qs = [bytes(rng.choice(list(b"ACGT"), n).astype(np.uint8)) for n, _ in lens]
    ts = [bytes(rng.choice(list(b"ACGT"), m).astype(np.uint8)) for _, m in lens]
    # pairs the list must leave out: empty sides, and long pairs with a byte outside ACGT (packed but not listed)
    qs += [b"", b"ACGT" * 600, b"ACGT" * 300 + b"N" + b"ACGT" * 400, b"acgt" * 700]
    ts += [b"ACGT" * 600, b"", b"ACGT" * 700, b"ACGT" * 700]
    arrays = wfa_amd.make_blob(qs, ts)
    blob, q_off, q_len, t_off, t_len = arrays
    words, table = _long_list(arrays)
    is_long = [(len(q) > SCORE_MAX_LEN or len(t) > SCORE_MAX_LEN) and len(q) > 0 and len(t) > 0 for q, t in zip(qs, ts)]
    clean = [set(q) <= set(b"ACGT") and set(t) <= set(b"ACGT") for q, t in zip(qs, ts)]
    want_ids = [i for i in range(len(qs)) if is_long[i] and clean[i]]
    assert list(table[:, 3]) == want_ids and (table[:, 7] == 0).all()
    # the listed pairs alone, through wfahip_pack_pairs: the same words, sequence for sequence
    sub = wfa_amd.make_blob([qs[i] for i in want_ids], [ts[i] for i in want_ids])
    packed, q_woff, t_woff = wfa_amd.pack_pairs(*sub, n_threads=3)
    for j, i in enumerate(want_ids):
        for (lo, hi, ln), woff, seq in (((table[j, 0], table[j, 1], table[j, 2]), q_woff[j], qs[i]),
                                        ((table[j, 4], table[j, 5], table[j, 6]), t_woff[j], ts[i])):
            off, nw = int(lo) | int(hi) << 32, (len(seq) + 15) // 16 + 1
            assert int(ln) == len(seq)
            assert np.array_equal(words[off:off + nw], packed[int(woff):int(woff) + nw]), (i, len(seq))
            assert words[off + nw - 1] == 0  # the pad word
    # every long pair has its room in the buffer, listed or not, in batch order
    assert len(words) == sum((len(q) + 15) // 16 + 1 + (len(t) + 15) // 16 + 1 for q, t, lg in zip(qs, ts, is_long) if lg)
    offs = [int(r[0]) | int(r[1]) << 32 for r in table]
    assert offs == sorted(offs)


def test_long_list_of_a_short_batch_is_empty(built):
    import wfa_amd
    words, table = _long_list(wfa_amd.generate_pairs(seed=2, n_pairs=50, length=1000, error_rate=0.05))
    assert len(words) == 0 and len(table) == 0
