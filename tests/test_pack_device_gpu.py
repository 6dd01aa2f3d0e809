"""GPU: wfahip_pack_pairs_device against the host packer wfahip_pack_pairs -- word for word, woff for woff, n_words equal.  Every call
goes through the sizing protocol first (WFAHIP_ERR_OOM with the total and the offsets, d_packed = NULL), then into a buffer pre-filled
with 0xA5A5A5A5 whose words behind the total must survive; the inputs must come back bit for bit."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
MAX_SEQ_LEN = (1 << 29) - 1
FILL = 0xA5A5A5A5
SLACK = 8


@pytest.fixture(scope="module")
def al():
    import wfa_amd
    a = wfa_amd.New(wfa_amd.Penalties(4, 6, 2), wfa_amd.Options(GlobalAlignment=True), device=0)
    yield a
    a.close()


def _words(ln):
    ln = np.asarray(ln, np.uint64)
    ln = np.where(ln > MAX_SEQ_LEN, 0, ln)
    return (ln + 15) // 16 + 1


def _host_pack(blob, q_off, q_len, t_off, t_len):
    """wfahip_pack_pairs itself: (rc, packed, q_woff, t_woff, n_words)"""
    from wfa_amd import _lib
    n = len(q_len)
    total = int(_words(q_len).sum() + _words(t_len).sum())
    packed = np.full(total + 1, FILL, np.uint32)
    qw, tw, nw = np.zeros(n, np.uint64), np.zeros(n, np.uint64), C.c_uint64()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = _lib.lib().wfahip_pack_pairs(vp(blob), vp(q_off), vp(q_len), vp(t_off), vp(t_len), n, 4, vp(packed), vp(qw), vp(tw), C.byref(nw))
    assert nw.value == total and packed[total] == FILL
    return rc, packed[:total], qw, tw, total


def _dev(a, dt):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(dt).copy()).to("cuda:0")


def _dev_pack(al, blob, q_off, q_len, t_off, t_len, stream=None, want_rc=0):
    """the device packer through the raw entry: sizing call, then the real one.  Returns (rc, packed words, q_woff, t_woff, n_words)
    after checking what holds whatever the input: the sentinels, the untouched inputs, the sizing call's answers"""
    import torch
    from wfa_amd import _lib
    f = _lib.lib().wfahip_pack_pairs_device
    n = len(q_len)
    ins_h = (blob, q_off, q_len, t_off, t_len)
    ins = [_dev(blob, np.uint8), _dev(q_off, np.int64), _dev(q_len, np.int32), _dev(t_off, np.int64), _dev(t_len, np.int32)]
    qw = torch.full((n,), -1, dtype=torch.int64, device="cuda:0")
    tw = torch.full((n,), -1, dtype=torch.int64, device="cuda:0")
    nw = C.c_uint64(12345)
    torch.cuda.synchronize()
    st = stream.cuda_stream if stream is not None else None
    args = lambda p, cap: (al._ctx, ins[0].data_ptr() if len(blob) else None, len(blob), ins[1].data_ptr(), ins[2].data_ptr(), ins[3].data_ptr(),
                           ins[4].data_ptr(), n, p, cap, qw.data_ptr(), tw.data_ptr(), C.byref(nw), st)
    rc = f(*args(None, 0))
    if want_rc == _lib.ERR_BAD_ARG:
        assert rc == _lib.ERR_BAD_ARG
        total = int(_words(q_len).sum() + _words(t_len).sum())
    else:
        assert rc == _lib.ERR_OOM  # the sizing call: every pair takes two words at least
        total = nw.value
        assert total == int(_words(q_len).sum() + _words(t_len).sum())
        sized = (qw.cpu().numpy().view(np.uint64).copy(), tw.cpu().numpy().view(np.uint64).copy())
    packed = torch.from_numpy(np.full(total + SLACK, FILL, np.uint32).view(np.int32)).to("cuda:0")
    torch.cuda.synchronize()
    rc = f(*args(packed.data_ptr(), total))
    torch.cuda.synchronize()
    assert rc == want_rc, rc
    out = packed.cpu().numpy().view(np.uint32)
    assert (out[total:] == FILL).all(), "a word at or beyond the total was written"
    for d, h in zip(ins, ins_h):
        assert np.array_equal(d.cpu().numpy().view(h.dtype), h), "an input was written"
    got_qw, got_tw = qw.cpu().numpy().view(np.uint64), tw.cpu().numpy().view(np.uint64)
    if want_rc != _lib.ERR_BAD_ARG:
        assert nw.value == total and np.array_equal(got_qw, sized[0]) and np.array_equal(got_tw, sized[1])
    else:
        assert (out == FILL).all(), "d_packed was touched"
    return rc, out[:total], got_qw, got_tw, total


def _same(al, blob, q_off, q_len, t_off, t_len, stream=None):
    blob = np.ascontiguousarray(blob, np.uint8)
    q_off, t_off = np.ascontiguousarray(q_off, np.uint64), np.ascontiguousarray(t_off, np.uint64)  # (callers pass strided views)
    q_len, t_len = np.ascontiguousarray(q_len, np.uint32), np.ascontiguousarray(t_len, np.uint32)
    hrc, hp, hqw, htw, hn = _host_pack(blob, q_off, q_len, t_off, t_len)
    assert hrc == 0
    rc, p, qw, tw, total = _dev_pack(al, blob, q_off, q_len, t_off, t_len, stream)
    assert total == hn and np.array_equal(qw, hqw) and np.array_equal(tw, htw)
    bad = np.nonzero(p != hp)[0]
    assert len(bad) == 0, (len(bad), bad[:8], p[bad[:8]], hp[bad[:8]])
    return p, qw, tw


def _place(rng, lengths, aligns, junk=b"n"):
    """sequences of the given lengths at offsets with the given residues mod 16, in a blob of junk that is not ACGT: junk lies directly
    before the first base and behind the last base of every sequence.  Returns (blob, offsets)"""
    parts, offs, pos = [], [], 0
    for ln, al16 in zip(lengths, aligns):
        gap = (al16 - pos) % 16
        gap += 16 if gap == 0 else 0
        parts.append(junk * gap)
        pos += gap
        offs.append(pos)
        parts.append(bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), ln)))
        pos += ln
    parts.append(junk * 5)
    return np.frombuffer(b"".join(parts), np.uint8).copy(), np.array(offs, np.uint64)


def test_every_length_at_every_source_alignment(al):
    """1 .. 40 at each of the 16 residues; 63 .. 65, 224 .. 240, 1 000, 2 047, 2 048 with the residue moving on; queries and targets
    interleaved; junk that is not ACGT around every sequence"""
    rng = np.random.default_rng(71)
    lengths = [ln for ln in range(1, 41) for _ in range(16)] + [63, 64, 65] * 6 + list(range(224, 241)) * 2 + [1000, 2047, 2048] * 6
    aligns = [k % 16 for k in range(len(lengths))]
    aligns[-18:] = [(3 * k + 1) % 16 for k in range(18)]
    if len(lengths) % 2:
        lengths.append(7), aligns.append(9)
    blob, offs = _place(rng, lengths, aligns)
    assert {int(o) % 16 for o in offs} == set(range(16))
    lengths = np.array(lengths, np.uint32)
    _same(al, blob, offs[0::2], lengths[0::2], offs[1::2], lengths[1::2])


def test_one_long_read_among_short_ones(al):
    """a 50 000-base read among 100-base reads: tiles that lie inside one sequence and tiles that hold seventy"""
    rng = np.random.default_rng(72)
    lengths = [100] * 300 + [50000] + [100] * 301
    blob, offs = _place(rng, lengths, [(5 * k) % 16 for k in range(len(lengths))])
    lengths = np.array(lengths, np.uint32)
    p, qw, tw = _same(al, blob, offs[0::2], lengths[0::2], offs[1::2], lengths[1::2])
    assert len(p) > 3 * 1024  # more than one tile, more than one workgroup


def test_shared_bytes_empty_sides_too_long_and_the_blob_end(al):
    rng = np.random.default_rng(73)
    blob, offs = _place(rng, [300, 41, 77, 500, 33], [0, 7, 12, 3, 1])
    blob = blob[:int(offs[4]) + 33].copy()  # the last sequence ends at the blob's last byte
    T, far = int(offs[3]), np.uint64
    q_off = [offs[0], offs[1], offs[2], offs[0] + far(10), offs[0] + far(16), offs[1], far(1 << 60), far((1 << 64) - 1), offs[2], offs[4], far(0)]
    q_len = [300, 41, 77, 100, 284, 0, MAX_SEQ_LEN + 1, 0xFFFFFFFF, 77, 33, 0]
    t_off = [far(T)] * 5 + [far(T), far(T), far(1 << 63), far((1 << 64) - 5), offs[4] + far(32), far(0)]
    t_len = [500, 500, 500, 500, 500, 500, 500, MAX_SEQ_LEN + 1, 0, 1, 0]
    # (one target under many queries; queries that are substrings of the first; pairs with an empty side, whose other side is
    # still packed; lengths over WFAHIP_MAX_SEQ_LEN and empty sequences with offsets far outside the blob; the blob's last byte)
    p, qw, tw = _same(al, blob, q_off, q_len, t_off, t_len)
    assert p[int(qw[5])] == 0 and p[int(qw[6])] == 0 and p[int(tw[7])] == 0
    assert p[int(tw[5])] != 0  # the target of the pair whose query is empty is packed


def test_bytes_outside_acgt(al):
    """UNSUPPORTED for a lowercase letter or an N at the first, a middle and the last base; OK directly before the first and behind the
    last base (that is where _place puts its junk, and every other test packs there)"""
    from wfa_amd import _lib
    rng = np.random.default_rng(74)
    lengths, aligns = [100, 37, 64, 1000, 16, 250], [0, 5, 9, 14, 3, 8]
    blob, offs = _place(rng, lengths, aligns)
    lens = np.array(lengths, np.uint32)
    a = lambda: (offs[0::2].copy(), lens[0::2].copy(), offs[1::2].copy(), lens[1::2].copy())
    assert _dev_pack(al, blob, *a())[0] == 0
    for k in range(len(lengths)):
        for pos in (0, lengths[k] // 2, lengths[k] - 1):
            for byte in (b"a", b"N", b"t"):
                b2 = blob.copy()
                b2[int(offs[k]) + pos] = byte[0]
                rc, _, qw, tw, total = _dev_pack(al, b2, *a(), want_rc=_lib.ERR_UNSUPPORTED)
                hrc, _, hqw, htw, hn = _host_pack(b2, *a())
                assert hrc == _lib.ERR_UNSUPPORTED and total == hn and np.array_equal(qw, hqw) and np.array_equal(tw, htw)
    for k in range(len(lengths)):  # ... and ACGT or not, the bytes around a sequence do not count
        b2 = blob.copy()
        b2[int(offs[k]) - 1], b2[int(offs[k]) + lengths[k]] = ord("N"), ord("g")
        _same(al, b2, *a())


def test_sequences_outside_the_blob(al):
    from wfa_amd import _lib
    rng = np.random.default_rng(75)
    blob, offs = _place(rng, [100, 90, 80, 70], [0, 4, 8, 12])
    blob = blob[:int(offs[3]) + 70].copy()
    lens = np.array([100, 90, 80, 70], np.uint32)
    good = (offs[0::2].copy(), lens[0::2].copy(), offs[1::2].copy(), lens[1::2].copy())
    assert _dev_pack(al, blob, *good)[0] == 0
    for which, idx, off, ln in ((2, 1, offs[3], 71), (2, 1, offs[3] + np.uint64(1), 70), (0, 0, np.uint64((1 << 64) - 50), 100),
                                (2, 0, np.uint64((1 << 64) - 1), 2), (0, 1, np.uint64(len(blob)), 1), (0, 1, np.uint64(1 << 63), 80)):
        a = [x.copy() for x in good]
        a[which][idx], a[which + 1][idx] = off, ln
        _dev_pack(al, blob, *a, want_rc=_lib.ERR_BAD_ARG)
    a = [x.copy() for x in good]
    a[2][1], a[3][1] = np.uint64(len(blob)), 0  # an empty sequence at the blob's end is inside
    _same(al, blob, *a)


def test_empty_batch_and_a_callers_stream(al):
    import torch
    from wfa_amd import _lib
    nw = C.c_uint64(99)
    assert _lib.lib().wfahip_pack_pairs_device(al._ctx, None, 0, None, None, None, None, 0, None, 0, None, None, C.byref(nw), None) == 0
    assert nw.value == 0
    rng = np.random.default_rng(76)
    lengths = [int(x) for x in rng.integers(1, 700, 400)]
    blob, offs = _place(rng, lengths, [int(x) for x in rng.integers(0, 16, 400)])
    lens = np.array(lengths, np.uint32)
    s = torch.cuda.Stream(device="cuda:0")
    want = _same(al, blob, offs[0::2], lens[0::2], offs[1::2], lens[1::2], stream=s)
    # the Python mirror: the same words, four words of slack behind them
    t = [_dev(blob, np.uint8), _dev(offs[0::2].copy(), np.int64), _dev(lens[0::2].copy(), np.int32), _dev(offs[1::2].copy(), np.int64),
         _dev(lens[1::2].copy(), np.int32)]
    for stream in (None, s):
        packed, qw, tw = al.pack_tensors(*t, stream=stream)
        assert packed.dtype == torch.int32 and packed.numel() == len(want[0]) + 4
        assert np.array_equal(packed.cpu().numpy().view(np.uint32)[:-4], want[0]) and not packed[-4:].any()
        assert np.array_equal(qw.cpu().numpy().view(np.uint64), want[1]) and np.array_equal(tw.cpu().numpy().view(np.uint64), want[2])
    e = torch.zeros(0, dtype=torch.int64, device="cuda:0")
    packed, qw, tw = al.pack_tensors(t[0], e, e.to(torch.int32), e, e.to(torch.int32))
    assert packed.numel() == 4 and qw.numel() == 0 and tw.numel() == 0
    import wfa_amd
    t[0][int(offs[10]) + 1] = ord("n")
    with pytest.raises(wfa_amd._lib.WfaHipError) as ei:
        al.pack_tensors(*t)
    assert ei.value.code == _lib.ERR_UNSUPPORTED
