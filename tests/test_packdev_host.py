"""CPU: wfa_amd/csrc/wfa_packdev.hpp, the 16-bytes-to-a-word rule of wfahip_pack_pairs_device's kernels, compiled stand-alone with the
host compiler (tests/packdev_host_test.cpp) and held against the host packer wfahip_pack_pairs, word for word and verdict for
verdict: every length 1 .. 40 (every tail length), every byte value 0 .. 255 inside a sequence, and bytes behind the range, which
must neither reach a word nor count.  The program's own checks run under the host sanitizers as well."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "packdev_host_test.cpp")


def _build(name, extra=()):
    exe = os.path.join(ROOT, "build", name)
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", *extra, "-o", exe, SRC])
    return exe


@pytest.fixture(scope="module")
def exe():
    return _build("packdev_host_test")


def _through_header(exe, tmp_path, seqs):
    """seqs: (bytes held, len) -- the first len bytes are the sequence, the rest lies behind it.  Returns [(bad, words)]"""
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        for held, ln in seqs:
            held = held + b"\xee" * (-len(held) % 16)
            f.write(np.array([ln, len(held)], np.uint32).tobytes() + held)
    subprocess.check_call([exe, src, dst])
    out = np.fromfile(dst, np.uint32)
    res, pos = [], 0
    for _, ln in seqs:
        nw = (ln + 15) // 16 + 1
        res.append((int(out[pos]), out[pos + 1:pos + 1 + nw].copy()))
        pos += 1 + nw
    assert pos == len(out)
    return res


def _through_host_packer(seqs):
    """every sequence as the query of a pair with an empty target, through wfahip_pack_pairs one by one: (rc, words)"""
    from wfa_amd import _lib
    f = _lib.lib().wfahip_pack_pairs
    res = []
    for held, ln in seqs:
        blob = np.frombuffer(held + b"\0", np.uint8).copy()
        off, q_len, t_len = np.zeros(1, np.uint64), np.array([ln], np.uint32), np.zeros(1, np.uint32)
        nw = (ln + 15) // 16 + 1
        packed = np.full(nw + 1, 0xA5A5A5A5, np.uint32)
        qw, tw, total = np.zeros(1, np.uint64), np.zeros(1, np.uint64), C.c_uint64()
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        rc = f(vp(blob), vp(off), vp(q_len), vp(off), vp(t_len), 1, 1, vp(packed), vp(qw), vp(tw), C.byref(total))
        assert total.value == nw + 1 and tw[0] == nw and packed[nw] == 0
        res.append((rc, packed[:nw].copy()))
    return res


def _compare(exe, tmp_path, seqs, words_too=True):
    from wfa_amd import _lib
    got, want = _through_header(exe, tmp_path, seqs), _through_host_packer(seqs)
    for k, ((bad, w), (rc, hw)) in enumerate(zip(got, want)):
        assert rc in (_lib.OK, _lib.ERR_UNSUPPORTED)
        assert bad == (rc == _lib.ERR_UNSUPPORTED), (k, seqs[k])
        if words_too:
            assert np.array_equal(w, hw), (k, seqs[k])
        assert w[-1] == 0  # the pad word
        ln = seqs[k][1]
        if ln % 16:
            assert int(w[-2]) >> (2 * (ln % 16)) == 0  # the tail bits


def test_every_length_against_the_host_packer(built, exe, tmp_path):
    rng = np.random.default_rng(7)
    letters = np.frombuffer(b"ACGT", np.uint8)
    seqs = []
    for ln in range(1, 41):
        for junk in (b"", b"\xff" * 16, b"acgtnN\0xX" * 2, bytes(rng.integers(0, 256, 16, dtype=np.uint8))):
            seqs.append((bytes(rng.choice(letters, ln)) + junk, ln))
    _compare(exe, tmp_path, seqs)
    assert all(rc == 0 for rc, _ in _through_host_packer(seqs[:8]))


def test_every_byte_value_inside_a_sequence(built, exe, tmp_path):
    """the verdict for each of the 256 byte values, at the first, a middle and the last base; the words of the ACGT ones"""
    base = b"ACGTTGCAGTCAACGTGTAC" * 2 + b"ACG"  # 43 bases: two full words and a tail of 11
    seqs = []
    for v in range(256):
        for pos in (0, 17, len(base) - 1):
            s = bytearray(base)
            s[pos] = v
            seqs.append((bytes(s) + b"nnnn", len(base)))
    _compare(exe, tmp_path, seqs)
    n_ok = sum(1 for bad, _ in _through_header(exe, tmp_path, seqs) if not bad)
    assert n_ok == 4 * 3


def test_bytes_behind_the_range_do_not_count(built, exe, tmp_path):
    """a byte outside ACGT directly behind the last base, for every tail length: no verdict, no bit"""
    seqs = []
    for ln in list(range(1, 18)) + [31, 32, 33]:
        for behind in (b"n", b"N", b"\xff", b"\0", b"a"):
            seqs.append((b"T" * ln + behind * 15, ln))
    _compare(exe, tmp_path, seqs)
    for bad, _ in _through_header(exe, tmp_path, seqs):
        assert bad == 0


def test_rule_under_sanitizers():
    exe = _build("packdev_host_test_asan_ubsan", ("-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "packdev host test ok" in r.stdout
