"""GPU: the retry rungs of the sub-wave router (align_device, wfa_host.hip) that no other test drives on purpose -- the rungs
for the long leftovers of a mixed-length batch and the second chance on the LDS-ring kernel.  Each case forces its route with
the debug options, shows that the rung ran (a launch count, and the rung's pass failing the call when option fail_pass
injects a failure into exactly its kind) and compares every record and CIGAR with the oracle.  The other rungs:
test_parity_gpu.py::test_mid_window_rung_and_learned_start (128 diagonals, 256 diagonals, four times the rows),
::test_wide_band_retry_kernel (256 diagonals), ::test_fuzz_short_reads and ::test_short_read_batches (32 -> 64 diagonals)."""
import numpy as np
import pytest

from test_parity_gpu import _aligner, _oracle_params, assert_batch_equal

pytestmark = pytest.mark.gpu


def _fails_in_pass(al, data, kind):
    """The call runs a sub-wave pass of `kind`: with a failure injected into that kind it fails as a whole."""
    from wfa_amd import _lib as L
    al.set_option("fail_pass", kind)
    with pytest.raises(L.WfaHipError) as ei:
        al.align_arrays(*data)
    al.set_option("fail_pass", 0)
    return ei.value.code == L.ERR_OOM


def test_long_leftovers_of_a_mixed_batch(built):
    """300 pairs of 1 000 bases and 8 of 12 000, wf-adaptive off: the short pairs' pipeline (wfa_blk_kernel<16>) hands the long
    ones on for their length, they take a sliding-window pass of their own sized by the batch's longest pair (a wave per pair,
    128 diagonals: kind 15), and what leaves that band (every one of them: 12 kbp at 5 % error is hundreds of diagonals wide)
    the 256-diagonal one (kind 13)."""
    import wfa_amd as w
    from oracle import oracle as O
    short = w.generate_pairs(seed=141, n_pairs=300, length=1000, error_rate=0.05)
    longp = w.generate_pairs(seed=142, n_pairs=8, length=12000, error_rate=0.05)
    off = np.uint64(len(short[0]))
    data = (np.concatenate([short[0], longp[0]]), np.concatenate([short[1], longp[1] + off]), np.concatenate([short[2], longp[2]]),
            np.concatenate([short[3], longp[3] + off]), np.concatenate([short[4], longp[4]]))
    want = O.align_batch(_oracle_params(True, None), *data, n_threads=8)
    al = _aligner(True, None)
    al.set_option("duo", 0)
    got = al.align_arrays(*data)
    t = al.last_timing()
    assert t.main_kernel_kind == 3, t
    assert t.n_retried_pairs >= 8, t
    # forward + backtrace kernel each: the first pass, the two rungs of the long pairs; then at least one launch of the ladder
    assert t.n_launches >= 2 + 2 + 2 + 1 and t.n_main_launches == 1, t
    assert_batch_equal(got, want, "mixed lengths, long leftovers")
    assert _fails_in_pass(al, data, 15)
    assert _fails_in_pass(al, data, 13)
    assert_batch_equal(al.align_arrays(*data), want, "after the injected failures")
    al.close()


def test_second_chance_on_the_lds_ring_kernel(built):
    """Without the 256-diagonal rung (blk_wide = 0), more leftovers than one launch of wfa_generic_kernel holds at once (32 per CU)
    get a pass on wfa_packed_kernel (kind 1) for their band first.  The threshold is in pairs handed on, so this case cannot do
    with a few hundred: 32 per CU and 300 more, 1 000 bases at 10 % error with wf-adaptive off -- every band outgrows 64 diagonals."""
    import torch
    import wfa_amd as w
    from oracle import oracle as O
    n = torch.cuda.get_device_properties(0).multi_processor_count * 32 + 300
    data = w.generate_pairs(seed=143, n_pairs=n, length=1000, error_rate=0.10, n_threads=8)
    want = O.align_batch(_oracle_params(True, None), *data, n_threads=8)
    al = _aligner(True, None)
    al.set_option("duo", 0)
    al.set_option("blk_wide", 0)
    got = al.align_arrays(*data)
    t = al.last_timing()
    assert t.main_kernel_kind == 3, t
    assert t.n_retried_pairs > n - 300, t
    # forward + backtrace kernel of the first pass and of the rung, then at least one launch of the ladder
    assert t.n_launches >= 2 + 2 + 1 and t.n_main_launches == 1, t
    assert_batch_equal(got, want, "second chance on the LDS-ring kernel")
    assert _fails_in_pass(al, data, 1)
    al.close()
