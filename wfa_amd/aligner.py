"""Host-side mirror of the reference's Go API (package wfa) over the libwfahip.so C-ABI.

Same names, argument meaning and error behaviour as the reference (file:line into shenwei356/wfa):

    Penalties / DefaultPenalties                     wfa.go:32-43
    AdaptiveReductionOption / DefaultAdaptiveOption  wfa.go:46-60
    Options / DefaultOptions                         wfa.go:64-71
    New, RecycleAligner                              wfa.go:102-131
    Aligner.AdaptiveReduction                        wfa.go:134-140
    Aligner.Align / AlignPointers                    wfa.go:196-268
    ErrEmptySeq, ErrSeqTooLong, MaxSeqLen            wfa.go:186-193
    AlignmentResult, Op, OpM.., CIGAR, AlignmentText wfa_cigar.go:30-66,236-333
    RecycleAlignmentResult / RecycleAlignmentText    wfa_cigar.go:92,347

New (not in the reference): Aligner.AlignBatch -- the batch entry a GPU needs.  All alignment work
happens in the HIP kernels; this module only marshals buffers.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib as L

MaxSeqLen = L.MAX_SEQ_LEN
MaskLower32 = 4294967295
OpM, OpD, OpI, OpX, OpH = ord("M"), ord("D"), ord("I"), ord("X"), ord("H")


class WfaError(Exception):
    pass


ErrEmptySeq = WfaError("wfa: invalid empty sequence")                                 # wfa.go:187
ErrSeqTooLong = WfaError(f"wfa: sequences longer than {MaxSeqLen} are not supported")  # wfa.go:193
ErrOverMaxScore = WfaError("wfa: alignment score exceeds max_score")                  # (no counterpart: AlignBatch(.., max_score))


@dataclass
class Penalties:
    Mismatch: int = 4
    GapOpen: int = 6
    GapExt: int = 2


@dataclass
class AdaptiveReductionOption:
    MinWFLen: int = 10
    MaxDistDiff: int = 50
    CutoffStep: int = 1  # not used by the reference either (wfa.go:49)


@dataclass
class Options:
    GlobalAlignment: bool = True


DefaultPenalties = Penalties()
DefaultAdaptiveOption = AdaptiveReductionOption()
DefaultOptions = Options()


def Op(op: int) -> Tuple[str, int]:
    """wfa_cigar.go:57-59: split an op word into (letter, count)."""
    return chr(int(op) >> 32), int(op) & MaskLower32


def trimOps(ops: Sequence[int]) -> List[int]:
    """wfa_cigar.go:217-233 (returns [] where the reference would panic: no M op)."""
    idx = [i for i, o in enumerate(ops) if (int(o) >> 32) == OpM]
    if not idx:
        return []
    return list(ops[idx[0]:idx[-1] + 1])


def _i32(v: int) -> int:  # a record word that holds a signed position
    return v - (1 << 32) if v >= (1 << 31) else v


@dataclass
class AlignmentResult:
    """wfa_cigar.go:30-48.  Ops are op<<32|n, already reversed/merged (process(), :136-214)."""
    Ops: List[int] = field(default_factory=list)
    Score: int = 0
    TBegin: int = 0
    TEnd: int = 0
    QBegin: int = 0
    QEnd: int = 0
    AlignLen: int = 0
    Matches: int = 0
    Gaps: int = 0
    GapRegions: int = 0

    def CIGAR(self, onlyAlignedRegion: bool = False) -> str:  # wfa_cigar.go:236-255
        ops = trimOps(self.Ops) if onlyAlignedRegion else self.Ops
        return "".join(f"{int(o) & MaskLower32}{chr(int(o) >> 32)}" for o in ops)

    def AlignmentText(self, q0: bytes, t0: bytes, onlyAlignedRegion: bool = False) -> Tuple[bytes, bytes, bytes]:
        """wfa_cigar.go:259-333: the three display lines (query, bars, target)."""
        if not onlyAlignedRegion:
            q, t, ops = q0, t0, self.Ops
        else:
            q, t = q0[self.QBegin - 1:self.QEnd], t0[self.TBegin - 1:self.TEnd]
            ops = trimOps(self.Ops)
        Q, A, T = bytearray(), bytearray(), bytearray()
        v = h = 0
        for op in ops:
            letter, n = int(op) >> 32, int(op) & MaskLower32
            if letter == OpM or letter == OpX:
                Q += q[v:v + n]
                A += (b"|" if letter == OpM else b" ") * n
                T += t[h:h + n]
                v += n
                h += n
            elif letter == OpI:
                Q += b"-" * n
                A += b" " * n
                T += t[h:h + n]
                h += n
            elif letter in (OpD, OpH):
                Q += q[v:v + n]
                A += b" " * n
                T += b"-" * n
                v += n
        return bytes(Q), bytes(A), bytes(T)

    def key(self):
        return (0, self.Score, self.CIGAR(False), self.QBegin, self.QEnd, self.TBegin, self.TEnd,
                self.AlignLen, self.Matches, self.Gaps, self.GapRegions)


def RecycleAlignmentResult(r: Optional[AlignmentResult]) -> None:  # wfa_cigar.go:92 (pool return: no-op here)
    return None


def RecycleAlignmentText(Q, A, T) -> None:  # wfa_cigar.go:347
    return None


@dataclass
class Timing:
    kernel_ms: float
    total_ms: float
    n_launches: int
    n_retried_pairs: int
    cells_stored: int
    ops_written: int
    arena_bytes: int
    main_kernel_ms: float
    n_main_launches: int = 0
    n_packed_pairs: int = 0
    main_kernel_kind: int = 0
    ladder_start_level: int = 0  # arena level the long-pair ladder started on (learned hint)


def make_blob(qs: Sequence[bytes], ts: Sequence[bytes]):
    """Flat byte blob + offset/length arrays, the C-ABI input layout (cgo rule: no Go pointers inside)."""
    n = len(qs)
    q_len = np.fromiter((len(x) for x in qs), dtype=np.uint32, count=n)
    t_len = np.fromiter((len(x) for x in ts), dtype=np.uint32, count=n)
    # 16-byte aligned starts: lets the staging loop use aligned dword loads
    q_cap = (q_len.astype(np.uint64) + 15) & ~np.uint64(15)
    t_cap = (t_len.astype(np.uint64) + 15) & ~np.uint64(15)
    tot = q_cap + t_cap
    starts = np.zeros(n, dtype=np.uint64)
    if n > 1:
        starts[1:] = np.cumsum(tot[:-1])
    q_off = starts
    t_off = starts + q_cap
    total = int(tot.sum()) if n else 0
    blob = np.zeros(max(total, 1), dtype=np.uint8)
    for i in range(n):
        blob[int(q_off[i]):int(q_off[i]) + int(q_len[i])] = np.frombuffer(qs[i], dtype=np.uint8)
        blob[int(t_off[i]):int(t_off[i]) + int(t_len[i])] = np.frombuffer(ts[i], dtype=np.uint8)
    return blob, q_off, q_len, t_off, t_len


class Aligner:
    """The aligner object (wfa.go:79-87).  Not safe for concurrent use; one per thread (wfa.go:73-78)."""

    def __init__(self, p: Penalties, opt: Options, device: int = -1):
        self.p = p
        self.opt = opt
        self.ad: Optional[AdaptiveReductionOption] = None
        self._ctx = C.c_void_p()
        self._one = None  # Align's reusable record / ops buffers
        self._device = device if device >= 0 else None  # (None: the HIP runtime's current device when the context was created)
        L.check(L.lib().wfahip_create(device, C.byref(self._ctx)), "wfahip_create")

    # -- reference API ---------------------------------------------------------------------------
    def AdaptiveReduction(self, ad: AdaptiveReductionOption) -> Optional[Exception]:
        """wfa.go:134-140: returns an error (not raises) iff MinWFLen == 0, like the Go method."""
        if ad.MinWFLen == 0:
            return WfaError("cutoff step should not be 0")
        self.ad = ad
        return None

    def Align(self, q: bytes, t: bytes) -> AlignmentResult:
        """wfa.go:196: raises ErrEmptySeq / ErrSeqTooLong where the Go method returns them."""
        if len(q) == 0 or len(t) == 0:
            raise ErrEmptySeq
        if len(q) > MaxSeqLen or len(t) > MaxSeqLen:
            raise ErrSeqTooLong
        # wfahip_align_pair: record + ops into two reusable buffers (no arrays to build, none to take apart); what does not
        # change between calls -- the parameter block, the entry point, the by-reference wrappers -- is built once
        # (a third of the Python side of a 150 us call)
        lq, lt = len(q), len(t)
        one = self._one
        if one is None or len(one[1]) < 2 * (lq + lt) + 64:
            rec, ops, n_ops, prm = (C.c_uint32 * L.REC_WORDS)(), (C.c_uint64 * (2 * (lq + lt) + 64))(), C.c_uint64(), self._params()
            one = self._one = (rec, ops, n_ops, C.byref(prm), C.byref(n_ops), L.lib().wfahip_align_pair, prm)
        rec, ops, n_ops, prm_ref, n_ref, entry = one[0], one[1], one[2], one[3], one[4], one[5]
        # The Go aligner reads algn.p / algn.opt / algn.ad on every Align (wfa.go:79-87,134-140): penalties or options
        # re-assigned, or an AdaptiveReductionOption mutated in place, between two calls must show in the second one -- the
        # cached block is REFILLED every call (a few attribute stores; the by-reference wrapper stays)
        prm, p_, ad = one[6], self.p, self.ad
        prm.mismatch, prm.gap_open, prm.gap_ext = p_.Mismatch, p_.GapOpen, p_.GapExt
        prm.global_alignment = 1 if self.opt.GlobalAlignment else 0
        if ad is None:
            prm.adaptive = 0
        else:
            prm.adaptive, prm.min_wf_len, prm.max_dist_diff, prm.cutoff_step = 1, ad.MinWFLen, ad.MaxDistDiff, ad.CutoffStep
        rc = entry(self._ctx, prm_ref, q, lq, t, lt, rec, ops, len(ops), n_ref)
        if rc != 0:
            L.check(rc, "wfahip_align_pair")
        if rec[L.REC_STATUS] != L.PAIR_OK:
            raise ErrSeqTooLong if rec[L.REC_STATUS] == L.PAIR_TOO_LONG else (
                ErrEmptySeq if rec[L.REC_STATUS] == L.PAIR_EMPTY else WfaError("pair could not be aligned (out of device memory)"))
        r = rec[0:10]  # (one slice instead of ten index calls: REC_STATUS .. REC_GAP_REGIONS)
        i32 = _i32
        return AlignmentResult(ops[:n_ops.value], r[L.REC_SCORE], i32(r[L.REC_TBEGIN]), i32(r[L.REC_TEND]), i32(r[L.REC_QBEGIN]),
                               i32(r[L.REC_QEND]), r[L.REC_ALIGN_LEN], r[L.REC_MATCHES], r[L.REC_GAPS], r[L.REC_GAP_REGIONS])

    AlignPointers = Align  # wfa.go:201 (pointer arguments have no Python analogue)

    # -- new: batch entry --------------------------------------------------------------------------
    def _params(self) -> L.Params:
        p = L.Params(self.p.Mismatch, self.p.GapOpen, self.p.GapExt, 1 if self.opt.GlobalAlignment else 0, 0)
        if self.ad is not None:
            p.adaptive = 1
            p.min_wf_len, p.max_dist_diff, p.cutoff_step = self.ad.MinWFLen, self.ad.MaxDistDiff, self.ad.CutoffStep
        return p

    def align_arrays(self, blob, q_off, q_len, t_off, t_len, max_score: int = 0) -> "BatchResult":
        """Batch alignment over the C-ABI layout; returns struct-of-arrays results (numpy copies).  max_score > 0
        (include/wfa_hip.h: wfahip_align_batch_bounded): a pair whose score exceeds it stops early, with status PAIR_OVER_MAX
        (8) and every other field 0; the pairs within the bound come back as without one."""
        if not 0 <= int(max_score) < 1 << 32:
            raise ValueError("max_score must fit in 32 bits")
        n = int(len(q_len))
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        q_off = np.ascontiguousarray(q_off, dtype=np.uint64)
        t_off = np.ascontiguousarray(t_off, dtype=np.uint64)
        q_len = np.ascontiguousarray(q_len, dtype=np.uint32)
        t_len = np.ascontiguousarray(t_len, dtype=np.uint32)
        res = L.Results()
        prm = self._params()
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        if int(max_score):
            L.check(L.lib().wfahip_align_batch_bounded(self._ctx, C.byref(prm), vp(blob), blob.size, vp(q_off), vp(q_len),
                                                       vp(t_off), vp(t_len), n, int(max_score), C.byref(res)), "wfahip_align_batch_bounded")
        else:
            L.check(L.lib().wfahip_align_batch(self._ctx, C.byref(prm), vp(blob), blob.size, vp(q_off), vp(q_len),
                                               vp(t_off), vp(t_len), n, C.byref(res)), "wfahip_align_batch")
        return _take_results(res, n)

    def align_arrays_packed(self, packed, q_woff, q_len, t_woff, t_len) -> "BatchResult":
        """Batch alignment of pre-packed 2-bit input (include/wfa_hip.h: wfahip_align_batch_packed); pack with
        pack_pairs().  A quarter of the bytes cross PCIe; results are those of align_arrays on the unpacked bytes."""
        return self.align_arrays_packed_rc(packed, q_woff, q_len, t_woff, t_len, None)

    def align_arrays_packed_rc(self, packed, q_woff, q_len, t_woff, t_len, q_rc) -> "BatchResult":
        """align_arrays_packed with a flag per pair (include/wfa_hip.h: wfahip_align_batch_packed_rc): a pair whose flag is non-zero
        aligns the reverse complement of its query, made on the GPU from the same words -- every field and CIGAR op equals
        align_arrays' on the bytes (revcomp(query), target); qbegin / qend count on the reverse-complemented query.  The last step of
        pack once, score_arrays_packed_rc both strands, align the survivors: a subset of the same offsets and flags on the same buffer.
        Offsets may repeat, under any lengths and flags.  q_rc=None: no flag set."""
        n = int(len(q_len))
        packed = np.ascontiguousarray(packed, dtype=np.uint32)
        q_woff = np.ascontiguousarray(q_woff, dtype=np.uint64)
        t_woff = np.ascontiguousarray(t_woff, dtype=np.uint64)
        q_len = np.ascontiguousarray(q_len, dtype=np.uint32)
        t_len = np.ascontiguousarray(t_len, dtype=np.uint32)
        if len(q_woff) != n or len(t_woff) != n or len(t_len) != n:
            raise ValueError("offset and length arrays differ in length")
        if q_rc is not None:
            q_rc = np.ascontiguousarray(np.asarray(q_rc) != 0, dtype=np.uint8)
            if q_rc.shape != (n,):
                raise ValueError("q_rc must hold one flag per pair")
        res = L.Results()
        prm = self._params()
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        if q_rc is None:
            L.check(L.lib().wfahip_align_batch_packed(self._ctx, C.byref(prm), vp(packed), packed.size, vp(q_woff), vp(q_len),
                                                      vp(t_woff), vp(t_len), n, C.byref(res)), "wfahip_align_batch_packed")
        else:
            L.check(L.lib().wfahip_align_batch_packed_rc(self._ctx, C.byref(prm), vp(packed), packed.size, vp(q_woff), vp(q_len),
                                                         vp(t_woff), vp(t_len), vp(q_rc), n, C.byref(res)), "wfahip_align_batch_packed_rc")
        return _take_results(res, n)

    # -- new: score only (include/wfa_hip.h: wfahip_score_batch) -----------------------------------
    def score_arrays(self, blob, q_off, q_len, t_off, t_len, max_score: int = 0):
        """(status: np.int32[n], score: np.uint32[n]) of every pair -- the AlignmentResult.Score and status align_arrays would
        give, from the forward pass alone (no CIGAR, no arena).  max_score > 0: a pair whose score exceeds it gets status
        PAIR_OVER_MAX (8) and score 0."""
        n = int(len(q_len))
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        q_off = np.ascontiguousarray(q_off, dtype=np.uint64)
        t_off = np.ascontiguousarray(t_off, dtype=np.uint64)
        q_len = np.ascontiguousarray(q_len, dtype=np.uint32)
        t_len = np.ascontiguousarray(t_len, dtype=np.uint32)
        if len(q_off) != n or len(t_off) != n or len(t_len) != n:
            raise ValueError("offset and length arrays differ in length")
        if not 0 <= int(max_score) < 1 << 32:
            raise ValueError("max_score must fit in 32 bits")
        res = L.Scores()
        prm = self._params()
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        rc = L.lib().wfahip_score_batch(self._ctx, C.byref(prm), vp(blob), blob.size, vp(q_off), vp(q_len), vp(t_off), vp(t_len), n,
                                        int(max_score), C.byref(res))
        L.check(rc, "wfahip_score_batch" + (f" ({L.lib().wfahip_last_error(self._ctx).decode(errors='replace')})" if rc else ""))
        try:
            if n == 0:
                return np.zeros(0, np.int32), np.zeros(0, np.uint32)
            return (np.ctypeslib.as_array(res.status, shape=(n,)).copy(), np.ctypeslib.as_array(res.score, shape=(n,)).copy())
        finally:
            L.lib().wfahip_scores_free(C.byref(res))

    def score_arrays_packed(self, packed, q_woff, q_len, t_woff, t_len, max_score: int = 0):
        """score_arrays on pre-packed 2-bit input (include/wfa_hip.h: wfahip_score_batch_packed): takes what pack_pairs() returns,
        and the same buffer then serves align_arrays_packed for the pairs worth aligning.  Offsets may repeat and come in any order;
        a quarter of the bytes cross PCIe.  (status, score) equal score_arrays' on the unpacked bytes."""
        return self.score_arrays_packed_rc(packed, q_woff, q_len, t_woff, t_len, None, max_score=max_score)

    def score_arrays_packed_rc(self, packed, q_woff, q_len, t_woff, t_len, q_rc, max_score: int = 0):
        """score_arrays_packed with a flag per pair (include/wfa_hip.h: wfahip_score_batch_packed_rc): a pair whose flag is non-zero
        scores the reverse complement of its query, made on the GPU from the same words -- (status, score) equal score_arrays' on the
        bytes (revcomp(query), target).  Both strands of a pair: list it twice, once flagged.  q_rc=None: no flag set."""
        n = int(len(q_len))
        packed = np.ascontiguousarray(packed, dtype=np.uint32)
        q_woff = np.ascontiguousarray(q_woff, dtype=np.uint64)
        t_woff = np.ascontiguousarray(t_woff, dtype=np.uint64)
        q_len = np.ascontiguousarray(q_len, dtype=np.uint32)
        t_len = np.ascontiguousarray(t_len, dtype=np.uint32)
        if len(q_woff) != n or len(t_woff) != n or len(t_len) != n:
            raise ValueError("offset and length arrays differ in length")
        if not 0 <= int(max_score) < 1 << 32:
            raise ValueError("max_score must fit in 32 bits")
        if q_rc is not None:
            q_rc = np.ascontiguousarray(np.asarray(q_rc) != 0, dtype=np.uint8)
            if q_rc.shape != (n,):
                raise ValueError("q_rc must hold one flag per pair")
        res = L.Scores()
        prm = self._params()
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        if q_rc is None:
            name = "wfahip_score_batch_packed"
            rc = L.lib().wfahip_score_batch_packed(self._ctx, C.byref(prm), vp(packed), packed.size, vp(q_woff), vp(q_len), vp(t_woff),
                                                   vp(t_len), n, int(max_score), C.byref(res))
        else:
            name = "wfahip_score_batch_packed_rc"
            rc = L.lib().wfahip_score_batch_packed_rc(self._ctx, C.byref(prm), vp(packed), packed.size, vp(q_woff), vp(q_len), vp(t_woff),
                                                      vp(t_len), vp(q_rc), n, int(max_score), C.byref(res))
        L.check(rc, name + (f" ({L.lib().wfahip_last_error(self._ctx).decode(errors='replace')})" if rc else ""))
        try:
            if n == 0:
                return np.zeros(0, np.int32), np.zeros(0, np.uint32)
            return (np.ctypeslib.as_array(res.status, shape=(n,)).copy(), np.ctypeslib.as_array(res.score, shape=(n,)).copy())
        finally:
            L.lib().wfahip_scores_free(C.byref(res))

    def ScoreBatch(self, qs: Sequence[bytes], ts: Sequence[bytes], max_score: int = 0):
        """(status, score) arrays of the pairs (qs[i], ts[i]): see score_arrays."""
        if len(qs) != len(ts):
            raise ValueError("qs and ts differ in length")
        if not qs:
            return np.zeros(0, np.int32), np.zeros(0, np.uint32)
        return self.score_arrays(*make_blob(qs, ts), max_score=max_score)

    def Score(self, q: bytes, t: bytes) -> int:
        """AlignmentResult.Score of Align(q, t) without the alignment; raises ErrEmptySeq / ErrSeqTooLong like Align."""
        if len(q) == 0 or len(t) == 0:
            raise ErrEmptySeq
        if len(q) > MaxSeqLen or len(t) > MaxSeqLen:
            raise ErrSeqTooLong
        st, sc = self.ScoreBatch([bytes(q)], [bytes(t)])
        if st[0] != L.PAIR_OK:
            raise WfaError("pair could not be aligned (out of device memory)")
        return int(sc[0])

    # -- new: score only on device-resident input (include/wfa_hip.h: wfahip_score_batch_device) ------
    def score_tensors(self, blob, q_off, q_len, t_off, t_len, max_score: int = 0, out=None, stream=None):
        """score_arrays for a batch that lives on the aligner's GPU: torch tensors in (blob uint8, q_off int64, q_len int32,
        t_off int64, t_len int32 -- what generate_pairs_device returns), a pair of int32 tensors (status, score) on the same
        device out.  `score` holds the C-ABI's uint32 bit for bit (torch has no unsigned 32-bit arithmetic: a score of 2^31 or
        more reads negative; view it through numpy as uint32 if that can happen).  status and score equal what score_arrays
        returns for the same bytes and max_score.  Nothing proportional to the batch crosses PCIe, and the inputs are never
        written.  out: an optional pair of contiguous int32 tensors of at least n elements each on that device; elements
        beyond n keep their contents.  stream: a torch.cuda.Stream, None = torch's current stream; the call returns when the
        results are there.  Raises ValueError -- before the library is called -- for anything that is not a contiguous
        tensor of the right dtype on the aligner's device, or for offset / length tensors of differing lengths.
        (The buffers are torch's: torch.cuda must have been initialised before the first aligner of the process was created
        -- torch ships its own HIP runtime, and it does not find the GPUs once the library's runtime has come up first.)"""
        import torch
        ins = (("blob", blob, torch.uint8), ("q_off", q_off, torch.int64), ("q_len", q_len, torch.int32),
               ("t_off", t_off, torch.int64), ("t_len", t_len, torch.int32))
        dev = None

        def want(name, t, dtype):
            nonlocal dev
            if not isinstance(t, torch.Tensor):
                raise ValueError(f"{name} must be a torch tensor on the aligner's device, not {type(t).__name__}")
            if not t.is_cuda:
                raise ValueError(f"{name} is on the host: score_tensors takes tensors on the aligner's device (score_arrays takes host arrays)")
            if self._device is not None and t.device.index != self._device:
                raise ValueError(f"{name} is on {t.device}, the aligner on device {self._device}")
            if dev is None:
                dev = t.device
            if t.device != dev:
                raise ValueError(f"{name} is on {t.device}, blob on {dev}")
            if t.dtype != dtype:
                raise ValueError(f"{name} must be {dtype}, not {t.dtype}")
            if t.dim() != 1 or not t.is_contiguous():
                raise ValueError(f"{name} must be one-dimensional and contiguous")

        for name, t, dtype in ins:
            want(name, t, dtype)
        n = int(q_len.numel())
        if q_off.numel() != n or t_off.numel() != n or t_len.numel() != n:
            raise ValueError("offset and length tensors differ in length")
        if not 0 <= int(max_score) < 1 << 32:
            raise ValueError("max_score must fit in 32 bits")
        if out is None:
            status = torch.zeros(n, dtype=torch.int32, device=dev)
            score = torch.zeros(n, dtype=torch.int32, device=dev)
        else:
            try:
                status, score = out
            except (TypeError, ValueError):
                raise ValueError("out must be a pair (status, score) of tensors") from None
            want("out status", status, torch.int32), want("out score", score, torch.int32)
            if status.numel() < n or score.numel() < n:
                raise ValueError(f"out tensors must hold at least {n} elements")
        if n == 0:
            return status, score
        if stream is None:
            stream = torch.cuda.current_stream(dev)
        elif not isinstance(stream, torch.cuda.Stream):
            raise ValueError("stream must be a torch.cuda.Stream")
        if out is None:
            stream.wait_stream(torch.cuda.current_stream(dev))  # (the fills above ran on torch's current stream)
        prm = self._params()
        rc = L.lib().wfahip_score_batch_device(self._ctx, C.byref(prm), blob.data_ptr(), blob.numel(), q_off.data_ptr(), q_len.data_ptr(),
                                               t_off.data_ptr(), t_len.data_ptr(), n, 0, int(max_score), status.data_ptr(),
                                               score.data_ptr(), stream.cuda_stream)
        L.check(rc, "wfahip_score_batch_device" + (f" ({L.lib().wfahip_last_error(self._ctx).decode(errors='replace')})" if rc else ""))
        return status, score

    # -- new: full alignment and CIGAR text on device-resident data (include/wfa_hip.h: wfahip_align_batch_device, wfahip_cigar_text_device)
    def _want_tensor(self, name, t, dtype, dev=None, dim=1):
        """the checks score_tensors makes, for one tensor: ValueError unless t is a contiguous dim-dimensional tensor of dtype on
        the aligner's device (and on dev, when given); returns its device"""
        import torch
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a torch tensor on the aligner's device, not {type(t).__name__}")
        if not t.is_cuda:
            raise ValueError(f"{name} is on the host: a tensor on the aligner's device is needed")
        if getattr(self, "_device", None) is not None and t.device.index != self._device:
            raise ValueError(f"{name} is on {t.device}, the aligner on device {self._device}")
        if dev is not None and t.device != dev:
            raise ValueError(f"{name} is on {t.device}, not on {dev}")
        if t.dtype != dtype:
            raise ValueError(f"{name} must be {dtype}, not {t.dtype}")
        if t.dim() != dim or not t.is_contiguous():
            raise ValueError(f"{name} must be {dim}-dimensional and contiguous")
        return t.device

    @staticmethod
    def _want_stream(stream, dev):
        import torch
        if stream is None:
            return torch.cuda.current_stream(dev)
        if not isinstance(stream, torch.cuda.Stream):
            raise ValueError("stream must be a torch.cuda.Stream")
        return stream

    @staticmethod
    def _order_after_torch(stream, dev):
        """what torch has queued on its current stream comes before the call on `stream`.  Torch's default stream has the handle 0,
        which the C-ABI reads as "the context's own stream" -- a non-blocking one, not ordered behind torch's: it is drained."""
        import torch
        cur = torch.cuda.current_stream(dev)
        if stream.cuda_stream == 0:
            cur.synchronize()
            stream.synchronize()
        else:
            stream.wait_stream(cur)

    def align_tensors(self, blob, q_off, q_len, t_off, t_len, max_score: int = 0, stream=None):
        """Full alignment of a batch that lives on the aligner's GPU, the results left there: torch tensors in, as score_tensors takes
        them (blob uint8, q_off int64, q_len int32, t_off int64, t_len int32 -- what generate_pairs_device returns); out
        (rec, ops): rec int32 [n, 16], one record per pair (the words of include/wfa_hip.h's WFAHIP_REC_*, the C-ABI's uint32 bit
        for bit), and ops int64, the op buffer the records' OPS_OFF / OPS_LEN index (op << 32 | count; in completion order, with
        slack between pairs and behind the last).  max_score > 0: wfahip_align_batch_bounded_device -- a pair over the bound has
        the record {8, 0, ..}.  The op buffer is sized by a first guess and the call repeated with what it needed when that was too
        small.  cigar_tensors renders the pair (rec, ops) to text.  Conventions, stream and ValueErrors as score_tensors."""
        import torch
        dev = self._want_tensor("blob", blob, torch.uint8)
        for name, t, dtype in (("q_off", q_off, torch.int64), ("q_len", q_len, torch.int32), ("t_off", t_off, torch.int64),
                               ("t_len", t_len, torch.int32)):
            self._want_tensor(name, t, dtype, dev)
        n = int(q_len.numel())
        if q_off.numel() != n or t_off.numel() != n or t_len.numel() != n:
            raise ValueError("offset and length tensors differ in length")
        if not 0 <= int(max_score) < 1 << 32:
            raise ValueError("max_score must fit in 32 bits")
        stream = self._want_stream(stream, dev)
        rec = torch.zeros((n, L.REC_WORDS), dtype=torch.int32, device=dev)
        if n == 0:
            return rec, torch.zeros(0, dtype=torch.int64, device=dev)
        # CIGAR ops are merged runs: the host entry's first guess of (n + m) / 4 + 8 per pair
        ops_cap = (int(q_len.sum(dtype=torch.int64)) + int(t_len.sum(dtype=torch.int64))) // 4 + 8 * n + 1024
        prm = self._params()
        lib = L.lib()
        for _attempt in range(6):
            ops = torch.zeros(ops_cap, dtype=torch.int64, device=dev)
            self._order_after_torch(stream, dev)  # (the fills above ran on torch's current stream)
            needed = C.c_uint64(0)
            ins = (blob.data_ptr(), blob.numel(), q_off.data_ptr(), q_len.data_ptr(), t_off.data_ptr(), t_len.data_ptr(), n, 0)
            if int(max_score):
                rc = lib.wfahip_align_batch_bounded_device(self._ctx, C.byref(prm), *ins, int(max_score), rec.data_ptr(), ops.data_ptr(),
                                                           ops_cap, C.byref(needed), stream.cuda_stream)
            else:
                rc = lib.wfahip_align_batch_device(self._ctx, C.byref(prm), *ins, rec.data_ptr(), ops.data_ptr(), ops_cap,
                                                   C.byref(needed), stream.cuda_stream)
            if rc == L.ERR_OOM and needed.value > ops_cap:
                ops_cap = needed.value + needed.value // 3 + 1024
                continue
            break
        L.check(rc, "wfahip_align_batch_device" + (f" ({lib.wfahip_last_error(self._ctx).decode(errors='replace')})" if rc else ""))
        return rec, ops

    def cigar_tensors(self, rec, ops, only_aligned: bool = False, out=None, stream=None):
        """AlignmentResult.CIGAR(only_aligned) of every pair of (rec, ops) -- align_tensors' output, or any records and ops of that
        layout on the aligner's GPU -- rendered there (include/wfa_hip.h: wfahip_cigar_text_device): returns (text uint8,
        off int64 [n + 1]); pair i's text is text[off[i]:off[i + 1]], without terminators, and off[n] the total.  A pair that is not
        OK renders the empty string, and so does, under only_aligned, a pair without an M op.  out=None: the text is sized by one
        call and written by a second, and has exactly off[n] bytes.  out=(text, off): contiguous tensors on that device, off of at
        least n + 1 elements, text of any size -- bytes at and beyond off[n] keep their contents; a text tensor that is too small
        raises WfaHipError (ERR_OOM) with off filled, so that off[n] says what is needed.  rec and ops are never written.  stream
        and ValueErrors as score_tensors."""
        import torch
        dev = self._want_tensor("rec", rec, torch.int32, dim=2)
        if rec.shape[1] != L.REC_WORDS:
            raise ValueError(f"rec must be [n, {L.REC_WORDS}]")
        self._want_tensor("ops", ops, torch.int64, dev)
        n = int(rec.shape[0])
        ptr = lambda t: t.data_ptr() if t.numel() else None

        def entry(text, cap, off, needed, stream):
            return L.lib().wfahip_cigar_text_device(self._ctx, rec.data_ptr(), ptr(ops), ops.numel(), n, 1 if only_aligned else 0, text, cap,
                                                    off.data_ptr(), C.byref(needed), stream.cuda_stream)
        return self._render_text(n, dev, out, stream, entry, "wfahip_cigar_text_device")

    def _render_text(self, n, dev, out, stream, entry, what):
        """what the methods that return one text share (cigar_tensors, diff_tensors, diff_tensors_packed): out= checked, one sizing call
        and one that writes (or one into out), the error raised.  entry(text, cap, off, needed, stream) is the C call with the
        text's pointer (None without a byte of capacity) and its capacity."""
        import torch
        if out is not None:
            try:
                text, off = out
            except (TypeError, ValueError):
                raise ValueError("out must be a pair (text, off) of tensors") from None
            self._want_tensor("out text", text, torch.uint8, dev), self._want_tensor("out off", off, torch.int64, dev)
            if off.numel() < n + 1:
                raise ValueError(f"out off must hold at least {n + 1} elements")
        stream = self._want_stream(stream, dev)
        if out is None:
            off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        self._order_after_torch(stream, dev)  # (the fill above, and whatever made the inputs, ran on torch's current stream)
        if n == 0:
            if out is not None:
                off[:1] = 0
            return (torch.zeros(0, dtype=torch.uint8, device=dev) if out is None else text), off
        needed = C.c_uint64(0)

        def call(t):
            return entry(t.data_ptr() if t is not None and t.numel() else None, t.numel() if t is not None else 0, off, needed, stream)
        if out is None:
            rc = call(None)  # the sizing call
            if rc == L.ERR_OOM:
                text = torch.empty(needed.value, dtype=torch.uint8, device=dev)
                rc = call(text)
            elif rc == L.OK:
                text = torch.zeros(0, dtype=torch.uint8, device=dev)
        else:
            rc = call(text)
        L.check(rc, what + (f" ({L.lib().wfahip_last_error(self._ctx).decode(errors='replace')})" if rc else ""))
        return text, off

    # -- new: the packed entries on device-resident data (include/wfa_hip.h: wfahip_pack_pairs_device, wfahip_align_batch_packed_device)
    def pack_tensors(self, blob, q_off, q_len, t_off, t_len, stream=None):
        """pack_pairs for a batch that lives on the aligner's GPU (include/wfa_hip.h: wfahip_pack_pairs_device): torch tensors in, as
        score_tensors takes them; out (packed int32, q_woff int64, t_woff int64) on the same device -- word for word, offset for
        offset what pack_pairs returns for the same bytes (the C-ABI's uint32 / uint64 bit for bit).  packed has four words of slack
        behind the words the offsets name (zero; packed.numel() - 4 is the total), so that it goes straight into
        align_tensors_packed.  Sized by one call and written by a second.  Raises WfaHipError, as pack_pairs does: ERR_UNSUPPORTED
        for a byte outside ACGT inside a sequence, ERR_BAD_ARG for a sequence outside the blob.  The inputs are never written.
        stream and ValueErrors as score_tensors."""
        import torch
        dev = self._want_tensor("blob", blob, torch.uint8)
        for name, t, dtype in (("q_off", q_off, torch.int64), ("q_len", q_len, torch.int32), ("t_off", t_off, torch.int64),
                               ("t_len", t_len, torch.int32)):
            self._want_tensor(name, t, dtype, dev)
        n = int(q_len.numel())
        if q_off.numel() != n or t_off.numel() != n or t_len.numel() != n:
            raise ValueError("offset and length tensors differ in length")
        stream = self._want_stream(stream, dev)
        q_woff = torch.zeros(n, dtype=torch.int64, device=dev)
        t_woff = torch.zeros(n, dtype=torch.int64, device=dev)
        if n == 0:
            return torch.zeros(4, dtype=torch.int32, device=dev), q_woff, t_woff
        lib = L.lib()
        n_words = C.c_uint64(0)

        def call(p):
            self._order_after_torch(stream, dev)  # (the fills ran on torch's current stream)
            return lib.wfahip_pack_pairs_device(self._ctx, blob.data_ptr() if blob.numel() else None, blob.numel(), q_off.data_ptr(),
                                                q_len.data_ptr(), t_off.data_ptr(), t_len.data_ptr(), n, p.data_ptr() if p is not None else None,
                                                p.numel() - 4 if p is not None else 0, q_woff.data_ptr(), t_woff.data_ptr(),
                                                C.byref(n_words), stream.cuda_stream)
        rc = call(None)  # the sizing call: every pair takes two words at least, so it ends in ERR_OOM with the total, or in an error
        packed = None
        if rc == L.ERR_OOM:
            packed = torch.zeros(n_words.value + 4, dtype=torch.int32, device=dev)
            rc = call(packed)
        L.check(rc, "wfahip_pack_pairs_device" + (f" ({lib.wfahip_last_error(self._ctx).decode(errors='replace')})" if rc else ""))
        return packed, q_woff, t_woff

    def align_tensors_packed(self, packed, q_woff, q_len, t_woff, t_len, q_rc=None, max_score: int = 0, stream=None):
        """align_tensors over 2-bit words that live on the aligner's GPU (include/wfa_hip.h: wfahip_align_batch_packed_device): packed
        int32 with at least four words of slack behind the words the offsets name (pack_tensors' output has them), q_woff / t_woff
        int64, q_len / t_len int32, q_rc an optional uint8 tensor of one flag per pair (non-zero: the pair aligns the reverse
        complement of its query, made on the GPU from the same words).  Returns (rec, ops) as align_tensors does -- every record
        field and every op equals align_arrays_packed_rc's on the same words, and with max_score > 0 align_arrays(max_score=)'s on
        the bytes -- and they go into cigar_tensors unchanged.  The inputs are never written.  Op-capacity retry, stream and
        ValueErrors as align_tensors."""
        import torch
        dev = self._want_tensor("packed", packed, torch.int32)
        for name, t, dtype in (("q_woff", q_woff, torch.int64), ("q_len", q_len, torch.int32), ("t_woff", t_woff, torch.int64),
                               ("t_len", t_len, torch.int32)):
            self._want_tensor(name, t, dtype, dev)
        n = int(q_len.numel())
        if q_woff.numel() != n or t_woff.numel() != n or t_len.numel() != n:
            raise ValueError("offset and length tensors differ in length")
        if q_rc is not None:
            self._want_tensor("q_rc", q_rc, torch.uint8, dev)
            if q_rc.numel() != n:
                raise ValueError("q_rc must hold one flag per pair")
        if packed.numel() < 4:
            raise ValueError("packed must hold four words of slack behind its words")
        if not 0 <= int(max_score) < 1 << 32:
            raise ValueError("max_score must fit in 32 bits")
        stream = self._want_stream(stream, dev)
        rec = torch.zeros((n, L.REC_WORDS), dtype=torch.int32, device=dev)
        if n == 0:
            return rec, torch.zeros(0, dtype=torch.int64, device=dev)
        n_words = int(packed.numel()) - 4
        # CIGAR ops are merged runs: the host entry's first guess of (n + m) / 4 + 8 per pair
        ops_cap = (int(q_len.sum(dtype=torch.int64)) + int(t_len.sum(dtype=torch.int64))) // 4 + 8 * n + 1024
        prm = self._params()
        lib = L.lib()
        for _attempt in range(6):
            ops = torch.zeros(ops_cap, dtype=torch.int64, device=dev)
            self._order_after_torch(stream, dev)  # (the fills above ran on torch's current stream)
            needed = C.c_uint64(0)
            rc = lib.wfahip_align_batch_packed_device(self._ctx, C.byref(prm), packed.data_ptr(), n_words, q_woff.data_ptr(), q_len.data_ptr(),
                                                      t_woff.data_ptr(), t_len.data_ptr(), q_rc.data_ptr() if q_rc is not None else None, n, 0,
                                                      int(max_score), rec.data_ptr(), ops.data_ptr(), ops_cap, C.byref(needed),
                                                      stream.cuda_stream)
            if rc == L.ERR_OOM and needed.value > ops_cap:
                ops_cap = needed.value + needed.value // 3 + 1024
                continue
            break
        L.check(rc, "wfahip_align_batch_packed_device" + (f" ({lib.wfahip_last_error(self._ctx).decode(errors='replace')})" if rc else ""))
        return rec, ops

    # -- new: the screen on device-resident words and its survivors (include/wfa_hip.h: wfahip_score_batch_packed_device, wfahip_select_pairs_device)
    def score_tensors_packed(self, packed, q_woff, q_len, t_woff, t_len, q_rc=None, max_score: int = 0, out=None, stream=None):
        """score_arrays_packed_rc over 2-bit words that live on the aligner's GPU (include/wfa_hip.h: wfahip_score_batch_packed_device):
        the tensors align_tensors_packed takes -- packed int32 with at least four words of slack behind the words the offsets name,
        q_woff / t_woff int64, q_len / t_len int32, q_rc an optional uint8 tensor of one flag per pair (non-zero: the pair scores the
        reverse complement of its query) -- in, a pair of int32 tensors (status, score) on the same device out, as score_tensors
        returns them: they equal score_arrays_packed_rc's on the same words, flags and max_score.  Only counters cross PCIe, and the
        inputs are never written.  out: an optional pair of contiguous int32 tensors of at least n elements each; elements beyond n
        keep their contents.  stream and ValueErrors as score_tensors."""
        import torch
        dev = self._want_tensor("packed", packed, torch.int32)
        for name, t, dtype in (("q_woff", q_woff, torch.int64), ("q_len", q_len, torch.int32), ("t_woff", t_woff, torch.int64),
                               ("t_len", t_len, torch.int32)):
            self._want_tensor(name, t, dtype, dev)
        n = int(q_len.numel())
        if q_woff.numel() != n or t_woff.numel() != n or t_len.numel() != n:
            raise ValueError("offset and length tensors differ in length")
        if q_rc is not None:
            self._want_tensor("q_rc", q_rc, torch.uint8, dev)
            if q_rc.numel() != n:
                raise ValueError("q_rc must hold one flag per pair")
        if packed.numel() < 4:
            raise ValueError("packed must hold four words of slack behind its words")
        if not 0 <= int(max_score) < 1 << 32:
            raise ValueError("max_score must fit in 32 bits")
        if out is None:
            status = torch.zeros(n, dtype=torch.int32, device=dev)
            score = torch.zeros(n, dtype=torch.int32, device=dev)
        else:
            try:
                status, score = out
            except (TypeError, ValueError):
                raise ValueError("out must be a pair (status, score) of tensors") from None
            self._want_tensor("out status", status, torch.int32, dev), self._want_tensor("out score", score, torch.int32, dev)
            if status.numel() < n or score.numel() < n:
                raise ValueError(f"out tensors must hold at least {n} elements")
        stream = self._want_stream(stream, dev)
        if n == 0:
            return status, score
        self._order_after_torch(stream, dev)  # (the fills above, and whatever made the inputs, ran on torch's current stream)
        prm = self._params()
        lib = L.lib()
        rc = lib.wfahip_score_batch_packed_device(self._ctx, C.byref(prm), packed.data_ptr(), int(packed.numel()) - 4, q_woff.data_ptr(),
                                                  q_len.data_ptr(), t_woff.data_ptr(), t_len.data_ptr(),
                                                  q_rc.data_ptr() if q_rc is not None else None, n, 0, int(max_score), status.data_ptr(),
                                                  score.data_ptr(), stream.cuda_stream)
        L.check(rc, "wfahip_score_batch_packed_device" + (f" ({lib.wfahip_last_error(self._ctx).decode(errors='replace')})" if rc else ""))
        return status, score

    def select_tensors(self, status, q_off, q_len, t_off, t_len, q_rc=None, stream=None):
        """The pairs whose status is PAIR_OK, in pair order, as the next stage's tensors (include/wfa_hip.h: wfahip_select_pairs_device):
        status int32 -- score_tensors' or score_tensors_packed's, under a max_score the screen's verdict --, q_off / t_off int64 (word
        or byte offsets: they are only copied), q_len / t_len int32, q_rc an optional uint8 tensor.  Returns
        (idx int32, q_off, q_len, t_off, t_len, q_rc) on the same device, each sliced to the number of selected pairs (q_rc None when
        none was given); idx holds the selected pairs' indices, the C-ABI's uint32 bit for bit.  They go into align_tensors_packed or
        align_tensors unchanged.  Only the count crosses PCIe.  stream and ValueErrors as score_tensors."""
        import torch
        dev = self._want_tensor("status", status, torch.int32)
        for name, t, dtype in (("q_off", q_off, torch.int64), ("q_len", q_len, torch.int32), ("t_off", t_off, torch.int64),
                               ("t_len", t_len, torch.int32)):
            self._want_tensor(name, t, dtype, dev)
        n = int(status.numel())
        if q_off.numel() != n or q_len.numel() != n or t_off.numel() != n or t_len.numel() != n:
            raise ValueError("status, offset and length tensors differ in length")
        if q_rc is not None:
            self._want_tensor("q_rc", q_rc, torch.uint8, dev)
            if q_rc.numel() != n:
                raise ValueError("q_rc must hold one flag per pair")
        stream = self._want_stream(stream, dev)
        outs = [torch.empty(n, dtype=dt, device=dev) for dt in (torch.int32, torch.int64, torch.int32, torch.int64, torch.int32)]
        outs.append(torch.empty(n, dtype=torch.uint8, device=dev) if q_rc is not None else None)
        if n == 0:
            return tuple(outs)
        self._order_after_torch(stream, dev)  # (whatever made the inputs ran on torch's current stream)
        lib = L.lib()
        cnt = C.c_uint64(0)
        ptr = lambda t: t.data_ptr() if t is not None else None
        rc = lib.wfahip_select_pairs_device(self._ctx, status.data_ptr(), n, q_off.data_ptr(), q_len.data_ptr(), t_off.data_ptr(), t_len.data_ptr(),
                                            ptr(q_rc), *[ptr(t) for t in outs], C.byref(cnt), stream.cuda_stream)
        L.check(rc, "wfahip_select_pairs_device" + (f" ({lib.wfahip_last_error(self._ctx).decode(errors='replace')})" if rc else ""))
        return tuple(t[:cnt.value] if t is not None else None for t in outs)

    # -- the check (include/wfa_hip.h: wfahip_check_alignments_device, wfahip_check_alignments_packed_device)
    def check_tensors(self, rec, ops, blob, q_off, q_len, t_off, t_len, mask: int = L.CHK_ALL, out=None, stream=None):
        """The verdict on every pair of (rec, ops) -- align_tensors' output -- over the blob and the four tensors that call was
        given, computed on the aligner's GPU under the aligner's penalties and options (include/wfa_hip.h:
        wfahip_check_alignments_device): returns (chk int32 [n, 8], passed int32 [n], n_flagged int).  chk[i] holds FLAGS, COST,
        Q_USED, T_USED, N_BAD, FIRST_BAD, 0, 0 of pair i, the C-ABI's uint32 bit for bit (the CHK_* bits of _lib name the flags);
        passed[i] is the record's status when that is not PAIR_OK, else PAIR_OK when FLAGS & mask == 0, else PAIR_CHECK_FAILED -- it
        goes into select_tensors as its status unchanged; n_flagged counts the OK pairs with FLAGS & mask != 0, the only number
        that crosses PCIe.  A bad pair is a flag, never an error.  out=(chk, passed): contiguous tensors on that device of those
        shapes.  No input is written.  stream and ValueErrors as score_tensors."""
        return self._check_tensors(False, rec, ops, blob, "blob", q_off, q_len, t_off, t_len, None, mask, out, stream)

    def check_tensors_packed(self, rec, ops, packed, q_woff, q_len, t_woff, t_len, q_rc=None, mask: int = L.CHK_ALL, out=None,
                             stream=None):
        """check_tensors over 2-bit words, both strands (include/wfa_hip.h: wfahip_check_alignments_packed_device): (rec, ops) are
        align_tensors_packed's output, packed (int32, every word of the tensor counts) / q_woff / q_len / t_woff / t_len / q_rc the
        tensors that call was given.  A flagged pair's columns compare the reverse complement of its query, the strand its record
        and ops speak of.  Returns, out=, stream and ValueErrors as check_tensors."""
        return self._check_tensors(True, rec, ops, packed, "packed", q_woff, q_len, t_woff, t_len, q_rc, mask, out, stream)

    def _check_tensors(self, is_packed, rec, ops, seqs, seqs_name, q_off, q_len, t_off, t_len, q_rc, mask, out, stream):
        import torch
        dev = self._want_tensor("rec", rec, torch.int32, dim=2)
        if rec.shape[1] != L.REC_WORDS:
            raise ValueError(f"rec must be [n, {L.REC_WORDS}]")
        self._want_tensor("ops", ops, torch.int64, dev)
        self._want_tensor(seqs_name, seqs, torch.int32 if is_packed else torch.uint8, dev)
        for name, t, dtype in (("q_off", q_off, torch.int64), ("q_len", q_len, torch.int32), ("t_off", t_off, torch.int64),
                               ("t_len", t_len, torch.int32)):
            self._want_tensor(name, t, dtype, dev)
        n = int(rec.shape[0])
        if q_off.numel() != n or q_len.numel() != n or t_off.numel() != n or t_len.numel() != n:
            raise ValueError("offset and length tensors must hold one element per record")
        if q_rc is not None:
            self._want_tensor("q_rc", q_rc, torch.uint8, dev)
            if q_rc.numel() != n:
                raise ValueError("q_rc must hold one flag per pair")
        if not 0 <= int(mask) <= 0xFFFFFFFF:
            raise ValueError("mask must fit 32 bits")
        if out is not None:
            try:
                chk, passed = out
            except (TypeError, ValueError):
                raise ValueError("out must be (chk, passed), two tensors") from None
            self._want_tensor("out chk", chk, torch.int32, dev, dim=2)
            self._want_tensor("out passed", passed, torch.int32, dev)
            if tuple(chk.shape) != (n, L.CHK_WORDS) or passed.numel() != n:
                raise ValueError(f"out chk must be [{n}, {L.CHK_WORDS}] and out passed [{n}]")
        stream = self._want_stream(stream, dev)
        if out is None:
            chk = torch.empty((n, L.CHK_WORDS), dtype=torch.int32, device=dev)
            passed = torch.empty(n, dtype=torch.int32, device=dev)
        if n == 0:
            return chk, passed, 0
        self._order_after_torch(stream, dev)  # (whatever made the inputs ran on torch's current stream)
        ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
        prm = self._params()
        cnt = C.c_uint64(0)
        lib = L.lib()
        head = (self._ctx, C.byref(prm), rec.data_ptr(), ptr(ops), ops.numel(), ptr(seqs), seqs.numel(), q_off.data_ptr(), q_len.data_ptr(),
                t_off.data_ptr(), t_len.data_ptr())
        tail = (n, int(mask), chk.data_ptr(), passed.data_ptr(), C.byref(cnt), stream.cuda_stream)
        if is_packed:
            what = "wfahip_check_alignments_packed_device"
            rc = lib.wfahip_check_alignments_packed_device(*head, ptr(q_rc), *tail)
        else:
            what = "wfahip_check_alignments_device"
            rc = lib.wfahip_check_alignments_device(*head, *tail)
        L.check(rc, what + (f" ({lib.wfahip_last_error(self._ctx).decode(errors='replace')})" if rc else ""))
        return chk, passed, int(cnt.value)

    def alignment_text_tensors(self, rec, ops, blob, q_off, q_len, t_off, t_len, only_aligned: bool = False, out=None, stream=None):
        """AlignmentResult.AlignmentText(q, t, only_aligned) of every pair of (rec, ops) -- align_tensors' output -- over the blob
        and the four tensors that call was given, rendered on the aligner's GPU (include/wfa_hip.h: wfahip_alignment_text_device):
        returns (q_row uint8, a_row uint8, t_row uint8, off int64 [n + 1]); pair i's three rows are the planes' [off[i]:off[i + 1]],
        and off[n] is the length of each plane.  A pair that is not OK has empty rows, and so has, under only_aligned, a pair
        without an M op.  out=None: the planes are sized by one call and written by a second, and have exactly off[n] bytes.
        out=(q_row, a_row, t_row, off): contiguous tensors on that device, off of at least n + 1 elements, the planes of any one
        size -- bytes at and beyond off[n] keep their contents; planes that are too small raise WfaHipError (ERR_OOM) with off
        filled.  A record whose ops or windows leave the op buffer or the sequences raises WfaHipError (ERR_BAD_ARG) and writes
        no row.  No input is written.  stream and ValueErrors as score_tensors."""
        import torch
        dev = self._want_tensor("rec", rec, torch.int32, dim=2)
        if rec.shape[1] != L.REC_WORDS:
            raise ValueError(f"rec must be [n, {L.REC_WORDS}]")
        self._want_tensor("ops", ops, torch.int64, dev)
        self._want_tensor("blob", blob, torch.uint8, dev)
        for name, t, dtype in (("q_off", q_off, torch.int64), ("q_len", q_len, torch.int32), ("t_off", t_off, torch.int64),
                               ("t_len", t_len, torch.int32)):
            self._want_tensor(name, t, dtype, dev)
        n = int(rec.shape[0])
        if q_off.numel() != n or q_len.numel() != n or t_off.numel() != n or t_len.numel() != n:
            raise ValueError("offset and length tensors must hold one element per record")
        ptr = lambda t: t.data_ptr() if t.numel() else None

        def entry(rows, cap, off, needed, stream):
            return L.lib().wfahip_alignment_text_device(self._ctx, rec.data_ptr(), ptr(ops), ops.numel(), ptr(blob), blob.numel(),
                                                    q_off.data_ptr(), q_len.data_ptr(), t_off.data_ptr(), t_len.data_ptr(), n,
                                                    1 if only_aligned else 0, *rows, cap, off.data_ptr(), C.byref(needed),
                                                    stream.cuda_stream)
        return self._render_rows(n, dev, out, stream, entry, "wfahip_alignment_text_device")

    def alignment_text_tensors_packed(self, rec, ops, packed, q_woff, q_len, t_woff, t_len, q_rc=None, only_aligned: bool = False,
                                      out=None, stream=None):
        """alignment_text_tensors over 2-bit words, both strands (include/wfa_hip.h: wfahip_alignment_text_packed_device): (rec, ops)
        are align_tensors_packed's output, packed / q_woff / q_len / t_woff / t_len / q_rc the tensors that call was given -- packed
        int32 (every word of the tensor counts: this entry needs no slack, and slack does no harm), q_woff / t_woff int64, q_len /
        t_len int32, q_rc an optional uint8 tensor of one flag per pair.  The query row of a flagged pair holds the reverse
        complement of its query, the strand its record and ops speak of.  Returns, out=, errors, stream and ValueErrors as
        alignment_text_tensors; the rows equal that method's over the corresponding bytes."""
        import torch
        dev = self._want_tensor("rec", rec, torch.int32, dim=2)
        if rec.shape[1] != L.REC_WORDS:
            raise ValueError(f"rec must be [n, {L.REC_WORDS}]")
        self._want_tensor("ops", ops, torch.int64, dev)
        self._want_tensor("packed", packed, torch.int32, dev)
        for name, t, dtype in (("q_woff", q_woff, torch.int64), ("q_len", q_len, torch.int32), ("t_woff", t_woff, torch.int64),
                               ("t_len", t_len, torch.int32)):
            self._want_tensor(name, t, dtype, dev)
        n = int(rec.shape[0])
        if q_woff.numel() != n or q_len.numel() != n or t_woff.numel() != n or t_len.numel() != n:
            raise ValueError("offset and length tensors must hold one element per record")
        if q_rc is not None:
            self._want_tensor("q_rc", q_rc, torch.uint8, dev)
            if q_rc.numel() != n:
                raise ValueError("q_rc must hold one flag per pair")
        ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None

        def entry(rows, cap, off, needed, stream):
            return L.lib().wfahip_alignment_text_packed_device(self._ctx, rec.data_ptr(), ptr(ops), ops.numel(), ptr(packed), packed.numel(),
                                                           q_woff.data_ptr(), q_len.data_ptr(), t_woff.data_ptr(), t_len.data_ptr(),
                                                           ptr(q_rc), n, 1 if only_aligned else 0, *rows, cap, off.data_ptr(),
                                                           C.byref(needed), stream.cuda_stream)
        return self._render_rows(n, dev, out, stream, entry, "wfahip_alignment_text_packed_device")

    def diff_tensors(self, rec, ops, blob, q_off, q_len, t_off, t_len, only_aligned: bool = False, out=None, stream=None):
        """The difference string (minimap2's cs tag, short form) of every pair of (rec, ops) -- align_tensors' output -- over the
        blob and the four tensors that call was given, rendered on the aligner's GPU (include/wfa_hip.h: wfahip_diff_text_device):
        returns (text uint8, off int64 [n + 1]); pair i's string is text[off[i]:off[i + 1]] -- ':' and a count per M op, '*' target
        base, query base per X column, '-' and the target's bases per I op, '+' and the query's per D or H op, bases in lower case --
        and off[n] the total.  The target is the string's reference sequence.  Which ops render, the windows under only_aligned, the
        empty strings and the refused records are alignment_text_tensors'; out=, the sizing call and the errors are cigar_tensors'.
        No input is written.  stream and ValueErrors as score_tensors."""
        import torch
        dev = self._want_tensor("rec", rec, torch.int32, dim=2)
        if rec.shape[1] != L.REC_WORDS:
            raise ValueError(f"rec must be [n, {L.REC_WORDS}]")
        self._want_tensor("ops", ops, torch.int64, dev)
        self._want_tensor("blob", blob, torch.uint8, dev)
        for name, t, dtype in (("q_off", q_off, torch.int64), ("q_len", q_len, torch.int32), ("t_off", t_off, torch.int64),
                               ("t_len", t_len, torch.int32)):
            self._want_tensor(name, t, dtype, dev)
        n = int(rec.shape[0])
        if q_off.numel() != n or q_len.numel() != n or t_off.numel() != n or t_len.numel() != n:
            raise ValueError("offset and length tensors must hold one element per record")
        ptr = lambda t: t.data_ptr() if t.numel() else None

        def entry(text, cap, off, needed, stream):
            return L.lib().wfahip_diff_text_device(self._ctx, rec.data_ptr(), ptr(ops), ops.numel(), ptr(blob), blob.numel(), q_off.data_ptr(),
                                                   q_len.data_ptr(), t_off.data_ptr(), t_len.data_ptr(), n, 1 if only_aligned else 0, text,
                                                   cap, off.data_ptr(), C.byref(needed), stream.cuda_stream)
        return self._render_text(n, dev, out, stream, entry, "wfahip_diff_text_device")

    def diff_tensors_packed(self, rec, ops, packed, q_woff, q_len, t_woff, t_len, q_rc=None, only_aligned: bool = False, out=None,
                            stream=None):
        """diff_tensors over 2-bit words, both strands (include/wfa_hip.h: wfahip_diff_text_packed_device): (rec, ops) are
        align_tensors_packed's output, packed / q_woff / q_len / t_woff / t_len / q_rc the tensors that call was given, as
        alignment_text_tensors_packed takes them.  The string of a flagged pair spells the bases of the reverse complement of its
        query, the strand its record and ops speak of.  Returns, out=, errors, stream and ValueErrors as diff_tensors; the text
        equals that method's over the corresponding bytes."""
        import torch
        dev = self._want_tensor("rec", rec, torch.int32, dim=2)
        if rec.shape[1] != L.REC_WORDS:
            raise ValueError(f"rec must be [n, {L.REC_WORDS}]")
        self._want_tensor("ops", ops, torch.int64, dev)
        self._want_tensor("packed", packed, torch.int32, dev)
        for name, t, dtype in (("q_woff", q_woff, torch.int64), ("q_len", q_len, torch.int32), ("t_woff", t_woff, torch.int64),
                               ("t_len", t_len, torch.int32)):
            self._want_tensor(name, t, dtype, dev)
        n = int(rec.shape[0])
        if q_woff.numel() != n or q_len.numel() != n or t_woff.numel() != n or t_len.numel() != n:
            raise ValueError("offset and length tensors must hold one element per record")
        if q_rc is not None:
            self._want_tensor("q_rc", q_rc, torch.uint8, dev)
            if q_rc.numel() != n:
                raise ValueError("q_rc must hold one flag per pair")
        ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None

        def entry(text, cap, off, needed, stream):
            return L.lib().wfahip_diff_text_packed_device(self._ctx, rec.data_ptr(), ptr(ops), ops.numel(), ptr(packed), packed.numel(),
                                                          q_woff.data_ptr(), q_len.data_ptr(), t_woff.data_ptr(), t_len.data_ptr(), ptr(q_rc),
                                                          n, 1 if only_aligned else 0, text, cap, off.data_ptr(), C.byref(needed),
                                                          stream.cuda_stream)
        return self._render_text(n, dev, out, stream, entry, "wfahip_diff_text_packed_device")

    # -- the pileup (include/wfa_hip.h: wfahip_pileup_device, wfahip_pileup_packed_device)
    def pileup_tensors(self, rec, ops, blob, q_off, q_len, t_off, t_len, pile_at, pile_n, only_aligned: bool = False, out=None, stream=None):
        """What the alignments of (rec, ops) -- align_tensors' output -- say about every base of the window [pile_at, pile_at +
        pile_n) of the blob, counted on the aligner's GPU (include/wfa_hip.h: wfahip_pileup_device): returns (counts int32 [pile_n,
        8], n_piled int).  counts[b] holds, for byte pile_at + b of the blob as a TARGET base, the alignments that put A, C, T, G or
        another byte over it, those in which it faces a gap, the runs of query-only bases behind it and their bases (the PILE_W_*
        words of _lib; the C-ABI's uint32 bit for bit); n_piled is the number of pairs whose ops were swept.  out=: a contiguous
        int32 tensor [pile_n, 8] on that device that the call ADDS to -- several batches, both strands or several calls accumulate
        into one pileup; without it a zeroed tensor is made.  Which pairs and ops count, the windows under only_aligned and the
        refused records (WfaHipError ERR_BAD_ARG, the counts untouched) are alignment_text_tensors'.  No input is written.  stream
        and ValueErrors as score_tensors."""
        return self._pileup_tensors(False, rec, ops, blob, "blob", q_off, q_len, t_off, t_len, None, pile_at, pile_n, only_aligned, out, stream)

    def pileup_tensors_packed(self, rec, ops, packed, q_woff, q_len, t_woff, t_len, pile_at, pile_n, q_rc=None, only_aligned: bool = False,
                              out=None, stream=None):
        """pileup_tensors over 2-bit words, both strands (include/wfa_hip.h: wfahip_pileup_packed_device): (rec, ops) are
        align_tensors_packed's output, packed / q_woff / q_len / t_woff / t_len / q_rc the tensors that call was given, as
        alignment_text_tensors_packed takes them.  The window counts in BASES of the words' storage: base p of the sequence at word
        woff is 16 * woff + p.  A flagged pair adds the bases of the reverse complement of its query, the strand its record and ops
        speak of.  Returns, out=, errors, stream and ValueErrors as pileup_tensors."""
        return self._pileup_tensors(True, rec, ops, packed, "packed", q_woff, q_len, t_woff, t_len, q_rc, pile_at, pile_n, only_aligned, out,
                                    stream)

    def _pileup_tensors(self, is_packed, rec, ops, seqs, seqs_name, q_off, q_len, t_off, t_len, q_rc, pile_at, pile_n, only_aligned, out,
                        stream):
        import torch
        dev = self._want_tensor("rec", rec, torch.int32, dim=2)
        if rec.shape[1] != L.REC_WORDS:
            raise ValueError(f"rec must be [n, {L.REC_WORDS}]")
        self._want_tensor("ops", ops, torch.int64, dev)
        self._want_tensor(seqs_name, seqs, torch.int32 if is_packed else torch.uint8, dev)
        for name, t, dtype in (("q_off", q_off, torch.int64), ("q_len", q_len, torch.int32), ("t_off", t_off, torch.int64),
                               ("t_len", t_len, torch.int32)):
            self._want_tensor(name, t, dtype, dev)
        n = int(rec.shape[0])
        if q_off.numel() != n or q_len.numel() != n or t_off.numel() != n or t_len.numel() != n:
            raise ValueError("offset and length tensors must hold one element per record")
        if q_rc is not None:
            self._want_tensor("q_rc", q_rc, torch.uint8, dev)
            if q_rc.numel() != n:
                raise ValueError("q_rc must hold one flag per pair")
        pile_at, pile_n = int(pile_at), int(pile_n)
        if not 0 <= pile_at < 1 << 64 or not 0 <= pile_n <= L.PILE_MAX_N:
            raise ValueError("pile_at must fit 64 bits and pile_n lie in [0, 2^61 / 8]")
        if out is not None:
            self._want_tensor("out", out, torch.int32, dev, dim=2)
            if tuple(out.shape) != (pile_n, L.PILE_WORDS):
                raise ValueError(f"out must be [{pile_n}, {L.PILE_WORDS}]")
        stream = self._want_stream(stream, dev)
        counts = out if out is not None else torch.zeros((pile_n, L.PILE_WORDS), dtype=torch.int32, device=dev)
        if n == 0 or pile_n == 0:
            return counts, 0
        self._order_after_torch(stream, dev)  # (the fill above, and whatever made the inputs, ran on torch's current stream)
        ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
        cnt = C.c_uint64(0)
        lib = L.lib()
        head = (self._ctx, rec.data_ptr(), ptr(ops), ops.numel(), ptr(seqs), seqs.numel(), q_off.data_ptr(), q_len.data_ptr(), t_off.data_ptr(),
                t_len.data_ptr())
        tail = (n, 1 if only_aligned else 0, pile_at, pile_n, counts.data_ptr(), C.byref(cnt), stream.cuda_stream)
        if is_packed:
            what = "wfahip_pileup_packed_device"
            rc = lib.wfahip_pileup_packed_device(*head, ptr(q_rc), *tail)
        else:
            what = "wfahip_pileup_device"
            rc = lib.wfahip_pileup_device(*head, *tail)
        L.check(rc, what + (f" ({lib.wfahip_last_error(self._ctx).decode(errors='replace')})" if rc else ""))
        return counts, int(cnt.value)

    def _render_rows(self, n, dev, out, stream, entry, what):
        """what the row methods share: out= checked, one sizing call and one that writes (or one into out), the error raised.
        entry(rows, cap, off, needed, stream) is the C call with three plane pointers of capacity cap."""
        import torch
        if out is not None:
            try:
                q_row, a_row, t_row, off = out
            except (TypeError, ValueError):
                raise ValueError("out must be (q_row, a_row, t_row, off), four tensors") from None
            for name, t in (("out q_row", q_row), ("out a_row", a_row), ("out t_row", t_row)):
                self._want_tensor(name, t, torch.uint8, dev)
            self._want_tensor("out off", off, torch.int64, dev)
            if not q_row.numel() == a_row.numel() == t_row.numel():
                raise ValueError("out q_row, a_row and t_row must be of one size")
            if off.numel() < n + 1:
                raise ValueError(f"out off must hold at least {n + 1} elements")
        stream = self._want_stream(stream, dev)
        if out is None:
            off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        self._order_after_torch(stream, dev)  # (the fill above, and whatever made the inputs, ran on torch's current stream)
        empty = lambda: torch.zeros(0, dtype=torch.uint8, device=dev)
        if n == 0:
            if out is not None:
                off[:1] = 0
                return q_row, a_row, t_row, off
            return empty(), empty(), empty(), off
        needed = C.c_uint64(0)

        def call(planes):
            cap = planes[0].numel() if planes else 0
            rows = [p.data_ptr() for p in planes] if cap else [None] * 3
            return entry(rows, cap, off, needed, stream)
        if out is None:
            rc = call(None)  # the sizing call
            if rc == L.ERR_OOM:
                q_row, a_row, t_row = (torch.empty(needed.value, dtype=torch.uint8, device=dev) for _ in range(3))
                rc = call((q_row, a_row, t_row))
            elif rc == L.OK:
                q_row, a_row, t_row = empty(), empty(), empty()
        else:
            rc = call((q_row, a_row, t_row))
        L.check(rc, what + (f" ({L.lib().wfahip_last_error(self._ctx).decode(errors='replace')})" if rc else ""))
        return q_row, a_row, t_row, off

    def align_arrays_text(self, blob, q_off, q_len, t_off, t_len, only_aligned: bool = False):
        """align_arrays with the CIGARs as text in place of the ops (include/wfa_hip.h: wfahip_align_batch_text): returns
        (BatchResult, text np.uint8, off np.uint64 [n + 1]).  Every field of the BatchResult equals align_arrays' except that
        ops_off is all 0 and ops is empty -- no op crosses PCIe; pair i's CIGAR(only_aligned) is text[off[i]:off[i + 1]].  The plain
        path: no sliced upload, no autopack (the header says when that matters)."""
        n = int(len(q_len))
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        q_off = np.ascontiguousarray(q_off, dtype=np.uint64)
        t_off = np.ascontiguousarray(t_off, dtype=np.uint64)
        q_len = np.ascontiguousarray(q_len, dtype=np.uint32)
        t_len = np.ascontiguousarray(t_len, dtype=np.uint32)
        for name, a in (("blob", blob), ("q_off", q_off), ("q_len", q_len), ("t_off", t_off), ("t_len", t_len)):
            if a.ndim != 1:
                raise ValueError(f"{name} must be one-dimensional")
        if len(q_off) != n or len(t_off) != n or len(t_len) != n:
            raise ValueError("offset and length arrays differ in length")
        res, cig = L.Results(), L.Cigars()
        prm = self._params()
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        L.check(L.lib().wfahip_align_batch_text(self._ctx, C.byref(prm), vp(blob), blob.size, vp(q_off), vp(q_len), vp(t_off), vp(t_len),
                                                n, 1 if only_aligned else 0, C.byref(res), C.byref(cig)), "wfahip_align_batch_text")
        try:
            text, off = _take_cigars(cig)
        finally:
            L.lib().wfahip_cigars_free(C.byref(cig))
        return _take_results(res, n), text, off

    # -- new: score matrix (include/wfa_hip.h: wfahip_score_matrix) ------------------------------------
    def score_matrix_arrays(self, blob, q_off, q_len, t_off, t_len, max_score: int = 0, out=None, q_rc=None):
        """(status: np.int32[n_q, n_t], score: np.uint32[n_q, n_t]) of every query against every target: cell (i, j) is what
        score_arrays gives for the pair (query i, target j).  Pass the same arrays as queries and targets for all against all.
        out: an optional pair of preallocated C-contiguous arrays of shape (n_q, n_t) -- or row-strided views of that shape into
        larger ones (one row stride for both); nothing outside the window is written.  Returns the arrays written.
        q_rc: optional flags, one per QUERY (wfahip_score_matrix_rc): the cells of a flagged row score the reverse complement of that
        query (A <-> T, C <-> G in either case, other bytes themselves); as a target the same sequence stays forward."""
        same = q_off is t_off and q_len is t_len  # (all against all: the entry packs and uploads each sequence once)
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        q_off = np.ascontiguousarray(q_off, dtype=np.uint64)
        t_off = np.ascontiguousarray(t_off, dtype=np.uint64)
        q_len = np.ascontiguousarray(q_len, dtype=np.uint32)
        t_len = np.ascontiguousarray(t_len, dtype=np.uint32)
        if same:
            t_off, t_len = q_off, q_len
        n_q, n_t = int(len(q_len)), int(len(t_len))
        if len(q_off) != n_q or len(t_off) != n_t:
            raise ValueError("offset and length arrays differ in length")
        if not 0 <= int(max_score) < 1 << 32:
            raise ValueError("max_score must fit in 32 bits")
        if q_rc is not None:
            q_rc = np.ascontiguousarray(np.asarray(q_rc) != 0, dtype=np.uint8)
            if q_rc.shape != (n_q,):
                raise ValueError("q_rc must hold one flag per query")
        if out is None:
            status, score = np.zeros((n_q, n_t), np.int32), np.zeros((n_q, n_t), np.uint32)
            stride = n_t
        else:
            try:
                status, score = out
            except (TypeError, ValueError):
                raise ValueError("out must be a pair (status, score) of arrays") from None
            if not (isinstance(status, np.ndarray) and isinstance(score, np.ndarray)):
                raise ValueError("out must be a pair (status, score) of arrays")
            if status.dtype != np.int32 or score.dtype != np.uint32:
                raise ValueError("out arrays must be int32 (status) and uint32 (score)")
            if status.shape != (n_q, n_t) or score.shape != (n_q, n_t):
                raise ValueError(f"out arrays must have shape ({n_q}, {n_t})")
            if not (status.flags.writeable and score.flags.writeable):
                raise ValueError("out arrays must be writeable")
            rows = [a.strides[0] for a in (status, score)] if n_q > 1 else [4 * n_t, 4 * n_t]
            if n_t > 1 and (status.strides[1] != 4 or score.strides[1] != 4):
                raise ValueError("out arrays must be contiguous within a row")
            if rows[0] != rows[1] or rows[0] % 4 or rows[0] < 4 * n_t:
                raise ValueError("out arrays must share one row stride of at least n_t elements")
            stride = rows[0] // 4
        if n_q == 0 or n_t == 0:
            return status, score
        prm = self._params()
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        if q_rc is None:
            name = "wfahip_score_matrix"
            rc = L.lib().wfahip_score_matrix(self._ctx, C.byref(prm), vp(blob), blob.size, vp(q_off), vp(q_len), n_q, vp(t_off), vp(t_len), n_t,
                                             int(max_score), vp(status), vp(score), stride)
        else:
            name = "wfahip_score_matrix_rc"
            rc = L.lib().wfahip_score_matrix_rc(self._ctx, C.byref(prm), vp(blob), blob.size, vp(q_off), vp(q_len), n_q, vp(q_rc), vp(t_off),
                                                vp(t_len), n_t, int(max_score), vp(status), vp(score), stride)
        L.check(rc, name + (f" ({L.lib().wfahip_last_error(self._ctx).decode(errors='replace')})" if rc else ""))
        return status, score

    def ScoreMatrix(self, qs: Sequence[bytes], ts: Optional[Sequence[bytes]] = None, max_score: int = 0, strands: str = "+"):
        """(status, score) arrays of shape (len(qs), len(ts)): every query against every target (see score_matrix_arrays).
        ts=None: all against all (qs against qs; each sequence is uploaded once).
        strands="both": every query runs in both orientations -- each is listed twice, once flagged (score_matrix_arrays' q_rc), in ONE
        call over ONE blob; the entry's table then holds a query's words twice, once per row (and with ts=None a third time as a target:
        the row list is no longer the target list) -- and (status, score, strand) come back, the better strand per cell: strand 0 forward, 1 reverse complement.  An OK strand
        beats one that is not; of two OK strands the lower score wins and a tie goes to the forward one; when neither is OK the status
        is OVER_MAX if both are OVER_MAX and the forward strand's otherwise (strand 0)."""
        if strands not in ("+", "both"):
            raise ValueError('strands must be "+" or "both"')
        both = strands == "both"
        n_q = len(qs)
        seqs = list(qs) + ([] if ts is None else list(ts))
        blob, off, ln, _, _ = make_blob(seqs, [b""] * len(seqs))
        if not both:
            if ts is None:
                return self.score_matrix_arrays(blob, off, ln, off, ln, max_score=max_score)
            return self.score_matrix_arrays(blob, off[:n_q], ln[:n_q], off[n_q:], ln[n_q:], max_score=max_score)
        # rows 0 .. n_q - 1 forward, rows n_q .. 2 n_q - 1 the same queries flagged (the blob holds a sequence once: offsets repeat)
        q_off, q_len = np.concatenate([off[:n_q], off[:n_q]]), np.concatenate([ln[:n_q], ln[:n_q]])
        t_off, t_len = (off[:n_q], ln[:n_q]) if ts is None else (off[n_q:], ln[n_q:])
        q_rc = np.repeat(np.array([0, 1], np.uint8), n_q)
        st, sc = self.score_matrix_arrays(blob, q_off, q_len, t_off, t_len, max_score=max_score, q_rc=q_rc)
        return best_strand(st[:n_q], sc[:n_q], st[n_q:], sc[n_q:])

    # -- new: one pair at a time behind the batch ----------------------------------------------------
    def Submit(self, q: bytes, t: bytes) -> int:
        """Hand in one pair (copied) and return its ticket; Collect() aligns everything submitted as ONE batch.  This is
        how a per-pair loop like the reference's CLI (wfa-go/wfa-go.go:166-178) is served at batch throughput."""
        ticket = C.c_uint64()
        L.check(L.lib().wfahip_submit(self._ctx, q, len(q), t, len(t), C.byref(ticket)), "wfahip_submit")
        return int(ticket.value)

    def Pending(self) -> int:
        return int(L.lib().wfahip_pending(self._ctx))

    def Collect(self):
        """([]*AlignmentResult, []error) of the pairs submitted since the last Collect, indexed by ticket."""
        n = self.Pending()
        res = L.Results()
        prm = self._params()
        L.check(L.lib().wfahip_collect(self._ctx, C.byref(prm), C.byref(res)), "wfahip_collect")
        return _results_and_errors(_take_results(res, n))

    def AlignBatch(self, qs: Sequence[bytes], ts: Sequence[bytes], max_score: int = 0):
        """([]*AlignmentResult, []error): per-pair results and per-pair errors (None = ok).  max_score > 0: a pair whose
        score exceeds it has no result and ErrOverMaxScore in the error list (see align_arrays)."""
        if len(qs) != len(ts):
            raise ValueError("qs and ts differ in length")
        if not qs:
            return [], []
        return _results_and_errors(self.align_arrays(*make_blob(qs, ts), max_score=max_score))

    # -- diagnostics ----------------------------------------------------------------------------
    def last_timing(self) -> Timing:
        t = L.Timing()
        L.check(L.lib().wfahip_last_timing(self._ctx, C.byref(t)))
        return Timing(t.kernel_ms, t.total_ms, t.n_launches, t.n_retried_pairs, t.cells_stored, t.ops_written,
                      t.arena_bytes, t.main_kernel_ms, t.n_main_launches, t.n_packed_pairs, t.main_kernel_kind, t.ladder_start_level)

    def set_option(self, key: str, value: int) -> None:
        L.check(L.lib().wfahip_set_option(self._ctx, key.encode(), int(value)), f"set_option({key})")

    def debug_team_compact(self, q: bytes, t: bytes):
        """The rows wfa_teamc_kernel leaves in its arena for one pair (include/wfa_hip.h: wfahip_debug_team_compact; option
        team_wgs must be set): ({score: {diagonal: backtrace word}}, AlignmentResult)."""
        rows, words = C.POINTER(L.Row)(), C.POINTER(C.c_uint32)()
        n_rows, n_words = C.c_uint64(), C.c_uint64()
        res = L.Results()
        prm = self._params()
        L.check(L.lib().wfahip_debug_team_compact(self._ctx, C.byref(prm), q, len(q), t, len(t), C.byref(rows),
                                                  C.byref(n_rows), C.byref(words), C.byref(n_words), C.byref(res)),
                "wfahip_debug_team_compact")
        try:
            out = {}
            for i in range(n_rows.value):
                r = rows[i]
                out[int(r.score)] = {r.lo + j: int(words[r.word_off + j]) for j in range(r.width)}
            br = BatchResult.from_c(res, 1)
        finally:
            L.lib().wfahip_free(rows)
            L.lib().wfahip_free(words)
            L.lib().wfahip_results_free(C.byref(res))
        return out, br.result(0)

    def debug_wavefronts(self, q: bytes, t: bytes):
        """All stored M/I/D rows of one alignment: ({'M': {s: {k: raw}}, 'I': .., 'D': ..}, AlignmentResult)."""
        rows, words = C.POINTER(L.Row)(), C.POINTER(C.c_uint32)()
        n_rows, n_words = C.c_uint64(), C.c_uint64()
        res = L.Results()
        prm = self._params()
        L.check(L.lib().wfahip_debug_wavefronts(self._ctx, C.byref(prm), q, len(q), t, len(t), C.byref(rows),
                                                C.byref(n_rows), C.byref(words), C.byref(n_words), C.byref(res)),
                "wfahip_debug_wavefronts")
        try:
            out = {"M": {}, "I": {}, "D": {}}
            for i in range(n_rows.value):
                r = rows[i]
                for ci, name in enumerate("MID"):
                    d = {}
                    for j in range(r.width):
                        w = words[r.word_off + ci * r.width + j]
                        if w:
                            d[r.lo + j] = int(w)
                    if d:
                        out[name][int(r.score)] = d
            br = BatchResult.from_c(res, 1)
        finally:
            L.lib().wfahip_free(rows)
            L.lib().wfahip_free(words)
            L.lib().wfahip_results_free(C.byref(res))
        return out, br.result(0)

    def debug_compact_arena(self, pair: int):
        """(words, fmt, meta) of pair `pair` of the most recent batch: the compact backtrace arena as the first-pass
        forward kernel left it (include/wfa_hip.h: wfahip_debug_compact_arena)."""
        words = C.POINTER(C.c_uint32)()
        n_words, fmt, meta = C.c_uint64(), C.c_uint32(), (C.c_uint32 * 4)()
        L.check(L.lib().wfahip_debug_compact_arena(self._ctx, pair, C.byref(words), C.byref(n_words), C.byref(fmt),
                                                   C.byref(meta)), "wfahip_debug_compact_arena")
        try:
            arr = np.ctypeslib.as_array(words, shape=(int(n_words.value),)).copy()
        finally:
            L.lib().wfahip_free(words)
        return arr, int(fmt.value), tuple(int(x) for x in meta)

    def debug_wide_plan(self, q_len, t_len):
        """(lists, counts, longest, ladder) of the length-class plan of a semi-global batch with these lengths, from the plan
        kernels alone (include/wfa_hip.h: wfahip_debug_wide_plan): lists[c] = the pair indices of class c of
        wide_class_bounds(), ascending; counts / longest per class; ladder = the pairs wfa_wide_kernel is not offered."""
        q_len = np.ascontiguousarray(q_len, dtype=np.uint32)
        t_len = np.ascontiguousarray(t_len, dtype=np.uint32)
        n, nc = int(len(q_len)), len(wide_class_bounds())
        if len(t_len) != n:
            raise ValueError("q_len and t_len differ in length")
        ids = C.POINTER(C.c_uint32)()
        counts, longest, n_ladder = (C.c_uint64 * nc)(), (C.c_uint32 * nc)(), C.c_uint64()
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        L.check(L.lib().wfahip_debug_wide_plan(self._ctx, vp(q_len), vp(t_len), n, C.byref(ids), counts, longest, C.byref(n_ladder)),
                "wfahip_debug_wide_plan")
        try:
            flat = np.ctypeslib.as_array(ids, shape=(n,)).copy() if n else np.zeros(0, dtype=np.uint32)
        finally:
            L.lib().wfahip_free(ids)
        counts = [int(c) for c in counts]
        cuts = np.cumsum([0] + counts)
        lists = [flat[cuts[c]:cuts[c + 1]] for c in range(nc)]
        return lists, counts, [int(x) for x in longest], flat[cuts[nc]:cuts[nc] + int(n_ladder.value)]

    def debug_prepack(self, blob, q_off, q_len, t_off, t_len, seq_words: int, ppw: int = 4, work=None):
        """The slots wfa_prepack_kernel makes of a batch on the aligner's GPU (include/wfa_hip.h: wfahip_debug_prepack): torch tensors
        in, as align_tensors takes them; work: an int32 tensor of pair indices (slot i = pair work[i]) or None (slot i = pair i).
        Returns uint32 [n, 4 + 2 * seq_words]; a word the kernel did not store reads 0xA5A5A5A5."""
        import torch
        dev = self._want_tensor("blob", blob, torch.uint8)
        for name, t, dtype in (("q_off", q_off, torch.int64), ("q_len", q_len, torch.int32), ("t_off", t_off, torch.int64),
                               ("t_len", t_len, torch.int32)):
            self._want_tensor(name, t, dtype, dev)
        if work is not None:
            self._want_tensor("work", work, torch.int32, dev)
        n = int(work.numel() if work is not None else q_len.numel())
        slots = np.zeros((n, 4 + 2 * int(seq_words)), dtype=np.uint32)
        torch.cuda.current_stream(dev).synchronize()
        L.check(L.lib().wfahip_debug_prepack(self._ctx, blob.data_ptr(), q_off.data_ptr(), q_len.data_ptr(), t_off.data_ptr(), t_len.data_ptr(),
                                             work.data_ptr() if work is not None else None, n, int(seq_words), int(ppw),
                                             slots.ctypes.data_as(C.c_void_p)), "wfahip_debug_prepack")
        return slots

    def Plot(self, q: bytes, t: bytes, component: str = "M", notChangeToMatch: bool = False, maxScore: int = -1) -> str:
        """(*Aligner).Plot (wfa_component_plot.go:41): the component table, from the DEVICE wavefronts of one pair."""
        wf, _ = self.debug_wavefronts(q, t)
        return plot_component(q, t, wf, component, self.p, notChangeToMatch, maxScore)

    def close(self):
        if getattr(self, "_ctx", None):
            L.lib().wfahip_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _take_results(res: "L.Results", n: int) -> "BatchResult":
    """numpy copies of a wfahip_results, which is then handed back to the library."""
    try:
        return BatchResult.from_c(res, n)
    finally:
        L.lib().wfahip_results_free(C.byref(res))


def _take_cigars(cig: "L.Cigars"):
    """numpy copies (text uint8 [n_bytes], off uint64 [n + 1]) of a wfahip_cigars, which stays the caller's to free"""
    n, nb = int(cig.n), int(cig.n_bytes)
    text = np.ctypeslib.as_array(cig.text, shape=(nb,)).copy() if nb else np.zeros(0, dtype=np.uint8)
    off = np.ctypeslib.as_array(cig.off, shape=(n + 1,)).copy() if cig.off else np.zeros(n + 1, dtype=np.uint64)
    return text, off


def cigar_text(batch_result: "BatchResult", only_aligned: bool = False, n_threads: int = 8):
    """AlignmentResult.CIGAR(only_aligned) of every pair of a BatchResult as bytes, rendered by host threads (include/wfa_hip.h:
    wfahip_cigar_text; no GPU, no Aligner): returns (text np.uint8, off np.uint64 [n + 1]); pair i's text is
    text[off[i]:off[i + 1]], empty for a pair that is not OK and, under only_aligned, for one without an M op.  ValueError for
    arrays of the wrong shape; WfaHipError (ERR_BAD_ARG) when an OK pair's ops lie outside batch_result.ops."""
    br = batch_result
    status = np.ascontiguousarray(br.status, dtype=np.int32)
    ops_off = np.ascontiguousarray(br.ops_off, dtype=np.uint64)
    ops_len = np.ascontiguousarray(br.ops_len, dtype=np.uint32)
    ops = np.ascontiguousarray(br.ops, dtype=np.uint64)
    n = int(status.size)
    if status.ndim != 1 or ops.ndim != 1 or ops_off.shape != (n,) or ops_len.shape != (n,):
        raise ValueError("status, ops_off and ops_len must be one-dimensional and of one length, ops one-dimensional")
    if int(n_threads) < 1:
        raise ValueError("n_threads must be at least 1")
    res = L.Results()
    res.n, res.n_ops = n, int(ops.size)
    res.status = status.ctypes.data_as(C.POINTER(C.c_int32))
    res.ops_off = ops_off.ctypes.data_as(C.POINTER(C.c_uint64))
    res.ops_len = ops_len.ctypes.data_as(C.POINTER(C.c_uint32))
    res.ops = ops.ctypes.data_as(C.POINTER(C.c_uint64))
    cig = L.Cigars()
    L.check(L.lib().wfahip_cigar_text(C.byref(res), 1 if only_aligned else 0, int(n_threads), C.byref(cig)), "wfahip_cigar_text")
    try:
        return _take_cigars(cig)
    finally:
        L.lib().wfahip_cigars_free(C.byref(cig))


def alignment_text(batch_result: "BatchResult", blob, q_off, q_len, t_off, t_len, only_aligned: bool = False, n_threads: int = 8):
    """AlignmentResult.AlignmentText(q, t, only_aligned) of every pair of a BatchResult over the blob and arrays it was aligned from,
    rendered by host threads (include/wfa_hip.h: wfahip_alignment_text; no GPU, no Aligner): returns (q_row np.uint8, a_row
    np.uint8, t_row np.uint8, off np.uint64 [n + 1]); pair i's rows are the three arrays' [off[i]:off[i + 1]], empty for a pair
    that is not OK and, under only_aligned, for one without an M op.  ValueError for arrays of the wrong shape; WfaHipError
    (ERR_BAD_ARG) when an OK pair's ops lie outside batch_result.ops, or its ops or windows leave the sequences."""
    blob = np.ascontiguousarray(blob, dtype=np.uint8)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    return _host_rows(batch_result, blob, "blob", q_off, q_len, t_off, t_len, None, n_threads,
                      lambda res, q_off, q_len, t_off, t_len, q_rc, txt: L.lib().wfahip_alignment_text(
                          C.byref(res), vp(blob), blob.size, vp(q_off), vp(q_len), vp(t_off), vp(t_len), 1 if only_aligned else 0,
                          int(n_threads), C.byref(txt)), "wfahip_alignment_text")


def alignment_text_packed(batch_result: "BatchResult", packed, q_woff, q_len, t_woff, t_len, q_rc=None, only_aligned: bool = False,
                          n_threads: int = 8):
    """alignment_text over 2-bit words, both strands (include/wfa_hip.h: wfahip_alignment_text_packed; no GPU, no Aligner): the rows
    of a BatchResult of align_arrays_packed_rc (or align_arrays_packed, q_rc=None) from the words, offsets, lengths and flags it was
    aligned from.  The query row of a flagged pair holds the reverse complement of its query, the strand its record and ops speak
    of.  Returns and errors as alignment_text."""
    packed = np.ascontiguousarray(packed, dtype=np.uint32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    return _host_rows(batch_result, packed, "packed", q_woff, q_len, t_woff, t_len, q_rc, n_threads,
                      lambda res, q_woff, q_len, t_woff, t_len, q_rc, txt: L.lib().wfahip_alignment_text_packed(
                          C.byref(res), vp(packed), packed.size, vp(q_woff), vp(q_len), vp(t_woff), vp(t_len), vp(q_rc),
                          1 if only_aligned else 0, int(n_threads), C.byref(txt)), "wfahip_alignment_text_packed")


def diff_text(batch_result: "BatchResult", blob, q_off, q_len, t_off, t_len, only_aligned: bool = False, n_threads: int = 8):
    """The difference string (minimap2's cs tag, short form) of every pair of a BatchResult over the blob and arrays it was aligned
    from, rendered by host threads (include/wfa_hip.h: wfahip_diff_text; no GPU, no Aligner): returns (text np.uint8, off np.uint64
    [n + 1]); pair i's string is text[off[i]:off[i + 1]], with the target as its reference sequence -- ':' and a count per M op, '*'
    target base, query base per X column, '-' and the target's bases per I op, '+' and the query's per D or H op, bases in lower
    case.  Empty strings, ValueErrors and WfaHipError (ERR_BAD_ARG) as alignment_text."""
    blob = np.ascontiguousarray(blob, dtype=np.uint8)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    return _host_rows(batch_result, blob, "blob", q_off, q_len, t_off, t_len, None, n_threads,
                      lambda res, q_off, q_len, t_off, t_len, q_rc, cig: L.lib().wfahip_diff_text(
                          C.byref(res), vp(blob), blob.size, vp(q_off), vp(q_len), vp(t_off), vp(t_len), 1 if only_aligned else 0,
                          int(n_threads), C.byref(cig)), "wfahip_diff_text", diff=True)


def diff_text_packed(batch_result: "BatchResult", packed, q_woff, q_len, t_woff, t_len, q_rc=None, only_aligned: bool = False,
                     n_threads: int = 8):
    """diff_text over 2-bit words, both strands (include/wfa_hip.h: wfahip_diff_text_packed; no GPU, no Aligner): the strings of a
    BatchResult of align_arrays_packed_rc (or align_arrays_packed, q_rc=None) from the words, offsets, lengths and flags it was
    aligned from.  The string of a flagged pair spells the bases of the reverse complement of its query, the strand its record and
    ops speak of.  Returns and errors as diff_text."""
    packed = np.ascontiguousarray(packed, dtype=np.uint32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    return _host_rows(batch_result, packed, "packed", q_woff, q_len, t_woff, t_len, q_rc, n_threads,
                      lambda res, q_woff, q_len, t_woff, t_len, q_rc, cig: L.lib().wfahip_diff_text_packed(
                          C.byref(res), vp(packed), packed.size, vp(q_woff), vp(q_len), vp(t_woff), vp(t_len), vp(q_rc),
                          1 if only_aligned else 0, int(n_threads), C.byref(cig)), "wfahip_diff_text_packed", diff=True)


def pileup(batch_result: "BatchResult", blob, q_off, q_len, t_off, t_len, pile_at, pile_n, only_aligned: bool = False, n_threads: int = 8,
           out=None):
    """What the alignments of a BatchResult say about every base of the window [pile_at, pile_at + pile_n) of the blob it was aligned
    from, counted by host threads (include/wfa_hip.h: wfahip_pileup; no GPU, no Aligner): returns counts np.uint32 [pile_n, 8] -- per
    byte of the blob as a TARGET base the alignments that put A, C, T, G or another byte over it, those in which it faces a gap, the
    runs of query-only bases behind it and their bases (the PILE_W_* words).  out=: a C-contiguous uint32 array of that shape that the
    call ADDS to and returns.  ValueErrors and WfaHipError (ERR_BAD_ARG, the counts untouched) as alignment_text."""
    blob = np.ascontiguousarray(blob, dtype=np.uint8)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    return _host_pileup(batch_result, blob, "blob", q_off, q_len, t_off, t_len, None, n_threads, pile_at, pile_n, out,
                        lambda res, q_off, q_len, t_off, t_len, q_rc, tail: L.lib().wfahip_pileup(
                            C.byref(res), vp(blob), blob.size, vp(q_off), vp(q_len), vp(t_off), vp(t_len), 1 if only_aligned else 0,
                            int(n_threads), *tail), "wfahip_pileup")


def pileup_packed(batch_result: "BatchResult", packed, q_woff, q_len, t_woff, t_len, pile_at, pile_n, q_rc=None, only_aligned: bool = False,
                  n_threads: int = 8, out=None):
    """pileup over 2-bit words, both strands (include/wfa_hip.h: wfahip_pileup_packed; no GPU, no Aligner): the window counts in bases
    of the words' storage, base p of the sequence at word woff being 16 * woff + p; a flagged pair adds the bases of the reverse
    complement of its query.  Returns, out= and errors as pileup."""
    packed = np.ascontiguousarray(packed, dtype=np.uint32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    return _host_pileup(batch_result, packed, "packed", q_woff, q_len, t_woff, t_len, q_rc, n_threads, pile_at, pile_n, out,
                        lambda res, q_woff, q_len, t_woff, t_len, q_rc, tail: L.lib().wfahip_pileup_packed(
                            C.byref(res), vp(packed), packed.size, vp(q_woff), vp(q_len), vp(t_woff), vp(t_len), vp(q_rc),
                            1 if only_aligned else 0, int(n_threads), *tail), "wfahip_pileup_packed")


def _host_pileup(br, seqs, seqs_name, q_off, q_len, t_off, t_len, q_rc, n_threads, pile_at, pile_n, out, call, what):
    """what the host pileups share: _host_rows' arrays and checks, the window and out= checked, call(res, q_off, q_len, t_off, t_len,
    q_rc, tail) -- the C entry, tail its last four arguments"""
    status = np.ascontiguousarray(br.status, dtype=np.int32)
    ops_off = np.ascontiguousarray(br.ops_off, dtype=np.uint64)
    ops_len = np.ascontiguousarray(br.ops_len, dtype=np.uint32)
    ops = np.ascontiguousarray(br.ops, dtype=np.uint64)
    windows = [np.ascontiguousarray(getattr(br, f), dtype=np.int32) for f in ("qbegin", "qend", "tbegin", "tend")]
    q_off = np.ascontiguousarray(q_off, dtype=np.uint64)
    t_off = np.ascontiguousarray(t_off, dtype=np.uint64)
    q_len = np.ascontiguousarray(q_len, dtype=np.uint32)
    t_len = np.ascontiguousarray(t_len, dtype=np.uint32)
    n = int(status.size)
    if status.ndim != 1 or ops.ndim != 1 or seqs.ndim != 1:
        raise ValueError(f"status, ops and {seqs_name} must be one-dimensional")
    if any(a.shape != (n,) for a in [ops_off, ops_len, q_off, q_len, t_off, t_len] + windows):
        raise ValueError("ops_off, ops_len, qbegin, qend, tbegin, tend and the offset and length arrays must hold one element per pair")
    if q_rc is not None:
        q_rc = np.ascontiguousarray(q_rc, dtype=np.uint8)
        if q_rc.shape != (n,):
            raise ValueError("q_rc must hold one flag per pair")
    if int(n_threads) < 1:
        raise ValueError("n_threads must be at least 1")
    pile_at, pile_n = int(pile_at), int(pile_n)
    if not 0 <= pile_at < 1 << 64 or not 0 <= pile_n <= L.PILE_MAX_N:
        raise ValueError("pile_at must fit 64 bits and pile_n lie in [0, 2^61 / 8]")
    if out is None:
        counts = np.zeros((pile_n, L.PILE_WORDS), dtype=np.uint32)
    else:
        counts = out
        if not isinstance(counts, np.ndarray) or counts.dtype != np.uint32 or counts.shape != (pile_n, L.PILE_WORDS) or \
                not counts.flags.c_contiguous or not counts.flags.writeable:
            raise ValueError(f"out must be a writeable C-contiguous uint32 array [{pile_n}, {L.PILE_WORDS}]")
    res = L.Results()
    res.n, res.n_ops = n, int(ops.size)
    res.status = status.ctypes.data_as(C.POINTER(C.c_int32))
    res.ops_off = ops_off.ctypes.data_as(C.POINTER(C.c_uint64))
    res.ops_len = ops_len.ctypes.data_as(C.POINTER(C.c_uint32))
    res.ops = ops.ctypes.data_as(C.POINTER(C.c_uint64))
    res.qbegin, res.qend, res.tbegin, res.tend = (a.ctypes.data_as(C.POINTER(C.c_int32)) for a in windows)
    cnt = C.c_uint64(0)
    tail = (pile_at, pile_n, counts.ctypes.data_as(C.c_void_p) if pile_n else None, C.byref(cnt))
    L.check(call(res, q_off, q_len, t_off, t_len, q_rc, tail), what)
    return counts


def check_alignments(batch_result: "BatchResult", blob, q_off, q_len, t_off, t_len, penalties=None, options=None, adaptive=None,
                     mask: int = L.CHK_ALL, n_threads: int = 8):
    """The verdict on every pair of a BatchResult over the blob and arrays it was aligned from, computed by host threads
    (include/wfa_hip.h: wfahip_check_alignments; no GPU, no Aligner): returns (chk np.uint32 [n, 8], passed np.int32 [n],
    n_flagged int) -- FLAGS, COST, Q_USED, T_USED, N_BAD, FIRST_BAD, 0, 0 per pair; the record's status, PAIR_OK or
    PAIR_CHECK_FAILED under mask; the number of OK pairs with a flag of the mask.  penalties / options / adaptive are the ones the
    batch was aligned under (defaults: DefaultPenalties, DefaultOptions, none); the rule reads the penalties and GlobalAlignment.
    ValueError for arrays of the wrong shape.  A bad pair is a flag, never an error."""
    blob = np.ascontiguousarray(blob, dtype=np.uint8)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    return _host_check(batch_result, blob, "blob", q_off, q_len, t_off, t_len, None, penalties, options, adaptive, mask, n_threads,
                       lambda res, prm, q_off, q_len, t_off, t_len, q_rc, tail: L.lib().wfahip_check_alignments(
                           C.byref(res), C.byref(prm), vp(blob), blob.size, vp(q_off), vp(q_len), vp(t_off), vp(t_len), *tail),
                       "wfahip_check_alignments")


def check_alignments_packed(batch_result: "BatchResult", packed, q_woff, q_len, t_woff, t_len, q_rc=None, penalties=None, options=None,
                            adaptive=None, mask: int = L.CHK_ALL, n_threads: int = 8):
    """check_alignments over 2-bit words, both strands (include/wfa_hip.h: wfahip_check_alignments_packed; no GPU, no Aligner): the
    verdicts on a BatchResult of align_arrays_packed_rc (or align_arrays_packed, q_rc=None) from the words, offsets, lengths and
    flags it was aligned from.  Returns and errors as check_alignments."""
    packed = np.ascontiguousarray(packed, dtype=np.uint32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    return _host_check(batch_result, packed, "packed", q_woff, q_len, t_woff, t_len, q_rc, penalties, options, adaptive, mask, n_threads,
                       lambda res, prm, q_woff, q_len, t_woff, t_len, q_rc, tail: L.lib().wfahip_check_alignments_packed(
                           C.byref(res), C.byref(prm), vp(packed), packed.size, vp(q_woff), vp(q_len), vp(t_woff), vp(t_len), vp(q_rc),
                           *tail), "wfahip_check_alignments_packed")


def _host_check(br, seqs, seqs_name, q_off, q_len, t_off, t_len, q_rc, penalties, options, adaptive, mask, n_threads, call, what):
    """what the host checks share: the arrays made contiguous and checked, the wfahip_results view of the BatchResult, the params,
    call(res, prm, q_off, q_len, t_off, t_len, q_rc, tail) -- the C entry, tail its last five arguments"""
    i32 = ("status", "tbegin", "tend", "qbegin", "qend")
    u32 = ("score", "align_len", "matches", "gaps", "gap_regions", "ops_len")
    f = {k: np.ascontiguousarray(getattr(br, k), dtype=np.int32) for k in i32}
    f.update({k: np.ascontiguousarray(getattr(br, k), dtype=np.uint32) for k in u32})
    f["ops_off"] = np.ascontiguousarray(br.ops_off, dtype=np.uint64)
    ops = np.ascontiguousarray(br.ops, dtype=np.uint64)
    q_off = np.ascontiguousarray(q_off, dtype=np.uint64)
    t_off = np.ascontiguousarray(t_off, dtype=np.uint64)
    q_len = np.ascontiguousarray(q_len, dtype=np.uint32)
    t_len = np.ascontiguousarray(t_len, dtype=np.uint32)
    n = int(f["status"].size)
    if f["status"].ndim != 1 or ops.ndim != 1 or seqs.ndim != 1:
        raise ValueError(f"status, ops and {seqs_name} must be one-dimensional")
    if any(a.shape != (n,) for a in list(f.values()) + [q_off, q_len, t_off, t_len]):
        raise ValueError("the fields of the result and the offset and length arrays must hold one element per pair")
    if q_rc is not None:
        q_rc = np.ascontiguousarray(q_rc, dtype=np.uint8)
        if q_rc.shape != (n,):
            raise ValueError("q_rc must hold one flag per pair")
    if int(n_threads) < 1:
        raise ValueError("n_threads must be at least 1")
    if not 0 <= int(mask) <= 0xFFFFFFFF:
        raise ValueError("mask must fit 32 bits")
    pen = penalties if penalties is not None else DefaultPenalties
    opt = options if options is not None else DefaultOptions
    prm = L.Params(pen.Mismatch, pen.GapOpen, pen.GapExt, 1 if opt.GlobalAlignment else 0, 0)
    if adaptive is not None:
        prm.adaptive = 1
        prm.min_wf_len, prm.max_dist_diff, prm.cutoff_step = adaptive.MinWFLen, adaptive.MaxDistDiff, adaptive.CutoffStep
    res = L.Results()
    res.n, res.n_ops = n, int(ops.size)
    for k in i32:
        setattr(res, k, f[k].ctypes.data_as(C.POINTER(C.c_int32)))
    for k in u32:
        setattr(res, k, f[k].ctypes.data_as(C.POINTER(C.c_uint32)))
    res.ops_off = f["ops_off"].ctypes.data_as(C.POINTER(C.c_uint64))
    res.ops = ops.ctypes.data_as(C.POINTER(C.c_uint64))
    chk = np.zeros((n, L.CHK_WORDS), dtype=np.uint32)
    passed = np.zeros(n, dtype=np.int32)
    cnt = C.c_uint64(0)
    tail = (int(mask), int(n_threads), chk.ctypes.data_as(C.c_void_p), passed.ctypes.data_as(C.c_void_p), C.byref(cnt))
    L.check(call(res, prm, q_off, q_len, t_off, t_len, q_rc, tail), what)
    return chk, passed, int(cnt.value)


def _host_rows(br, seqs, seqs_name, q_off, q_len, t_off, t_len, q_rc, n_threads, call, what, diff=False):
    """what the host row renderers share: the arrays made contiguous and checked, the wfahip_results view of the BatchResult,
    call(res, q_off, q_len, t_off, t_len, q_rc, txt) -- the C entry --, and the rows copied out of its struct.  diff: the struct is a
    wfahip_cigars and (text, off) is returned -- the difference string's host functions"""
    status = np.ascontiguousarray(br.status, dtype=np.int32)
    ops_off = np.ascontiguousarray(br.ops_off, dtype=np.uint64)
    ops_len = np.ascontiguousarray(br.ops_len, dtype=np.uint32)
    ops = np.ascontiguousarray(br.ops, dtype=np.uint64)
    windows = [np.ascontiguousarray(getattr(br, f), dtype=np.int32) for f in ("qbegin", "qend", "tbegin", "tend")]
    q_off = np.ascontiguousarray(q_off, dtype=np.uint64)
    t_off = np.ascontiguousarray(t_off, dtype=np.uint64)
    q_len = np.ascontiguousarray(q_len, dtype=np.uint32)
    t_len = np.ascontiguousarray(t_len, dtype=np.uint32)
    n = int(status.size)
    if status.ndim != 1 or ops.ndim != 1 or seqs.ndim != 1:
        raise ValueError(f"status, ops and {seqs_name} must be one-dimensional")
    if any(a.shape != (n,) for a in [ops_off, ops_len, q_off, q_len, t_off, t_len] + windows):
        raise ValueError("ops_off, ops_len, qbegin, qend, tbegin, tend and the offset and length arrays must hold one element per pair")
    if q_rc is not None:
        q_rc = np.ascontiguousarray(q_rc, dtype=np.uint8)
        if q_rc.shape != (n,):
            raise ValueError("q_rc must hold one flag per pair")
    if int(n_threads) < 1:
        raise ValueError("n_threads must be at least 1")
    res = L.Results()
    res.n, res.n_ops = n, int(ops.size)
    res.status = status.ctypes.data_as(C.POINTER(C.c_int32))
    res.ops_off = ops_off.ctypes.data_as(C.POINTER(C.c_uint64))
    res.ops_len = ops_len.ctypes.data_as(C.POINTER(C.c_uint32))
    res.ops = ops.ctypes.data_as(C.POINTER(C.c_uint64))
    res.qbegin, res.qend, res.tbegin, res.tend = (a.ctypes.data_as(C.POINTER(C.c_int32)) for a in windows)
    if diff:
        cig = L.Cigars()
        L.check(call(res, q_off, q_len, t_off, t_len, q_rc, cig), what)
        try:
            return _take_cigars(cig)
        finally:
            L.lib().wfahip_cigars_free(C.byref(cig))
    txt = L.AlignTexts()
    L.check(call(res, q_off, q_len, t_off, t_len, q_rc, txt), what)
    try:
        nb = int(txt.n_bytes)
        rows = [np.ctypeslib.as_array(p, shape=(nb,)).copy() if nb else np.zeros(0, dtype=np.uint8) for p in (txt.q_row, txt.a_row, txt.t_row)]
        off = np.ctypeslib.as_array(txt.off, shape=(n + 1,)).copy()
    finally:
        L.lib().wfahip_align_texts_free(C.byref(txt))
    return rows[0], rows[1], rows[2], off


def _results_and_errors(br: "BatchResult"):
    results: List[Optional[AlignmentResult]] = []
    errors: List[Optional[Exception]] = []
    for i in range(len(br.status)):
        st = int(br.status[i])
        if st == L.PAIR_OK:
            results.append(br.result(i))
            errors.append(None)
        else:
            results.append(None)
            errors.append(ErrEmptySeq if st == L.PAIR_EMPTY else ErrSeqTooLong if st == L.PAIR_TOO_LONG
                          else ErrOverMaxScore if st == L.PAIR_OVER_MAX
                          else WfaError("wfa: out of device memory for this pair"))
    return results, errors


def wide_class_bounds() -> List[int]:
    """Upper bounds of the length classes semi-global batches are cut into (include/wfa_hip.h: wfahip_wide_class_bounds):
    strictly ascending, the last one 2 047.  Host only."""
    n = L.lib().wfahip_wide_class_bounds(None, 0)
    b = (C.c_uint32 * n)()
    L.lib().wfahip_wide_class_bounds(b, n)
    return [int(x) for x in b]


def best_strand(st_f, sc_f, st_r, sc_r):
    """The better of a forward and a reverse-strand result per element -> (status, score, strand): OK beats any other status, of two
    OK results the lower score wins and a tie goes to the forward strand (0); when neither is OK the status is OVER_MAX if both are
    OVER_MAX and the forward strand's otherwise, with strand 0."""
    st_f, st_r = np.asarray(st_f, np.int32), np.asarray(st_r, np.int32)
    sc_f, sc_r = np.asarray(sc_f, np.uint32), np.asarray(sc_r, np.uint32)
    ok_f, ok_r = st_f == L.PAIR_OK, st_r == L.PAIR_OK
    rev = ok_r & (~ok_f | (sc_r < sc_f))
    status = np.where(rev, st_r, st_f)
    score = np.where(rev, sc_r, sc_f)
    return status.astype(np.int32), score.astype(np.uint32), rev.astype(np.uint8)


def revcomp_packed(words, length: int):
    """The reverse complement of one 2-bit packed sequence of `length` bases (include/wfa_hip.h: wfahip_revcomp_packed) as
    pack_pairs() would have written it: (length + 15) // 16 + 1 words, tail bits and pad word zero.  Host only."""
    words = np.ascontiguousarray(words, dtype=np.uint32)
    length = int(length)
    if length < 0 or words.size < (length + 15) // 16:
        raise ValueError("words does not hold `length` bases")
    dst = np.zeros((length + 15) // 16 + 1, dtype=np.uint32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    L.check(L.lib().wfahip_revcomp_packed(vp(words), length, vp(dst)), "wfahip_revcomp_packed")
    return dst


def pack_pairs(blob, q_off, q_len, t_off, t_len, n_threads: int = 8):
    """Host-side 2-bit packer (include/wfa_hip.h: wfahip_pack_pairs) -> (packed, q_woff, t_woff).  Raises WfaHipError
    (ERR_UNSUPPORTED) when a byte outside ACGT is found: such input must use the byte entry."""
    n = int(len(q_len))
    blob = np.ascontiguousarray(blob, dtype=np.uint8)
    q_off = np.ascontiguousarray(q_off, dtype=np.uint64)
    t_off = np.ascontiguousarray(t_off, dtype=np.uint64)
    q_len = np.ascontiguousarray(q_len, dtype=np.uint32)
    t_len = np.ascontiguousarray(t_len, dtype=np.uint32)
    words = int(((q_len.astype(np.uint64) + 15) // 16 + 1).sum() + ((t_len.astype(np.uint64) + 15) // 16 + 1).sum())
    packed = np.zeros(max(words, 1), dtype=np.uint32)
    q_woff = np.zeros(n, dtype=np.uint64)
    t_woff = np.zeros(n, dtype=np.uint64)
    n_words = C.c_uint64()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    L.check(L.lib().wfahip_pack_pairs(vp(blob), vp(q_off), vp(q_len), vp(t_off), vp(t_len), n, n_threads, vp(packed),
                                      vp(q_woff), vp(t_woff), C.byref(n_words)), "wfahip_pack_pairs")
    assert int(n_words.value) == words
    return packed, q_woff, t_woff


class MultiAligner:
    """One aligner over several GPUs (include/wfa_hip.h: wfahip_create_multi): AlignBatch cuts the batch into
    contiguous shards, one per GPU, each aligned from its own host thread; results come back in pair order.  The
    reference's model is one Aligner per goroutine (wfa.go:73-78); this is that, behind one call."""

    def __init__(self, p: Penalties = None, opt: Options = None, devices: Optional[Sequence[int]] = None):
        self.p = p or DefaultPenalties
        self.opt = opt or DefaultOptions
        self.ad: Optional[AdaptiveReductionOption] = None
        self._m = C.c_void_p()
        if devices is None:
            L.check(L.lib().wfahip_create_multi(None, 0, C.byref(self._m)), "wfahip_create_multi")
        else:
            ids = (C.c_int * len(devices))(*devices)
            L.check(L.lib().wfahip_create_multi(ids, len(devices), C.byref(self._m)), "wfahip_create_multi")

    AdaptiveReduction = Aligner.AdaptiveReduction
    _params = Aligner._params

    def size(self) -> int:
        return int(L.lib().wfahip_multi_size(self._m))

    def set_option(self, key: str, value: int) -> None:
        for i in range(self.size()):
            L.check(L.lib().wfahip_set_option(L.lib().wfahip_multi_ctx(self._m, i), key.encode(), int(value)))

    def align_arrays(self, blob, q_off, q_len, t_off, t_len) -> "BatchResult":
        n = int(len(q_len))
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        q_off = np.ascontiguousarray(q_off, dtype=np.uint64)
        t_off = np.ascontiguousarray(t_off, dtype=np.uint64)
        q_len = np.ascontiguousarray(q_len, dtype=np.uint32)
        t_len = np.ascontiguousarray(t_len, dtype=np.uint32)
        res = L.Results()
        prm = self._params()
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        L.check(L.lib().wfahip_align_batch_multi(self._m, C.byref(prm), vp(blob), blob.size, vp(q_off), vp(q_len),
                                                 vp(t_off), vp(t_len), n, C.byref(res)), "wfahip_align_batch_multi")
        return _take_results(res, n)

    def AlignBatch(self, qs: Sequence[bytes], ts: Sequence[bytes]):
        if len(qs) != len(ts):
            raise ValueError("qs and ts differ in length")
        if not qs:
            return [], []
        return _results_and_errors(self.align_arrays(*make_blob(qs, ts)))

    def close(self):
        if getattr(self, "_m", None):
            L.lib().wfahip_destroy_multi(self._m)
            self._m = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


WFA_ARROWS = "⊕⟼🠦↧🠧⬂⬊"  # wfa_backtrace_types.go:39: no type, InsOpen, InsExt, DelOpen, DelExt, Mismatch, Match


def plot_component(q: bytes, t: bytes, wavefronts: dict, component: str = "M", penalties: Penalties = None,
                   notChangeToMatch: bool = False, maxScore: int = -1) -> str:
    """The text table of (*Aligner).Plot (wfa_component_plot.go:41-209) for one component, built from the stored
    wavefront words {'M': {score: {k: raw}}, 'I': .., 'D': ..} (raw = offset<<3 | type) -- the form
    Aligner.debug_wavefronts returns from the device and the oracle's dump has.

    Every cell shows the first (lowest) score that reached it and the arrow of its type; with the M component,
    cells reached by extension become matches and only the cell a run started from keeps its type
    (wfa_component_plot.go:97-99,133-177)."""
    p = penalties or DefaultPenalties
    lenQ, lenT = len(q), len(t)
    M, I, D = wavefronts["M"], wavefronts["I"], wavefronts["D"]
    comp = wavefronts[component]
    isM = component == "M"
    m = [[-1] * lenT for _ in range(lenQ)]

    def after_diff(c, s, diff, k):  # Component.GetAfterDiff (wfa_component.go:158-167): 0 when missing
        if diff > s:
            return 0
        return c.get(s - diff, {}).get(k, 0) >> 3

    vp = hp = 0  # the reference declares them outside the loops (wfa_component_plot.go:66)
    for s in sorted(comp):
        if maxScore >= 0 and s > maxScore:
            break
        row = comp[s]
        for k in sorted(row):
            raw = row[k]
            offset, typ = raw >> 3, raw & 7
            h = offset - 1
            v = h - k
            if v < 0 or h < 0 or v >= lenQ or h >= lenT:
                continue
            if m[v][h] >= 0:  # recorded with a lower score
                continue
            m[v][h] = (s << 3) | typ
            if not isM or q[v] != t[h]:
                continue
            if typ == 2:  # InsExt
                offset0 = max(after_diff(M, s, p.GapOpen + p.GapExt, k - 1), after_diff(I, s, p.GapExt, k - 1)) + 1
            elif typ == 4:  # DelExt
                offset0 = max(after_diff(M, s, p.GapOpen + p.GapExt, k + 1), after_diff(D, s, p.GapExt, k + 1))
            else:
                isk = max(after_diff(M, s, p.GapOpen + p.GapExt, k - 1), after_diff(I, s, p.GapExt, k - 1)) + 1
                dsk = max(after_diff(M, s, p.GapOpen + p.GapExt, k + 1), after_diff(D, s, p.GapExt, k + 1))
                offset0 = max(isk, dsk, after_diff(M, s, p.Mismatch, k) + 1)
            h00 = offset0 - 1
            if h == h00:  # not extended at all
                continue
            v0, h0 = v, h
            if not notChangeToMatch:
                m[v0][h0] = (s << 3) | 6
            n = 0
            while True:
                h -= 1
                v -= 1
                if v < 0 or h < 0:
                    break
                n += 1
                if m[v][h] >= 0:
                    continue
                m[v][h] = (s << 3) | (typ if notChangeToMatch else 6)
                vp, hp = v, h
                if q[v] != t[h] or h == h00:
                    break
            if n == 0:
                vp, hp = v0, h0
            if not notChangeToMatch:
                m[vp][hp] = (s << 3) | typ  # the run's first cell keeps the original type
    out = ["   \t " + "".join("\t%3d" % (h + 1) for h in range(lenT)),
           "   \t " + "".join("\t%3s" % chr(b) for b in t)]
    for v in range(lenQ):
        cells = "".join("\t  ." if c < 0 else "\t%s%2d" % (WFA_ARROWS[c & 7], c >> 3) for c in m[v])
        out.append("%3d\t%s%s" % (v + 1, chr(q[v]), cells))
    return "\n".join(out) + "\n"


@dataclass
class BatchResult:
    status: np.ndarray
    score: np.ndarray
    tbegin: np.ndarray
    tend: np.ndarray
    qbegin: np.ndarray
    qend: np.ndarray
    align_len: np.ndarray
    matches: np.ndarray
    gaps: np.ndarray
    gap_regions: np.ndarray
    ops_off: np.ndarray
    ops_len: np.ndarray
    ops: np.ndarray

    @staticmethod
    def from_c(res: "L.Results", n: int) -> "BatchResult":
        def arr(ptr, dt, cnt):
            if cnt == 0:
                return np.zeros(0, dtype=dt)
            return np.ctypeslib.as_array(ptr, shape=(cnt,)).astype(dt, copy=True)
        return BatchResult(arr(res.status, np.int32, n), arr(res.score, np.uint32, n), arr(res.tbegin, np.int32, n),
                           arr(res.tend, np.int32, n), arr(res.qbegin, np.int32, n), arr(res.qend, np.int32, n),
                           arr(res.align_len, np.uint32, n), arr(res.matches, np.uint32, n),
                           arr(res.gaps, np.uint32, n), arr(res.gap_regions, np.uint32, n),
                           arr(res.ops_off, np.uint64, n), arr(res.ops_len, np.uint32, n),
                           arr(res.ops, np.uint64, int(res.n_ops)))

    def pair_ops(self, i: int) -> np.ndarray:
        return self.ops[int(self.ops_off[i]):int(self.ops_off[i]) + int(self.ops_len[i])]

    def result(self, i: int) -> AlignmentResult:
        return AlignmentResult(Ops=[int(o) for o in self.pair_ops(i)], Score=int(self.score[i]),
                               TBegin=int(self.tbegin[i]), TEnd=int(self.tend[i]), QBegin=int(self.qbegin[i]),
                               QEnd=int(self.qend[i]), AlignLen=int(self.align_len[i]),
                               Matches=int(self.matches[i]), Gaps=int(self.gaps[i]),
                               GapRegions=int(self.gap_regions[i]))


def New(p: Penalties = DefaultPenalties, opt: Options = DefaultOptions, device: int = -1) -> Aligner:
    """wfa.go:120."""
    return Aligner(p, opt, device)


def RecycleAligner(algn: Optional[Aligner]) -> None:
    """wfa.go:102: returns the aligner to the pool; here it releases the device context."""
    if algn is not None:
        algn.close()


def generate_pairs(seed: int, n_pairs: int, length: int, error_rate: float, first_index: int = 0,
                   n_threads: int = 8):
    """Seeded synthetic dataset (include/wfa_hip.h: wfahip_generate_pairs).  Host only, no GPU needed."""
    stride = int(L.lib().wfahip_gen_stride(length, error_rate))
    blob = np.zeros(max(n_pairs * stride, 1) + 16, dtype=np.uint8)
    q_off = np.zeros(n_pairs, dtype=np.uint64)
    t_off = np.zeros(n_pairs, dtype=np.uint64)
    q_len = np.zeros(n_pairs, dtype=np.uint32)
    t_len = np.zeros(n_pairs, dtype=np.uint32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    if n_pairs:
        L.check(L.lib().wfahip_generate_pairs(seed, first_index, n_pairs, length, float(error_rate), n_threads,
                                              vp(blob), vp(q_off), vp(q_len), vp(t_off), vp(t_len)),
                "wfahip_generate_pairs")
    return blob, q_off, q_len, t_off, t_len


def generate_pairs_device(ctx_owner: "Aligner", seed: int, n_pairs: int, length: int, error_rate: float, first_index: int = 0):
    """The same dataset generated on the aligner's GPU (include/wfa_hip.h: wfahip_generate_pairs_device): returns torch
    tensors (blob u8, q_off i64, q_len i32, t_off i64, t_len i32) resident in HBM; nothing crosses PCIe.  (The buffers
    are torch's: torch.cuda must have been initialised before the first aligner of the process was created -- torch
    ships its own HIP runtime, and it does not find the GPUs once the library's runtime has come up first.)"""
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    stride = int(L.lib().wfahip_gen_stride(length, error_rate))
    blob = torch.zeros(max(n_pairs * stride, 1) + 16, dtype=torch.uint8, device=dev)
    q_off = torch.zeros(n_pairs, dtype=torch.int64, device=dev)
    t_off = torch.zeros(n_pairs, dtype=torch.int64, device=dev)
    q_len = torch.zeros(n_pairs, dtype=torch.int32, device=dev)
    t_len = torch.zeros(n_pairs, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)  # (the fills run on torch's stream, the generator on the library's: not ordered otherwise)
    L.check(L.lib().wfahip_generate_pairs_device(ctx_owner._ctx, seed, first_index, n_pairs, length, float(error_rate),
                                                 blob.data_ptr(), q_off.data_ptr(), q_len.data_ptr(), t_off.data_ptr(),
                                                 t_len.data_ptr(), None), "wfahip_generate_pairs_device")
    return blob, q_off, q_len, t_off, t_len
