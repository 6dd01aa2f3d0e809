"""CPU: the length-class table of the semi-global router and the debug entry of its plan kernels (include/wfa_hip.h:
wfahip_wide_class_bounds, wfahip_debug_wide_plan) are declared, exported, bound, and validate their arguments before they touch
a device."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("wfahip_wide_class_bounds", "wfahip_debug_wide_plan")


def test_entries_declared_exported_and_resolvable(built):
    from wfa_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "wfa_hip.h")).read(), flags=re.S)
    flat = " ".join(hdr.split())
    declared = set(re.findall(r"\b(wfahip_[a-z_]+)\s*\(", hdr))
    for name in NAMES:
        assert name in declared and name in _lib.EXPORTS
        assert getattr(_lib.lib(), name) is not None
    assert "int wfahip_wide_class_bounds(uint32_t *bounds, int cap);" in flat
    assert ("int wfahip_debug_wide_plan(wfahip_ctx *ctx, const uint32_t *q_len, const uint32_t *t_len, uint64_t n_pairs, "
            "uint32_t **ids, uint64_t *counts, uint32_t *longest, uint64_t *n_ladder);") in flat
    u32, u64 = C.c_uint32, C.c_uint64
    assert _lib.lib().wfahip_debug_wide_plan.argtypes == [C.c_void_p, C.c_void_p, C.c_void_p, u64, C.POINTER(C.POINTER(u32)),
                                                          C.POINTER(u64), C.POINTER(u32), C.POINTER(u64)]
    import wfa_amd
    assert callable(wfa_amd.Aligner.debug_wide_plan) and callable(wfa_amd.wide_class_bounds)


def test_class_bounds(built):
    import wfa_amd
    from wfa_amd import _lib
    L = _lib.lib()
    n = L.wfahip_wide_class_bounds(None, 0)
    assert 2 <= n <= 6
    full = (C.c_uint32 * n)()
    assert L.wfahip_wide_class_bounds(full, n) == n
    bounds = [int(x) for x in full]
    assert all(a < b for a, b in zip(bounds, bounds[1:])) and bounds[0] >= 1 and bounds[-1] == 2047
    assert wfa_amd.wide_class_bounds() == bounds
    # a buffer that is too small: the count comes back, the buffer's entries are filled, nothing beyond them is written
    short = (C.c_uint32 * n)(*([0xDEAD] * n))
    assert L.wfahip_wide_class_bounds(short, n - 1) == n
    assert [int(x) for x in short] == bounds[:n - 1] + [0xDEAD]
    big = (C.c_uint32 * (n + 2))(*([0xDEAD] * (n + 2)))
    assert L.wfahip_wide_class_bounds(big, n + 2) == n
    assert [int(x) for x in big] == bounds + [0xDEAD] * 2


def test_debug_wide_plan_bad_args_without_device(built):
    from wfa_amd import _lib
    L = _lib.lib()
    ctx = C.c_void_p(1)  # (a dummy context: it must not be touched)
    lens = (C.c_uint32 * 4)(10, 20, 30, 40)
    ids, counts, longest, n_ladder = C.POINTER(C.c_uint32)(), (C.c_uint64 * 6)(), (C.c_uint32 * 6)(), C.c_uint64()
    good = [ctx, lens, lens, 4, C.byref(ids), counts, longest, C.byref(n_ladder)]
    for hole in (0, 1, 2, 4, 5, 6, 7):  # the context, each length array, each output in turn
        args = list(good)
        args[hole] = None
        assert L.wfahip_debug_wide_plan(*args) == _lib.ERR_BAD_ARG, hole
