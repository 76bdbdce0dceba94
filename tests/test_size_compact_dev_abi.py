"""CPU: size plans with device tables (mscomp_amd_plan_create_size_dev / mscomp_amd_plan_execute_size_dev) and mscomp_amd_compact_dev are
exported, declared in the header and named in api.EXPORTS, and refuse bad arguments before they touch a device."""
import ctypes as C

import abi_rig as R

NAMES = ("mscomp_amd_plan_create_size_dev", "mscomp_amd_plan_execute_size_dev", "mscomp_amd_compact_dev")
FAKE = C.c_void_p(8)                                              # a non-null pointer that must never be followed


def test_size_compact_dev_symbols_are_exported_and_declared():
    import ms_compress_amd as m
    lib = m.load_library()
    R.check_declared(lib, NAMES)
    for s in NAMES:
        assert getattr(lib, s).argtypes is not None and getattr(lib, s).restype is C.c_int, s
    assert m.SizeDevPlan is not None and callable(m.compact_dev)
    assert m.SizeDevPlan.execute is not m.DevPlan.execute


def test_size_dev_create_argument_errors_without_gpu():
    import ms_compress_amd as m
    create = m.load_library().mscomp_amd_plan_create_size_dev
    plan = C.c_void_p(123)
    for f in (2, 3, 4):                                           # a null context
        assert create(None, f, 4, 1 << 20, C.byref(plan)) == m.MSCOMP_ARG_ERROR
        assert not plan.value                                     # the plan pointer is cleared on failure
        plan = C.c_void_p(123)
    for bad in (0, 1, 5, 99):                                     # a bad format (checked before the context is used)
        assert create(FAKE, bad, 4, 1 << 20, C.byref(plan)) == m.MSCOMP_ARG_ERROR
        assert not plan.value
        plan = C.c_void_p(123)
    for f in (2, 3, 4):                                           # too many units
        assert create(FAKE, f, 0x7FFFFFF1, 1 << 20, C.byref(plan)) == m.MSCOMP_ARG_ERROR
        assert not plan.value
        plan = C.c_void_p(123)
    assert create(None, 2, 4, 1 << 20, None) == m.MSCOMP_ARG_ERROR   # a null plan pointer
    assert create(FAKE, 2, 4, 1 << 20, None) == m.MSCOMP_ARG_ERROR


def test_size_dev_bounds_beyond_the_scratch_without_gpu():
    """LZNT1 segments and Xpress+Huffman tiles / candidates are counted in 32 bits: bounds that need more are MSCOMP_MEM_ERROR, found before
    the context is used"""
    import ms_compress_amd as m
    create = m.load_library().mscomp_amd_plan_create_size_dev
    for f, total in ((2, 49152 << 31), (4, 16384 << 31), (4, 260 << 31)):
        plan = C.c_void_p(123)
        assert create(FAKE, f, 1 << 20, total, C.byref(plan)) == m.MSCOMP_MEM_ERROR, (f, total)
        assert not plan.value


def test_size_dev_execute_and_compact_dev_argument_errors_without_gpu():
    import ms_compress_amd as m
    lib = m.load_library()
    assert lib.mscomp_amd_plan_execute_size_dev(None, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE) == m.MSCOMP_ARG_ERROR   # a null plan
    compact = lib.mscomp_amd_compact_dev
    assert compact(None, 4, FAKE, FAKE, FAKE, 1, FAKE, 1 << 20, FAKE) == m.MSCOMP_ARG_ERROR      # a null context
    assert compact(None, 0, None, None, None, 1, None, 0, FAKE) == m.MSCOMP_ARG_ERROR
    assert compact(FAKE, 4, FAKE, FAKE, FAKE, 1, FAKE, 1 << 20, None) == m.MSCOMP_ARG_ERROR      # null offsets to write
    assert compact(FAKE, 0, None, None, None, 1, None, 0, None) == m.MSCOMP_ARG_ERROR
    for hole in range(4):                                         # a null array with n_units > 0
        a = [FAKE, FAKE, FAKE, FAKE]
        a[hole] = None
        assert compact(FAKE, 4, a[0], a[1], a[2], 16, a[3], 1 << 20, FAKE) == m.MSCOMP_ARG_ERROR, hole
    assert compact(FAKE, 0x7FFFFFF1, FAKE, FAKE, FAKE, 1, FAKE, 1 << 20, FAKE) == m.MSCOMP_ARG_ERROR   # too many units
