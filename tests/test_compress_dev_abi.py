"""CPU: compress plans with device tables (mscomp_amd_plan_create_compress_dev) and mscomp_amd_plan_layout_dev are exported, declared in
the header and named in api.EXPORTS, and refuse bad arguments before they touch a device."""
import ctypes as C

import abi_rig as R

NAMES = ("mscomp_amd_plan_create_compress_dev", "mscomp_amd_plan_layout_dev")


def test_compress_dev_symbols_are_exported_and_declared():
    import ms_compress_amd as m
    lib = m.load_library()
    R.check_declared(lib, NAMES)
    assert m.CompressDevPlan is not None and callable(m.plan_layout_dev)


def test_compress_dev_argument_errors_without_gpu():
    import ms_compress_amd as m
    lib = m.load_library()
    create = lib.mscomp_amd_plan_create_compress_dev
    plan = C.c_void_p(123)
    for f in (2, 3, 4):                                           # a null context
        assert create(None, f, 4, 1 << 20, 65536, C.byref(plan)) == m.MSCOMP_ARG_ERROR
        assert not plan.value                                     # the plan pointer is cleared on failure
        plan = C.c_void_p(123)
    for bad in (0, 1, 5, 99):                                     # a bad format (checked before the context is used)
        assert create(C.c_void_p(8), bad, 4, 1 << 20, 65536, C.byref(plan)) == m.MSCOMP_ARG_ERROR
        assert not plan.value
        plan = C.c_void_p(123)
    for unit_max in (0, 0xFFFFF001):                              # in_unit_max out of range
        assert create(C.c_void_p(8), 2, 4, 1 << 20, unit_max, C.byref(plan)) == m.MSCOMP_ARG_ERROR
        assert not plan.value
        plan = C.c_void_p(123)
    assert create(C.c_void_p(8), 2, 0x7FFFFFF1, 1 << 20, 65536, C.byref(plan)) == m.MSCOMP_ARG_ERROR   # too many units
    assert not plan.value
    assert create(None, 2, 4, 1 << 20, 65536, None) == m.MSCOMP_ARG_ERROR   # a null plan pointer
    assert create(C.c_void_p(8), 2, 4, 1 << 20, 65536, None) == m.MSCOMP_ARG_ERROR
    for f in (2, 3, 4):
        assert lib.mscomp_amd_plan_layout_dev(None, f, 4, None, 16, None, None) == m.MSCOMP_ARG_ERROR
