"""CPU: decompress plans with device tables (mscomp_amd_plan_create_decompress_dev / _execute_dev) and mscomp_amd_layout_dev are exported,
declared in the header and named in api.EXPORTS, and refuse bad arguments before they touch a device."""
import ctypes as C

import abi_rig as R

NAMES = ("mscomp_amd_plan_create_decompress_dev", "mscomp_amd_plan_execute_dev", "mscomp_amd_layout_dev")


def test_dev_plan_symbols_are_exported_and_declared():
    import ms_compress_amd as m
    lib = m.load_library()
    R.check_declared(lib, NAMES)
    assert m.DevPlan is not None and callable(m.layout_dev)


def test_dev_plan_argument_errors_without_gpu():
    import ms_compress_amd as m
    lib = m.load_library()
    plan = C.c_void_p(123)
    for f in (2, 3, 4):                                           # a null context
        assert lib.mscomp_amd_plan_create_decompress_dev(None, f, 4, 1 << 20, 1 << 20, C.byref(plan)) == m.MSCOMP_ARG_ERROR
        assert not plan.value                                     # the plan pointer is cleared on failure
        plan = C.c_void_p(123)
    for bad in (0, 1, 5, 99):                                     # a bad format (checked before the context is used)
        assert lib.mscomp_amd_plan_create_decompress_dev(C.c_void_p(8), bad, 4, 1 << 20, 1 << 20, C.byref(plan)) == m.MSCOMP_ARG_ERROR
        assert not plan.value
        plan = C.c_void_p(123)
    assert lib.mscomp_amd_plan_create_decompress_dev(None, 2, 4, 1 << 20, 1 << 20, None) == m.MSCOMP_ARG_ERROR   # a null plan pointer
    assert lib.mscomp_amd_plan_create_decompress_dev(C.c_void_p(8), 2, 4, 1 << 20, 1 << 20, None) == m.MSCOMP_ARG_ERROR
    assert lib.mscomp_amd_plan_execute_dev(None, None, None, None, None, None, None, None, None) == m.MSCOMP_ARG_ERROR
    assert lib.mscomp_amd_layout_dev(None, 4, None, 16, None) == m.MSCOMP_ARG_ERROR
