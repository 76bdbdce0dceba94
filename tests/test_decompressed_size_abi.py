"""CPU: the decompressed-size query (mscomp_amd_plan_create_size / _execute_size / mscomp_amd_decompressed_size_batch) is exported,
declared in the header and named in api.EXPORTS, and refuses bad arguments before it touches a device."""
import ctypes as C

import numpy as np

import abi_rig as R

NAMES = ("mscomp_amd_plan_create_size", "mscomp_amd_plan_execute_size", "mscomp_amd_decompressed_size_batch")


def test_size_query_is_exported_and_declared():
    import ms_compress_amd as m
    lib = m.load_library()
    R.check_declared(lib, NAMES)
    assert callable(m.decompressed_sizes) and callable(m.decompress_units_auto) and m.SizePlan is not None


def test_size_query_argument_errors_without_gpu():
    import ms_compress_amd as m
    lib = m.load_library()
    off = np.zeros(2, np.uint64)
    ln = np.array([10, 20], np.uint64)
    lim = np.array([100, 100], np.uint64)
    plan = C.c_void_p(123)
    for f in (2, 3, 4):
        assert lib.mscomp_amd_plan_create_size(None, f, 2, off.ctypes.data, ln.ctypes.data, lim.ctypes.data, C.byref(plan)) == m.MSCOMP_ARG_ERROR
        assert not plan.value                                    # the plan pointer is cleared on failure
        plan = C.c_void_p(123)
        assert lib.mscomp_amd_plan_create_size(None, f, 2, off.ctypes.data, ln.ctypes.data, None, C.byref(plan)) == m.MSCOMP_ARG_ERROR
    for bad in (0, 1, 5, 99):
        assert lib.mscomp_amd_plan_create_size(None, bad, 2, off.ctypes.data, ln.ctypes.data, None, C.byref(plan)) == m.MSCOMP_ARG_ERROR
    assert lib.mscomp_amd_plan_create_size(None, 2, 2, off.ctypes.data, ln.ctypes.data, None, None) == m.MSCOMP_ARG_ERROR
    assert lib.mscomp_amd_plan_execute_size(None, None, None, None, None) == m.MSCOMP_ARG_ERROR
    assert lib.mscomp_amd_decompressed_size_batch(None, 2, 2, None, off.ctypes.data, ln.ctypes.data, None, None, None, None) == m.MSCOMP_ARG_ERROR
    assert lib.mscomp_amd_decompressed_size_batch(None, 7, 2, None, off.ctypes.data, ln.ctypes.data, None, None, None, None) == m.MSCOMP_ARG_ERROR
