"""CPU: the interface of dev plans for batches with large units (MSCOMP_AMD_DEV_LARGE_UNITS): mscomp_amd_plan_create_decompress_dev_ex,
mscomp_amd_plan_create_size_dev_ex and the test hook mscomp_amd_debug_plan_paths are declared, exported and bound; the argument checks of
the two creators, which need no GPU."""
import ctypes as C
import re

import abi_rig as R

NAMES = ("mscomp_amd_plan_create_decompress_dev_ex", "mscomp_amd_plan_create_size_dev_ex", "mscomp_amd_debug_plan_paths")


def test_the_three_names_are_declared_exported_and_bound():
    import ms_compress_amd as m
    lib = m.load_library()
    R.check_declared(lib, NAMES)
    assert re.search(r"#define\s+MSCOMP_AMD_DEV_LARGE_UNITS\s+1u\b", R.flat_header())
    assert m.api.MSCOMP_AMD_DEV_LARGE_UNITS == 1


def test_creators_check_their_arguments_like_the_plain_dev_creators():
    """without a context nothing can be created: every call below is refused before the GPU is touched, and the _ex creators answer what the
    creators without _ex answer"""
    import ms_compress_amd as m
    lib = m.load_library()
    ARG = m.MSCOMP_ARG_ERROR
    fake_ctx = C.c_void_p(0)
    for flags in (0, 1):
        plan = C.c_void_p(123)
        assert lib.mscomp_amd_plan_create_decompress_dev_ex(fake_ctx, 3, 4, 1 << 20, 1 << 20, flags, C.byref(plan)) == ARG   # null ctx
        assert plan.value is None                                    # (the plan pointer is cleared, as by the plain creator)
        assert lib.mscomp_amd_plan_create_decompress_dev(fake_ctx, 3, 4, 1 << 20, 1 << 20, C.byref(plan)) == ARG
        assert lib.mscomp_amd_plan_create_decompress_dev_ex(fake_ctx, 3, 4, 1 << 20, 1 << 20, flags, None) == ARG           # null plan pointer
        plan = C.c_void_p(123)
        assert lib.mscomp_amd_plan_create_size_dev_ex(fake_ctx, 3, 4, 1 << 20, flags, C.byref(plan)) == ARG and plan.value is None
        assert lib.mscomp_amd_plan_create_size_dev(fake_ctx, 3, 4, 1 << 20, C.byref(plan)) == ARG
        assert lib.mscomp_amd_plan_create_size_dev_ex(fake_ctx, 3, 4, 1 << 20, flags, None) == ARG
    # a context that is never dereferenced: these checks come before the context is used
    bogus = C.c_void_p(0x1000)
    plan = C.c_void_p()
    for fmt in (0, 1, 5, 77):                                        # bad format
        assert lib.mscomp_amd_plan_create_decompress_dev_ex(bogus, fmt, 4, 64, 64, 1, C.byref(plan)) == ARG
        assert lib.mscomp_amd_plan_create_size_dev_ex(bogus, fmt, 4, 64, 1, C.byref(plan)) == ARG
    for fmt in (2, 3, 4):
        assert lib.mscomp_amd_plan_create_decompress_dev_ex(bogus, fmt, 0x7FFFFFF1, 64, 64, 1, C.byref(plan)) == ARG        # n_units above 0x7FFFFFF0
        assert lib.mscomp_amd_plan_create_size_dev_ex(bogus, fmt, 0x7FFFFFF1, 64, 1, C.byref(plan)) == ARG
        for flags in (2, 3, 0x80000000, 0xFFFFFFFE):                # a bit other than MSCOMP_AMD_DEV_LARGE_UNITS
            assert lib.mscomp_amd_plan_create_decompress_dev_ex(bogus, fmt, 4, 64, 64, flags, C.byref(plan)) == ARG, (fmt, flags)
            assert lib.mscomp_amd_plan_create_size_dev_ex(bogus, fmt, 4, 64, flags, C.byref(plan)) == ARG, (fmt, flags)
    assert plan.value is None
    out = (C.c_uint32 * 3)()
    assert lib.mscomp_amd_debug_plan_paths(None, out) == -1 and lib.mscomp_amd_debug_plan_paths(None, None) == -1
