"""CPU: mscomp_amd_writer_resize and mscomp_amd_res_crc_dev are exported, declared in the header and named in api.EXPORTS, and refuse bad
arguments before they touch a device -- in the manner of tests/test_writer_abi.py. The creators still take no flags."""
import ctypes as C

import abi_rig as R

NAMES = ("mscomp_amd_writer_resize", "mscomp_amd_res_crc_dev")


def test_resize_symbols_are_exported_and_declared():
    import ms_compress_amd as m
    lib = m.load_library()
    R.check_declared(lib, NAMES)
    assert callable(m.BlockWriter.resize) and callable(m.blocks_resize) and callable(m.res_crc_from_blocks) and callable(m.res_crc_dev)


def test_resize_null_object():
    import ms_compress_amd as m
    lib = m.load_library()
    p = C.c_void_p(8)                                             # never dereferenced: the writer is null
    assert lib.mscomp_amd_writer_resize(None, p, 16, p, p, p, None, p, p, 16, p, p, None, p, p) == m.MSCOMP_ARG_ERROR
    assert lib.mscomp_amd_writer_resize(None, p, 16, p, p, p, p, p, p, 16, p, p, p, p, p) == m.MSCOMP_ARG_ERROR
    assert lib.mscomp_amd_writer_resize(None, None, 0, None, None, None, None, None, None, 0, None, None, None, None, None) == m.MSCOMP_ARG_ERROR


def test_res_crc_argument_errors_without_gpu():
    import ms_compress_amd as m
    lib = m.load_library()
    call = lib.mscomp_amd_res_crc_dev
    ctx, p = C.c_void_p(8), C.c_void_p(8)                         # never dereferenced: every check below comes before the context is used
    assert call(None, 4096, 4, 64, p, p, p, p, p) == m.MSCOMP_ARG_ERROR             # a null context
    assert call(None, 4096, 0, 0, None, None, None, None, None) == m.MSCOMP_ARG_ERROR
    for bs in (0, 4095, 6144, 2048, 1048576, 0x80000000):         # block_size: a power of two from 4096 to 524288
        assert call(ctx, bs, 4, 64, p, p, p, p, p) == m.MSCOMP_ARG_ERROR
    big = 0x7FFFFFF1
    assert call(ctx, 4096, big, 64, p, p, p, p, p) == m.MSCOMP_ARG_ERROR            # both counts
    assert call(ctx, 4096, 4, big, p, p, p, p, p) == m.MSCOMP_ARG_ERROR
    assert call(ctx, 4096, 4, 1 << 40, p, p, p, p, p) == m.MSCOMP_ARG_ERROR
    for hole in range(5):                                         # each of the five arrays is needed when there are resources
        args = [p] * 5
        args[hole] = None
        assert call(ctx, 65536, 4, 64, *args) == m.MSCOMP_ARG_ERROR
    assert call(ctx, 524288, 0, 64, None, None, None, None, None) == m.MSCOMP_OK    # no resources: nothing to report on, nothing used


def test_creators_still_take_no_flags():
    import ms_compress_amd as m
    lib = m.load_library()
    ctx = C.c_void_p(8)
    for create in (lib.mscomp_amd_reader_create, lib.mscomp_amd_writer_create):
        obj = C.c_void_p(123)
        assert create(ctx, 3, 65536, 4, 64, 8, 16, 1, C.byref(obj)) == m.MSCOMP_ARG_ERROR and not obj.value
    obj = C.c_void_p(123)
    assert lib.mscomp_amd_blocks_create(ctx, 3, 65536, 4, 1 << 20, 1, C.byref(obj)) == m.MSCOMP_ARG_ERROR and not obj.value
