"""CPU: the two symbols of splice by extents are exported, declared in the header and named in api.EXPORTS, and refuse bad arguments before
they touch a device -- in the manner of tests/test_splice_abi.py."""
import ctypes as C

import pytest

import abi_rig as R

NAMES = ("mscomp_amd_splicer_create_extents", "mscomp_amd_splicer_splice_extents")


def test_extents_symbols_are_exported_and_declared():
    import ms_compress_amd as m
    lib = m.load_library()
    hdr = R.check_declared(lib, NAMES)
    assert "#define MSCOMP_AMD_SPLICE_ROW_TILE %du" % m.MSCOMP_AMD_SPLICE_ROW_TILE in hdr
    assert callable(m.BlockSplicer.for_extents) and callable(m.BlockSplicer.splice_extents)
    assert all(callable(f) for f in (m.blocks_splice_extents, m.blocks_concat, m.blocks_split_at, m.blocks_cut_range))


def test_create_extents_argument_errors_without_gpu():
    import ms_compress_amd as m
    lib = m.load_library()
    create = lib.mscomp_amd_splicer_create_extents
    ctx = C.c_void_p(8)                                           # never dereferenced: every check below comes before the context is used

    def refused(*args):
        obj = C.c_void_p(123)
        return create(*args, C.byref(obj)) == m.MSCOMP_ARG_ERROR and not obj.value
    assert refused(None, 4096, 1, 4, 8, 64, 0)                    # a null context
    assert create(ctx, 4096, 1, 4, 8, 64, 0, None) == m.MSCOMP_ARG_ERROR            # a null out pointer
    for bs in (0, 4095, 6144, 2048, 1048576, 0x80000000):         # block_size: a power of two from 4096 to 524288
        assert refused(ctx, bs, 1, 4, 8, 64, 0), bs
    for n_src in (0, 5, 0xFFFFFFFF):                              # 1 .. MSCOMP_AMD_SPLICE_SRC_MAX sources
        assert refused(ctx, 4096, n_src, 4, 8, 64, 0), n_src
    assert refused(ctx, 65536, 2, 4, 8, 64, 1)                    # no flags
    big = 0x7FFFFFF1                                              # n_res, n_ext and n_blocks_table: the bound of n_pick, each
    assert refused(ctx, 4096, 4, big, 8, 64, 0) and refused(ctx, 4096, 4, 4, big, 64, 0) and refused(ctx, 4096, 4, 4, 8, big, 0)
    assert refused(ctx, 524288, 1, 4, 1 << 40, 64, 0) and refused(ctx, 524288, 1, 1 << 40, 8, 64, 0)


def test_splice_extents_null_object():
    import ms_compress_amd as m
    lib = m.load_library()
    p = C.c_void_p(8)                                             # never dereferenced: the splicer is null
    views = (m.BlocksView * 1)()
    assert lib.mscomp_amd_splicer_splice_extents(None, views, p, p, p, 16, p, p, p, p, p) == m.MSCOMP_ARG_ERROR
    assert lib.mscomp_amd_splicer_splice_extents(None, views, p, p, p, 16, p, p, None, p, p) == m.MSCOMP_ARG_ERROR
    assert lib.mscomp_amd_splicer_splice_extents(None, None, None, None, None, 0, None, None, None, None, None) == m.MSCOMP_ARG_ERROR


@pytest.mark.gpu
def test_a_splicer_made_for_picks_refuses_extents(gpu_ctx):
    """(needs a device: a splicer cannot be created without one) MSCOMP_ARG_ERROR on the host, nothing launched, nothing written"""
    import torch
    import ms_compress_amd as m
    dev = torch.device("cuda", gpu_ctx.device)
    sp = m.BlockSplicer(gpu_ctx, 4096, 1, 2, 8)
    z = lambda k, dt=torch.int64: torch.full((k,), 77, dtype=dt, device=dev)
    src = (z(64, torch.uint8), torch.zeros(2, dtype=torch.int64, device=dev), torch.zeros(2, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.int64, device=dev), None, 0, 1, 1)
    outs = [z(64, torch.uint8), z(3), z(9), z(2), z(2, torch.int32)]
    with pytest.raises(m.MSCompError) as e:
        sp.splice_extents([src], torch.zeros(3, dtype=torch.int64, device=dev), torch.zeros(8, dtype=torch.int64, device=dev), *outs)
    assert e.value.status == m.MSCOMP_ARG_ERROR
    sp.close()
    torch.cuda.synchronize()
    assert all(bool((t == 77).all()) for t in outs)
