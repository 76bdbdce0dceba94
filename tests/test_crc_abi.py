"""CPU: the CRC calls (mscomp_amd_plan_*_crc_dev, mscomp_amd_blocks_crc / _check) are exported, declared and named in api.EXPORTS, refuse bad
arguments before they touch a device, and tests/crc_model.py holds against the known answers."""
import ctypes as C
import zlib

import numpy as np

import abi_rig as R
import blocks_model as M
import crc_model as K

NAMES = ("mscomp_amd_plan_create_crc_dev", "mscomp_amd_plan_execute_crc_dev", "mscomp_amd_blocks_crc", "mscomp_amd_blocks_check")


def test_crc_symbols_are_exported_and_declared():
    import ms_compress_amd as m
    lib = m.load_library()
    R.check_declared(lib, NAMES)
    for s in ("CrcDevPlan", "crc32_units", "blocks_crc"):
        assert getattr(m, s) is not None, s
    assert callable(m.BlockContainer.crc) and callable(m.BlockContainer.check)
    row, slc = K.kernel_sizes()
    assert row == 4096 and slc % row == 0


def test_crc_argument_errors_without_gpu():
    import ms_compress_amd as m
    lib = m.load_library()
    create = lib.mscomp_amd_plan_create_crc_dev
    ctx = C.c_void_p(8)                                           # never dereferenced: every check below comes before the context is used
    plan = C.c_void_p(123)
    assert create(None, 4, 1 << 20, C.byref(plan)) == m.MSCOMP_ARG_ERROR and not plan.value     # a null context; the pointer is cleared
    plan = C.c_void_p(123)
    assert create(ctx, 0x7FFFFFF1, 1 << 20, C.byref(plan)) == m.MSCOMP_ARG_ERROR and not plan.value
    plan = C.c_void_p(123)
    assert create(ctx, 4, 1 << 50, C.byref(plan)) == m.MSCOMP_ARG_ERROR and not plan.value      # distances stay below 2^50
    assert create(ctx, 4, 1 << 20, None) == m.MSCOMP_ARG_ERROR and create(None, 4, 1 << 20, None) == m.MSCOMP_ARG_ERROR
    p = C.c_void_p(8)
    # no plan: every execute call refuses it, the CRC one included (a plan of another kind needs a device to exist)
    assert lib.mscomp_amd_plan_execute_crc_dev(None, p, p, p, p, p) == m.MSCOMP_ARG_ERROR
    assert lib.mscomp_amd_plan_execute_dev(None, p, p, p, p, p, p, p, p) == m.MSCOMP_ARG_ERROR
    # a null container, with every array given
    assert lib.mscomp_amd_blocks_crc(None, p, p, p, p, p, p) == m.MSCOMP_ARG_ERROR
    assert lib.mscomp_amd_blocks_check(None, p, p, p, p, None, p, p, p) == m.MSCOMP_ARG_ERROR


def test_crc_model_known_answers():
    assert K.crc(b"") == 0 and K.crc(b"123456789") == 0xCBF43926
    mem = np.frombuffer(b"xx123456789yy", dtype=np.uint8)
    c, st = K.units(mem, [2, 0, 2], [9, 0, 9], 10)
    assert c.tolist() == [0xCBF43926, 0, 0] and st.tolist() == [0, 0, M.ARG]
    bufs = [b"123456789" * 1000, b"", np.random.RandomState(3).bytes(4096 * 2 + 5)]
    B = 4096
    bc, rc, st = K.blocks(bufs, B, sum(len(b) for b in bufs))
    assert len(bc) == 3 + (9000 + 8197) // B and st.tolist() == [0, 0, 0]
    joined = [b"".join(b[at: at + B] for at in range(0, len(b), B)) for b in bufs]
    assert [int(x) for x in rc] == [zlib.crc32(j) for j in joined]
    assert int(bc[0]) == zlib.crc32(bufs[0][:B]) and int(bc[2]) == zlib.crc32(bufs[0][2 * B:]) and int(bc[3]) == zlib.crc32(bufs[2][:B])
    assert not bc[6:].any()
    # a rejected resource has no blocks and a CRC of 0
    bc2, rc2, st2 = K.blocks(bufs, B, 9000)
    assert st2.tolist() == [0, 0, M.ARG] and int(rc2[2]) == 0 and not bc2[3:].any()
    # check: a wrong block CRC fails its resource alone; a resource that is not OK on entry is left alone
    out = np.frombuffer(b"".join(bufs), dtype=np.uint8)
    off, first = [0, 9000, 9000], [0, 3, 3, 6]
    assert K.check(out, off, [9000, 0, 8197], first, bc, [0, 0, 0], [9000, 0, 8197], B, 17197) == ([0, 0, 0], [9000, 0, 8197])
    bad = bc.copy(); bad[4] ^= 1
    assert K.check(out, off, [9000, 0, 8197], first, bad, [0, 0, 0], [9000, 0, 8197], B, 17197) == ([0, 0, M.DATA], [9000, 0, 0])
    assert K.check(out, off, [9000, 0, 8197], first, bad, [0, 0, M.BUF], [9000, 0, 7], B, 17197) == ([0, 0, M.BUF], [9000, 0, 7])
    assert K.check(out, off, [9000, 0, 8197], first, bad, [0, 0, 0], [9000, 0, 8197], B, 17197, ranges=[(0, 9), (0, 0), (0, 1)])[0] == [0, 0, 0]
