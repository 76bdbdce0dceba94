"""The device's v_alignbyte_b32 takes its byte shift from bits [1:0] of the third operand and ignores the rest: csrc/lznt1.hip hands it a byte
address (common.h alignbyte_addr) instead of masking the address first. The library's self-check (csrc/util.hip alignbyte_check_kernel) runs the
instruction for every low byte 0..255 under sixteen settings of the bits above it (none, all, fourteen patterns), four dword pairs, with the
operand in a vector register and in a scalar one, and compares with {hi, lo} >> 8 (operand & 3) computed on the host. A device that behaves
otherwise fails here, before any compare of the encoder goes wrong."""
import pytest

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", [1, 0xFFFFFFFF, 0x5EED1234])
def test_alignbyte_reads_the_low_two_bits_of_its_shift(gpu_ctx, seed):
    bad = gpu_ctx.lib.mscomp_amd_debug_alignbyte(gpu_ctx._h, seed)
    assert bad != 0xFFFFFFFF, "the check could not run"
    assert bad == 0, "%d of %d results differ from {hi, lo} >> 8 (shift & 3)" % (bad, 256 * 128)
