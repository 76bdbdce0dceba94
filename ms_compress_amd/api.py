"""Host-side binding of libmscomp_amd.so (the C-ABI declared in include/mscomp_amd.h): the one module callers import. It defines nothing;
every name lives in the module of its concern --

  _abi.py         the constants, SIGNATURES, the ctypes structures, load_library
  _core.py        Context, _Handle, _run, the one-shot host calls, the frame and the upload helpers of the host conveniences
  plans.py        the plan classes and *_dev calls, their host conveniences, the host-batch entry, the plan and scratch hooks
  blocks.py       the block objects, as thin wrappers over device tensors
  blocks_host.py  the blocks_* host conveniences
  device.py       DeviceBlocks and BlockOps: containers that stay in device memory from call to call

Mirrors the reference's own ctypes fixture (/root/reference/test/compressors.py:187-251: ``OpenSrc.Compress`` ->
``ms_compress``; default output buffer, status codes) so that the parity tests read like the reference's tests,
and adds the batch interface (device-resident units) the GPU path needs.

PyTorch is plumbing only: device memory (``torch.empty(..., device="cuda")``), the current HIP stream and
``torch.distributed``. There is NO CPU encoder behind these functions: if the HIP extension is missing or no
GPU is visible they raise.

The loader's state (``_lib``) is _abi's alone: a copy here would go stale, so a test that stands in for the library patches _abi.
"""
from . import _abi, _core, blocks, blocks_host, device, plans  # noqa: F401
from ._abi import (HERE, LIB_PATH, MSCOMP_NONE, MSCOMP_RESERVED, MSCOMP_LZNT1, MSCOMP_XPRESS, MSCOMP_XPRESS_HUFF, MSCOMP_OK, MSCOMP_ERRNO,  # noqa: F401
                   MSCOMP_ARG_ERROR, MSCOMP_DATA_ERROR, MSCOMP_MEM_ERROR, MSCOMP_BUF_ERROR, FORMATS, CHUNK, SIGNATURES, EXPORTS,
                   MSCOMP_AMD_SPLICE_SRC_MAX, MSCOMP_AMD_SPLICE_ROW_TILE, MSCOMP_AMD_SYNC_TILE, MSCOMP_AMD_DIGEST_LEAF, MSCOMP_AMD_PARITY_K_MAX,
                   MSCOMP_AMD_PARITY_M_MAX, MSCOMP_AMD_DEV_LARGE_UNITS, MSCOMP_AMD_DIFF_NO_BASE, MSCOMP_AMD_BLOCK_GOOD, MSCOMP_AMD_BLOCK_TABLE,
                   MSCOMP_AMD_BLOCK_DECODE, MSCOMP_AMD_BLOCK_CRC, MSCOMP_AMD_BLOCK_SKIPPED, ScratchRec, BlocksView, _CODES, signature, MSCompError,
                   load_library)
from ._core import (max_compressed_size, compress, decompress, pack_offsets, Context, _run, _fetch, _Frame, _call, _outputs, _three_counts,  # noqa: F401
                    _byte_bounds, _Handle, _upload_units, _upload_unit_tables, _dev_u64, _dev_packed, _dev_block_crc, _upload_containers,
                    _new_container, _fetch_container, _covering_blocks)
from .blocks import (BlockContainer, _BlockAccess, BlockReader, BlockWriter, _blocks_views, BlockSplicer, BlockDeduper, BlockTranscoder,  # noqa: F401
                     BlockSyncer, BlockDigester, BlockParity, res_crc_dev)
from .plans import (Plan, SizePlan, DevPlan, CompressDevPlan, SizeDevPlan, CrcDevPlan, compact_dev, plan_layout_dev, layout_dev, crc32_units,  # noqa: F401
                    decompressed_sizes, decompress_units_auto, compact_batch, decompress_units, compress_units, decompress_units_host, HostViews,
                    _host_tables, compress_units_host, plan_paths, _scratch_target, scratch_names, scratch_poison, scratch_report)
from .blocks_host import (blocks_compress, blocks_crc, blocks_decompress, blocks_salvage, blocks_read, blocks_write, blocks_resize,  # noqa: F401
                          _splice_host, blocks_splice_extents, blocks_concat, blocks_split_at, blocks_cut_range, blocks_splice, _diff_pairs,
                          _extent_lists, blocks_diff, blocks_delta, blocks_patch, blocks_repair, blocks_match, blocks_match_delta,
                          blocks_match_patch, blocks_single_instance, blocks_dedup, blocks_transcode, blocks_digest, _dev_block_digest,
                          blocks_sync, blocks_sync_delta, blocks_sync_patch, blocks_parity, blocks_rebuild, res_crc_from_blocks)
from .device import BlockDiff, BlockOps, DeviceBlocks  # noqa: F401
