"""ms_compress_amd -- MI355X-native (gfx950, HIP) one-shot compressors for the MS-XCA codecs LZNT1, Xpress and
Xpress+Huffman, bit-exact with coderforlife/ms-compress, behind that library's ``mscomp.h`` C-ABI.

Only the compress hot path is here: ``csrc/`` holds the HIP kernels and the C-ABI
(``libmscomp_amd.so``, declared in ``include/mscomp_amd.h``); ``api.py`` is the host-side mirror of the
reference interface, a facade over ``_abi.py``, ``_core.py``, ``plans.py``, ``blocks.py``, ``blocks_host.py`` and ``device.py``; ``search.py`` binds the block searchers of ``include/mscomp_amd_search.h``, ``match_digest.py`` match by block digest of ``include/mscomp_amd_match_digest.h``; ``corpus.py`` the synthetic Silesia-shaped bench input; ``sharding.py`` the per-GPU split.
"""
from .api import (MSCOMP_NONE, MSCOMP_LZNT1, MSCOMP_XPRESS, MSCOMP_XPRESS_HUFF, MSCOMP_OK, MSCOMP_ERRNO,  # noqa: F401
                  MSCOMP_ARG_ERROR, MSCOMP_DATA_ERROR, MSCOMP_MEM_ERROR, MSCOMP_BUF_ERROR, FORMATS, CHUNK,
                  MSCompError, load_library, max_compressed_size, compress, compress_units, compress_units_host, decompress_units_host, HostViews, pack_offsets, decompress, decompress_units, compact_batch,
                  Context, Plan, SizePlan, decompressed_sizes, decompress_units_auto, DevPlan, layout_dev,
                  CompressDevPlan, plan_layout_dev, SizeDevPlan, compact_dev,
                  BlockContainer, blocks_compress, blocks_decompress, blocks_salvage, blocks_repair,
                  MSCOMP_AMD_BLOCK_GOOD, MSCOMP_AMD_BLOCK_TABLE, MSCOMP_AMD_BLOCK_DECODE, MSCOMP_AMD_BLOCK_CRC, MSCOMP_AMD_BLOCK_SKIPPED,
                  CrcDevPlan, crc32_units, blocks_crc,
                  BlockReader, blocks_read,
                  BlockWriter, blocks_write, blocks_resize, res_crc_dev, res_crc_from_blocks,
                  BlockSplicer, BlocksView, blocks_splice, MSCOMP_AMD_SPLICE_SRC_MAX, MSCOMP_AMD_SPLICE_ROW_TILE,
                  blocks_splice_extents, blocks_concat, blocks_split_at, blocks_cut_range,
                  BlockDeduper, blocks_dedup,
                  BlockTranscoder, blocks_transcode,
                  blocks_diff, blocks_delta, blocks_patch, MSCOMP_AMD_DIFF_NO_BASE,
                  blocks_match, blocks_match_delta, blocks_match_patch, blocks_single_instance,
                  BlockSyncer, blocks_sync, blocks_sync_delta, blocks_sync_patch, MSCOMP_AMD_SYNC_TILE,
                  BlockDigester, blocks_digest, MSCOMP_AMD_DIGEST_LEAF,
                  BlockParity, blocks_parity, blocks_rebuild, MSCOMP_AMD_PARITY_K_MAX, MSCOMP_AMD_PARITY_M_MAX,
                  device, DeviceBlocks, BlockOps, BlockDiff)
from . import search  # noqa: F401  (the binding of include/mscomp_amd_search.h: a module of its own beside api)
from .search import BlockSearcher, blocks_search, MSCOMP_AMD_SEARCH_PAT_MAX, MSCOMP_AMD_SEARCH_LEN_MAX  # noqa: F401
from . import match_digest  # noqa: F401  (the binding of include/mscomp_amd_match_digest.h, likewise)
from .match_digest import BlockDigestMatcher, blocks_match_digest, blocks_match_digest_delta  # noqa: F401
