/* include/mscomp_amd_search.h -- block searchers of libmscomp_amd.so: batched byte-pattern search in a block container. The entry points
 * live in the same library as those of mscomp_amd.h and follow its conventions (plain C types, device pointers named d_*, every call
 * asynchronous on the context's stream); they are declared here so that mscomp_amd.h keeps exactly the prototypes it has.
 *
 * Block searchers: where do these bytes occur? A searcher answers, for n_req byte ranges of a container's resources and up to 64
 * patterns at once, with every start position of every pattern, in order, without the container's data ever leaving HBM or being
 * materialised there: it is a block reader (mscomp_amd_reader_*) whose last pass scans the blocks where a reader would copy them out. It
 * needs no mscomp_amd_blocks object, only the tables a container wrote and the packed bytes, and it trusts no byte of a block before the
 * block has its verdict. A block that several requests touch is decoded once, checked once, and scanned once per request that covers it.
 *   Creation:     format, block_size = B, n_res, n_blocks_table, n_req, blocks_max and flags exactly as mscomp_amd_reader_create takes
 *                 them, with the same checks in the same order before the context is used. On top of them n_pat patterns per call,
 *                 1 <= n_pat <= MSCOMP_AMD_SEARCH_PAT_MAX; len_max, the longest pattern a call accepts, 1 <= len_max <=
 *                 MSCOMP_AMD_SEARCH_LEN_MAX; hits_max <= 0x7FFFFFF0, the records d_hits has room for; flags must be 0: otherwise
 *                 MSCOMP_ARG_ERROR. All scratch is reserved here, once, and never grows: what the reader reserves for the same bounds (the
 *                 block cache, the inner decompress dev plan, its tables) and the searcher's own columns: 8 KiB of pattern tables and 8
 *                 bytes per 4096 bytes of blocks_max B. MSCOMP_MEM_ERROR when it cannot be reserved; *sr is cleared on failure.
 *   Patterns:     pattern p is the bytes d_pat[d_pat_off[p] .. d_pat_off[p + 1]), p < n_pat; d_pat_off has n_pat + 1 entries. Both
 *                 arrays are read on the device when the call executes, so earlier work on the stream may have written them. A pattern
 *                 whose length is 0 or above len_max, or whose offsets run backwards, is refused: d_pat_status[p] = MSCOMP_ARG_ERROR,
 *                 it never hits, and the other patterns are not affected. Otherwise d_pat_status[p] = MSCOMP_OK. Equal patterns are
 *                 legal; each reports its own hits.
 *   Search:       d_req = 3 n_req uint64: resource, offset, length, clipped exactly as the reader clips them (its rule 3) to off' and
 *                 want. A hit of pattern p (of len_p bytes) in request q is a position x of the resource's data with
 *                 off' <= x < off' + want (it STARTS inside the range), x + len_p <= L (it lies inside the resource) and the bytes
 *                 [x, x + len_p) equal to the pattern. Every start position counts: overlapping occurrences are separate hits. A hit
 *                 may end up to len_p - 1 bytes behind the range, so consecutive ranges that tile a resource find every hit exactly
 *                 once. Per request, the reader's rules with two differences:
 *                   1-3. as mscomp_amd_reader_read: MSCOMP_ARG_ERROR for r >= n_res or a d_block_first entry above n_blocks_table,
 *                      MSCOMP_DATA_ERROR for a wrong block count, the clipping; want = 0 is MSCOMP_OK with no blocks and no hits;
 *                   4. there is no capacity rule;
 *                   5. the budget counts the blocks that cover [off', min(L, off' + want + len_max - 1)): the range and its
 *                      look-ahead. The look-ahead is len_max, the creation constant, whatever the patterns of the call: admission
 *                      stays a pass over the tables that depends on no data. Otherwise as the reader's: a running total in request
 *                      order, before any sharing, MSCOMP_ARG_ERROR above blocks_max;
 *                   6. as the reader's, over those covering blocks, the look-ahead's included: table checks, decode, and with
 *                      d_block_crc the CRC-32 of every whole block; any failure is MSCOMP_DATA_ERROR for every request that covers
 *                      the block and for no other.
 *                 A request that is not MSCOMP_OK has d_req_hits[q] = 0 and contributes no hit.
 *   Results:      d_req_hits[q] (n_req) = the exact number of hits of request q; d_count[0] = their exact total; d_count[1] =
 *                 min(d_count[0], hits_max) = the records written. Record i is d_hits[2 i] = x, d_hits[2 i + 1] = (q << 32) | p. The
 *                 records are in ascending (q, x, p) order; when there are more hits than hits_max, the records are the first
 *                 hits_max of that order -- the same ones every time, and a caller can retry with more room knowing how much.
 *                 Nothing is written at or behind d_hits[2 d_count[1]].
 *   Sharing:      as the reader's: a unit is one (request, covering block) pair, the lowest unit that covers a block owns it, only
 *                 owners are decoded or read raw and checksummed. mscomp_amd_searcher_counts gives the reader's three numbers for the
 *                 last execution (units, distinct blocks, blocks decoded rather than raw), synchronises the stream and returns -1 on
 *                 error, 0 otherwise.
 *   Execution:    as the reader's: asynchronous on the ctx stream, kernels only (no memset or copy node), no allocation, no
 *                 synchronisation, nothing read back, a launch sequence fixed by the creation bounds. Legal while the caller captures
 *                 the ctx stream, the first execution included; outside capture the call replays a graph of its own from its second
 *                 execution on, captured again when an argument changes. MSCOMP_ARG_ERROR for a null sr or a null required array
 *                 (d_packed may be null when blocks_max is 0, d_res_len when n_res is 0, d_req, d_req_hits and d_status when n_req is
 *                 0, d_hits when hits_max is 0, d_block_crc always). n_req = 0 returns MSCOMP_OK and writes nothing.
 *   Left out:     patterns longer than 256 bytes, regular expressions, case folding; hits that span two resources; searching the
 *                 stored (undecoded) bytes; more than 64 patterns per call; the device layer of the Python package (BlockOps) and
 *                 the scratch-report hooks (mscomp_amd_debug_scratch_*), which do not know a searcher. */
#ifndef MSCOMP_AMD_SEARCH_H
#define MSCOMP_AMD_SEARCH_H
#include "mscomp_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MSCOMP_AMD_SEARCH_PAT_MAX 64u     /* patterns per searcher */
#define MSCOMP_AMD_SEARCH_LEN_MAX 256u    /* bytes per pattern: below the smallest block, so a hit spans at most two blocks */
typedef struct mscomp_amd_searcher mscomp_amd_searcher;
MSCompStatus mscomp_amd_searcher_create(mscomp_amd_ctx* ctx, MSCompFormat format, uint32_t block_size, size_t n_res, uint64_t n_blocks_table,
                                        size_t n_req, uint64_t blocks_max, uint32_t n_pat, uint32_t len_max, uint64_t hits_max, uint32_t flags,
                                        mscomp_amd_searcher** sr);
void         mscomp_amd_searcher_destroy(mscomp_amd_searcher* sr);
MSCompStatus mscomp_amd_searcher_search(mscomp_amd_searcher* sr, const uint8_t* d_packed, uint64_t packed_len,
                                        const uint64_t* d_block_first, const uint64_t* d_block_off, const uint64_t* d_res_len,
                                        const uint32_t* d_block_crc /* may be NULL */,
                                        const uint64_t* d_req /* 3 n_req: resource, offset, length */,
                                        const uint8_t* d_pat, const uint64_t* d_pat_off /* n_pat + 1 */,
                                        uint64_t* d_hits /* 2 hits_max */, uint64_t* d_req_hits /* n_req */, uint64_t* d_count /* 2 */,
                                        int32_t* d_pat_status /* n_pat */, int32_t* d_status /* n_req */);
int          mscomp_amd_searcher_counts(mscomp_amd_searcher* sr, uint32_t out[3]);

#ifdef __cplusplus
}
#endif
#endif
