/* include/mscomp_amd_match_digest.h -- block dedupers of libmscomp_amd.so that match by block digest. The entry points live in the same
 * library as those of mscomp_amd.h and follow its conventions (plain C types, device pointers named d_*, every call asynchronous on the
 * context's stream); they are declared here so that mscomp_amd.h keeps exactly the prototypes it has.
 *
 * Match by digest: mscomp_amd_deduper_match (mscomp_amd.h) decides equality on the STORED bytes, so its views must share one format and
 * every payload must lie in HBM. A digester (mscomp_amd_digester_blocks) writes 128 bits of BLAKE2s per block over the block's DATA: that
 * column survives a transcode and a move, and it is all this call reads of a block. For every block of the resources of a container (next),
 * whether an EQUAL block lies in one of up to three stores, earlier in next, or nowhere -- equal by data length and digest --, answered
 * word for word in the shape match gives: the DELTA and the PATCH extent lists, the classes, the counts, the statuses. No stored byte is
 * read, so a store may be known by its tables and its column alone ("which blocks do I have to send?"), and the views of one call may be
 * written by different codecs. The contract is match's ("Rules" of mscomp_amd_deduper_match, mscomp_amd.h) with the differences below and
 * nothing else.
 *   Creation:     mscomp_amd_deduper_create_match_digest makes a mscomp_amd_deduper of a fourth kind beside dedup's, diff's, match's and
 *                 repair's (destroyed by mscomp_amd_deduper_destroy, reported by the scratch hooks under MSCOMP_AMD_SCRATCH_DEDUPER), with
 *                 the arguments, the bounds and the checks of mscomp_amd_deduper_create_match, in the same order, before the context is
 *                 used and with *dd cleared: MSCOMP_ARG_ERROR for a null ctx or dd, a block_size that is not a power of two from 4096 to
 *                 524288, n_src above 3 (0 is legal: no store), non-zero flags, n_res_total or n_blocks_total above 0x7FFFFFF0, or
 *                 n_blocks_new above n_blocks_total; MSCOMP_MEM_ERROR when the scratch cannot be reserved. Such a deduper answers
 *                 mscomp_amd_deduper_dedup, _diff, _match and _repair with MSCOMP_ARG_ERROR and launches nothing, and a deduper made by
 *                 any other create answers mscomp_amd_deduper_match_digest the same way.
 *   Scratch:      match's formula, reserved once, at creation, and never grown: 48 n_res_total + 40 n_blocks_total + 4 n_blocks_new +
 *                 64 ceil(n_blocks_new / MSCOMP_AMD_SPLICE_ROW_TILE) + 848 bytes -- match keeps no table for its compare's slices, so
 *                 dropping that pass frees nothing, and the digests are read where the caller holds them. No context buffer is used.
 *   Sources:      as match's. mscomp_amd_blocks_view does not change; the digest columns travel beside the views: d_store_digest is a HOST
 *                 array of n_src device pointers (may be null when n_src is 0), d_store_digest[s] the column of store[s], d_next_digest the
 *                 column of next. A column has four uint32 words per table row of its view, 4 n_blocks_table in all, row j's at
 *                 [4 j, 4 j + 3] -- the layout mscomp_amd_digester_blocks writes --, and must be 16-byte aligned (a row is one load). It
 *                 is read on the device when the call executes. A null column for a view with n_res > 0, or a misaligned one, is
 *                 MSCOMP_ARG_ERROR from the call, on the host, with nothing launched.
 *   Rules:        match's rules 1-8 with rule 6 replaced. Rules 1-3 are unchanged, so rule 3 still holds every row to
 *                 off[j] <= off[j + 1] <= packed_len of its view, whatever d_packed is.
 *                   6. equality: two rows are EQUAL when their data lengths e(k) are equal and their four digest words are equal. Stored
 *                      lengths, CRC words and stored bytes take no part: d_block_crc of a view is ignored and may be null in some views
 *                      and not in others. rep, FOUND / SHARED / FRESH, the runs of rule 7, both extent lists, d_class, d_count[0 .. 4]
 *                      and d_status are defined from this equality exactly as match defines them from its own; d_count[4] is still the
 *                      stored bytes of the fresh rows, from next's offset table. The digest of a row of a refused resource is not read.
 *   Payload:      nothing dereferences d_packed: it may be null with any packed_len, in any view.
 *   Formats:      the call has no format argument, as match has none. The verdicts, the classes, the counts and the DELTA list are right
 *                 whatever codec each view was written with; the delta extents refer to next alone, so the delta splice always gives a
 *                 container, of next's format. The PATCH list names rows of the stores: splicing it gives a container only when all views
 *                 share a format and a block size -- the caller's duty, as for match and for splice. Across formats the patch list is a
 *                 read recipe: every extent names (source, resource, first block, count), which that source's reader or ranged decode
 *                 serves. B is common to all views in either case: a digest belongs to a block of B bytes. By the data-length clause of
 *                 rule 6 a short block is only ever represented by a short block of the SAME data length, and no full block by a short
 *                 one, so splice-extents' rule 4 holds by the argument match's header gives.
 *   Key:          the KEY TUPLE of a row is its data length and its digest words h0 and h1, mixed into 64 bits; the candidate of a row is
 *                 the smallest row with the same key. REFUTED, d_count[5], is the number of rows of accepted resources, stores included,
 *                 that share their key with a smaller row but are not equal to the smallest such one. They are still answered exactly:
 *                 rep is the smallest EQUAL row. With true digests this takes two blocks that agree in 64 bits of BLAKE2s and is never
 *                 hit; with a caller-made column it is.
 *   Trust:        the columns are taken as given. A digest that does not belong to its block gives an answer about the column, not about
 *                 the data: two blocks with one digest are one block to this call. mscomp_amd_digester_check holds decoded data to the
 *                 column, and the reader still holds every row it decodes to its CRC-32.
 *   Consequence:  for healthy containers of one format and one block size, with checksums present in every view and columns written by
 *                 mscomp_amd_digester_blocks over their data, every output equals what mscomp_amd_deduper_match writes for the same views,
 *                 d_count[5] apart; both splices of match's consequence then rebuild next byte for byte.
 *   Execution:    as match's: asynchronous on the ctx stream, kernels only (no memset or copy node), no allocation, no synchronisation,
 *                 nothing read back, ten launches fixed by the creation bounds (three when n_blocks_total is 0, seven when n_blocks_new
 *                 is 0): the key table cleared; the seed; rule 3, the keys and the confirm, fixed grids over the rows with a lane per row
 *                 -- the confirm compares a data length and 16 bytes per row, there is no pass over data --; the settle, one workgroup;
 *                 the three run passes in tiles of MSCOMP_AMD_SPLICE_ROW_TILE rows of next; the counts. Legal inside a caller's capture
 *                 from the first execution, a graph of its own from the second outside one, captured again when an argument changes --
 *                 a field of a view and a digest pointer count as arguments. MSCOMP_ARG_ERROR for a null dd, next or d_count, a null
 *                 store or d_store_digest when n_src > 0, a deduper of another kind, any other null array when n_res_total > 0
 *                 (d_delta_ext and d_patch_ext may be null while n_blocks_new is 0), a view with a null table while its n_res > 0, or
 *                 views beyond the creation bounds.
 *   Left out:     dedup and diff by digest; a digest per resource; different block sizes in one call -- digests are per block of B, so B
 *                 stays common --; carrying the column through write, resize, splice and transcode (a caller digests the new container
 *                 again); and what match leaves out. */
#ifndef MSCOMP_AMD_MATCH_DIGEST_H
#define MSCOMP_AMD_MATCH_DIGEST_H
#include "mscomp_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

MSCompStatus mscomp_amd_deduper_create_match_digest(mscomp_amd_ctx* ctx, uint32_t block_size, uint32_t n_src /* 0 .. 3 stores */, size_t n_res_total,
                                                    uint64_t n_blocks_total, uint64_t n_blocks_new, uint32_t flags, mscomp_amd_deduper** dd);
MSCompStatus mscomp_amd_deduper_match_digest(mscomp_amd_deduper* dd,
                                             const mscomp_amd_blocks_view* store /* host array, n_src; may be NULL when n_src is 0 */,
                                             const uint32_t* const* d_store_digest /* host array of n_src device pointers, 4 n_blocks_table words each */,
                                             const mscomp_amd_blocks_view* next  /* host, by value, only read */,
                                             const uint32_t* d_next_digest     /* 4 next->n_blocks_table */,
                                             uint64_t* d_delta_ext_first       /* next->n_res + 1 */,
                                             uint64_t* d_delta_ext             /* 4 n_blocks_new */,
                                             uint64_t* d_patch_ext_first       /* next->n_res + 1 */,
                                             uint64_t* d_patch_ext             /* 4 n_blocks_new */,
                                             uint64_t* d_class                 /* 3 next->n_res: found, shared, fresh blocks of the resource */,
                                             uint64_t* d_count                 /* 6: found, shared, fresh, rows looked at, fresh stored bytes, refuted */,
                                             int32_t*  d_status                /* one per resource: the stores' back to back, then next's */);

#ifdef __cplusplus
}
#endif
#endif
