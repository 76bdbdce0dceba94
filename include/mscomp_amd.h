/* include/mscomp_amd.h -- C-ABI of libmscomp_amd.so, the MI355X-native drop-in for the one-shot
 * compressors of coderforlife/ms-compress.
 *
 * Part 1 re-exports, with identical names / argument meaning / error behaviour, exactly the symbols that
 * the reference's three compressor translation units and its facade export for this path:
 *
 *   reference symbol (file:line)                                              -> replaced by
 *   ms_compress               include/mscomp.h:59,  src/mscomp.cpp:113-117     -> ms_compress
 *   ms_max_compressed_size    include/mscomp.h:99,  src/mscomp.cpp:96-100      -> ms_max_compressed_size
 *   lznt1_compress            include/lznt1.h:49,   src/lznt1_compress.cpp:233 -> lznt1_compress
 *   lznt1_max_compressed_size include/lznt1.h:50,   src/lznt1_compress.cpp:27  -> lznt1_max_compressed_size
 *   xpress_compress           include/xpress.h:47,  src/xpress_compress.cpp:240-> xpress_compress
 *   xpress_max_compressed_size include/xpress.h:48, src/xpress_compress.cpp:30 -> xpress_max_compressed_size
 *   xpress_huff_compress      include/xpress_huff.h:46, src/xpress_huff_compress.cpp:247 -> xpress_huff_compress
 *   xpress_huff_max_compressed_size include/xpress_huff.h:47, src/xpress_huff_compress.cpp:46 -> (same name)
 *
 * These take HOST pointers (the reference contract). Every byte of output is produced by HIP kernels on
 * the current device; there is no CPU encoder in this library -- if no usable GPU/HIP runtime is present
 * the calls return MSCOMP_ERRNO and never fall back.
 *
 * Part 1 also holds the rows SURVEY.md 8f lists next, each declared below with the reference file:line it replaces:
 * the one-shot decompressors (ms_decompress, lznt1_decompress, xpress_decompress, xpress_huff_decompress) and the
 * LZNT1 streaming compressor / decompressor with the reference's stream object (ms_deflate*, ms_inflate*, lznt1_deflate*,
 * lznt1_inflate*). Same rule: the bytes come from the GPU, there is no CPU codec to fall back to.
 *
 * Part 2 is the additive batch interface the GPU needs (SURVEY.md 8b "batch extension"): many independent
 * units (buffers) already resident in HBM, compressed (or decompressed) in one pass, output written to HBM; plus
 * capacity planning and device-side compaction of a batch's outputs.
 *
 * Plain C types only (no torch / HIP types in any signature; a hipStream_t is passed as void*).
 */
#ifndef MSCOMP_AMD_H
#define MSCOMP_AMD_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- enums: values identical to include/mscomp/general.h:65-93 of the reference ---- */
typedef enum _MSCompFormat {
	MSCOMP_NONE = 0, MSCOMP_RESERVED = 1, MSCOMP_LZNT1 = 2, MSCOMP_XPRESS = 3, MSCOMP_XPRESS_HUFF = 4
} MSCompFormat;
typedef enum _MSCompStatus {
	MSCOMP_OK = 0, MSCOMP_STREAM_END = 1, MSCOMP_POSSIBLE_STREAM_END = 2,
	MSCOMP_ERRNO = -1, MSCOMP_ARG_ERROR = -2, MSCOMP_DATA_ERROR = -3, MSCOMP_MEM_ERROR = -4, MSCOMP_BUF_ERROR = -5
} MSCompStatus;

/* ================= Part 1: drop-in one-shot interface (host pointers) ================= */
MSCompStatus ms_compress(MSCompFormat format, const uint8_t* in, size_t in_len, uint8_t* out, size_t* out_len);
size_t       ms_max_compressed_size(MSCompFormat format, size_t in_len);

MSCompStatus lznt1_compress(const uint8_t* in, size_t in_len, uint8_t* out, size_t* out_len);
size_t       lznt1_max_compressed_size(size_t in_len);
MSCompStatus xpress_compress(const uint8_t* in, size_t in_len, uint8_t* out, size_t* out_len);
size_t       xpress_max_compressed_size(size_t in_len);
MSCompStatus xpress_huff_compress(const uint8_t* in, size_t in_len, uint8_t* out, size_t* out_len);
size_t       xpress_huff_max_compressed_size(size_t in_len);

/* Decompressors. Same contract as the reference: *out_len holds the capacity on entry and the number of
 * bytes produced on MSCOMP_OK; MSCOMP_BUF_ERROR when the output (or what is left of the input) does not fit,
 * MSCOMP_DATA_ERROR for a malformed stream.
 *   ms_decompress      include/mscomp.h:88,   src/mscomp.cpp:119-134               -> ms_decompress
 *   lznt1_decompress   include/lznt1.h:51,    src/lznt1_decompress.cpp:293 (the inflate wrapper, internal.h:616-630) -> lznt1_decompress
 *   xpress_decompress  include/xpress.h:50,   src/xpress_decompress.cpp:405                -> xpress_decompress
 *   xpress_huff_decompress include/xpress_huff.h:49, src/xpress_huff_decompress.cpp:130      -> xpress_huff_decompress */
MSCompStatus ms_decompress(MSCompFormat format, const uint8_t* in, size_t in_len, uint8_t* out, size_t* out_len);
MSCompStatus lznt1_decompress(const uint8_t* in, size_t in_len, uint8_t* out, size_t* out_len);
MSCompStatus xpress_decompress(const uint8_t* in, size_t in_len, uint8_t* out, size_t* out_len);
MSCompStatus xpress_huff_decompress(const uint8_t* in, size_t in_len, uint8_t* out, size_t* out_len);

/* Streaming compression: the reference's stream object and its LZNT1 streaming compressor -- the only format
 * whose ms_deflate works in the reference. Layout of mscomp_stream = include/mscomp/general.h:95-121 in the default build
 * (MSCOMP_WITH_ERROR_MESSAGES and MSCOMP_WITH_WARNING_MESSAGES, include/mscomp/config.h:54-63). Same call protocol and statuses
 * (include/mscomp.h:102-158); the bytes are those of the reference for every way of slicing the input and the output windows.
 *   ms_deflate_init / ms_deflate / ms_deflate_end          include/mscomp.h:114,143,158, src/mscomp.cpp:136-165 (MSCOMP_NONE, MSCOMP_LZNT1)
 *   lznt1_deflate_init / lznt1_deflate / lznt1_deflate_end include/lznt1.h:55-57,       src/lznt1_compress.cpp:132-231 */
typedef enum _MSCompFlush { MSCOMP_NO_FLUSH = 0, MSCOMP_FLUSH = 2, MSCOMP_FINISH = 4 } MSCompFlush;
typedef struct _mscomp_internal_state mscomp_internal_state;
typedef struct _mscomp_stream {
	MSCompFormat format;
#ifdef __cplusplus
	bool compressing;
#else
	int compressing;
#endif
	const uint8_t* in;  size_t in_avail,  in_total;
	uint8_t*       out; size_t out_avail, out_total;
	char error[256];
	char warning[256];
	mscomp_internal_state* state;
} mscomp_stream;
MSCompStatus ms_deflate_init(MSCompFormat format, mscomp_stream* stream);
MSCompStatus ms_deflate(mscomp_stream* stream, MSCompFlush flush);
MSCompStatus ms_deflate_end(mscomp_stream* stream);
MSCompStatus lznt1_deflate_init(mscomp_stream* stream);
MSCompStatus lznt1_deflate(mscomp_stream* stream, MSCompFlush flush);
MSCompStatus lznt1_deflate_end(mscomp_stream* stream);
/* The Xpress streaming compressor is unfinished in the reference; its three entry points exist and return fixed statuses in the default
 * build (include/xpress.h:52-54; src/xpress_compress.cpp:52-73 MSCOMP_MEM_ERROR, :74-218 MSCOMP_ARG_ERROR, :219-235 stream check). Exported
 * with the same statuses so that a program naming them links against the drop-in and sees what it saw before. */
MSCompStatus xpress_deflate_init(mscomp_stream* stream);
MSCompStatus xpress_deflate(mscomp_stream* stream, MSCompFlush flush);
MSCompStatus xpress_deflate_end(mscomp_stream* stream);
/* ... and its streaming decompressor: ms_inflate_init / ms_inflate / ms_inflate_end (include/mscomp.h:174,198,213, src/mscomp.cpp:167-196;
 * MSCOMP_NONE and MSCOMP_LZNT1) and lznt1_inflate_init / lznt1_inflate / lznt1_inflate_end (include/lznt1.h:59-61,
 * src/lznt1_decompress.cpp:210-290). Every chunk is decoded on the GPU. */
/* xpress_inflate_init / xpress_inflate / xpress_inflate_end (include/xpress.h:56-58, src/xpress_decompress.cpp:45-403) are NOT offloaded (one
 * stream is a serial token chain, handed over piecewise): the symbols exist so that programs naming them link; xpress_inflate_init -- and
 * ms_inflate_init(MSCOMP_XPRESS) -- returns MSCOMP_MEM_ERROR without touching the stream, the other two MSCOMP_ARG_ERROR. Build with
 * -DMSCOMP_AMD_NO_XPRESS_INFLATE and keep the reference's xpress_decompress.cpp in the link where streaming Xpress decompression is needed. */
MSCompStatus xpress_inflate_init(mscomp_stream* stream);
MSCompStatus xpress_inflate(mscomp_stream* stream);
MSCompStatus xpress_inflate_end(mscomp_stream* stream);
MSCompStatus ms_inflate_init(MSCompFormat format, mscomp_stream* stream);
MSCompStatus ms_inflate(mscomp_stream* stream);
MSCompStatus ms_inflate_end(mscomp_stream* stream);
MSCompStatus lznt1_inflate_init(mscomp_stream* stream);
MSCompStatus lznt1_inflate(mscomp_stream* stream);
MSCompStatus lznt1_inflate_end(mscomp_stream* stream);

/* ================= Part 2: batch interface (device pointers) ================= */
typedef struct mscomp_amd_ctx  mscomp_amd_ctx;    /* one per (device, stream); owns scratch in HBM  */
typedef struct mscomp_amd_plan mscomp_amd_plan;   /* unit layout of one batch, uploaded once        */

/* device = HIP ordinal; hip_stream = hipStream_t to launch on (NULL = the null stream).
 * A context belongs to ONE host thread at a time (its scratch, its pinned table staging and its pool of table buffers are not locked): use one
 * context per thread -- the one-shot entries of Part 1 do that themselves (a thread-local context), mscomp_amd_compress_units_host keeps one per
 * sub-batch slot. mscomp_amd_plan_create must not run while the context's stream is being captured into a graph (it waits on an event of that
 * stream when its table staging is still in flight); capture mscomp_amd_plan_execute instead, with the plan made beforehand. */
MSCompStatus mscomp_amd_ctx_create(int device, void* hip_stream, mscomp_amd_ctx** ctx);
void         mscomp_amd_ctx_destroy(mscomp_amd_ctx* ctx);

/* A batch is n_units independent buffers resident in HBM. Unit i is (all four arrays: n_units entries, host memory)
 *   input    d_in  + in_off[i]  , in_len[i]  bytes
 *   output   d_out + out_off[i] , out_cap[i] bytes of capacity
 * and is compressed exactly as one ms_compress(format, ...) call would compress it:
 *   LZNT1        4 KiB chunks inside the unit, End_of_buffer 00 00 appended when capacity allows
 *   XPRESS       one Xpress stream per unit
 *   XPRESS_HUFF  64 KiB chunks inside the unit, matches reach into the previous chunk, EOS in the last
 * Units must not overlap on the output side. For best load/store width keep in_off[i] and out_off[i] multiples
 * of 16 (any alignment is accepted). */
MSCompStatus mscomp_amd_plan_create(mscomp_amd_ctx* ctx, MSCompFormat format, size_t n_units,
                                    const uint64_t* in_off, const uint64_t* in_len,
                                    const uint64_t* out_off, const uint64_t* out_cap, mscomp_amd_plan** plan);
void         mscomp_amd_plan_destroy(mscomp_amd_plan* plan);

/* Asynchronous on the ctx stream. d_out_len[i] (device, uint64) receives the compressed size of unit i,
 * d_status[i] (device, int32) MSCOMP_OK or MSCOMP_BUF_ERROR (unit did not fit its capacity; its output
 * bytes are then unspecified). Returns MSCOMP_OK when everything was enqueued, MSCOMP_ERRNO on a HIP error. */
MSCompStatus mscomp_amd_plan_execute(mscomp_amd_plan* plan, const uint8_t* d_in, uint8_t* d_out,
                                     uint64_t* d_out_len, int32_t* d_status);

/* SURVEY.md 8e "Multi-GPU" + 8f-3 "host pipeline" (no counterpart in the reference: ms_compress, mscomp.h:59 / src/mscomp.cpp:113-117, is one
 * buffer per call on one thread): n independent units given by HOST pointers, compressed on n_dev GPUs of this process. Unit i is exactly one
 * ms_compress(format, in_ptrs[i], in_lens[i], out_ptrs[i], &out_lens[i]) call with *out_len = out_caps[i] on entry: same bytes, statuses[i] =
 * MSCOMP_OK or MSCOMP_BUF_ERROR (out_lens[i] = 0 and nothing written behind the capacity then), the uncounted LZNT1 00 00 behind the stream
 * when the capacity has room. Bytes of a unit's capacity behind its stream are unspecified afterwards.
 * devices = n_dev device ordinals (NULL: 0 .. n_dev - 1; the same ordinal may appear twice: two ranges share that GPU). The units are cut into
 * n_dev contiguous ranges with near-equal input bytes (no exchange step, no collective: units are independent); every range runs on its own
 * host thread as a pipeline of sub-batches (MSCOMP_AMD_HOST_BATCH_MB MiB of input each, default 32 -- 96 for Xpress+Huffman --, up to
 * MSCOMP_AMD_HOST_SLOTS = 8 in flight, each with its own context and stream; an uploader and a downloader thread beside it); units
 * that lie back to back in the caller's memory travel as one copy. Returns MSCOMP_OK when every range ran (per-unit results in statuses),
 * MSCOMP_ARG_ERROR for a bad format / device / pointer, MSCOMP_MEM_ERROR / MSCOMP_ERRNO when a range could not run (statuses of units not
 * reached stay MSCOMP_ERRNO; a failed allocation or a thread the system refuses is MSCOMP_MEM_ERROR, never an abort: csrc/hostbatch.hip is built
 * with exceptions and catches at this boundary). ONE LZNT1 unit of 36 MiB or more on the calling thread's range takes the one-shot call's path
 * (caller buffers mapped into the GPU's address space; the two environment knobs do not apply to it). With outputs laid out capacity after
 * capacity, the bytes of a capacity behind its stream -- including the capacities of units that failed -- are unspecified afterwards (they come
 * down with the streams in one copy). Contexts and staging are kept per device between calls; mscomp_amd_host_pool_release() frees them. */
MSCompStatus mscomp_amd_compress_units_host(MSCompFormat format, int n_dev, const int* devices, size_t n_units,
                                            const uint8_t* const* in_ptrs, const size_t* in_lens, uint8_t* const* out_ptrs, const size_t* out_caps,
                                            size_t* out_lens, MSCompStatus* statuses);
/* The same for the decoders: unit i is one ms_decompress call (mscomp.h:88) with *out_len = out_caps[i] on entry; statuses[i] =
 * MSCOMP_OK / MSCOMP_BUF_ERROR / MSCOMP_DATA_ERROR exactly as the reference's one-shot decoder returns them (DESIGN_DECODERS.md). */
MSCompStatus mscomp_amd_decompress_units_host(MSCompFormat format, int n_dev, const int* devices, size_t n_units,
                                              const uint8_t* const* in_ptrs, const size_t* in_lens, uint8_t* const* out_ptrs, const size_t* out_caps,
                                              size_t* out_lens, MSCompStatus* statuses);
void         mscomp_amd_host_pool_release(void);

/* Convenience: create plan + execute + stream-synchronize + destroy. */
MSCompStatus mscomp_amd_compress_batch(mscomp_amd_ctx* ctx, MSCompFormat format, size_t n_units,
                                       const uint8_t* d_in, const uint64_t* in_off, const uint64_t* in_len,
                                       uint8_t* d_out, const uint64_t* out_off, const uint64_t* out_cap,
                                       uint64_t* d_out_len, int32_t* d_status);

/* The same for decompression: unit i holds one compressed buffer (what one ms_decompress call takes), out_cap[i] is the
 * capacity the caller passes in *out_len. d_status[i] is MSCOMP_OK / MSCOMP_BUF_ERROR / MSCOMP_DATA_ERROR exactly as the
 * reference's one-shot call returns them; d_out_len[i] is the decompressed size on MSCOMP_OK (0 otherwise; the output bytes
 * of a failed unit are unspecified). Executed with mscomp_amd_plan_execute. Units are limited to 4 GiB - 4096 of input. */
MSCompStatus mscomp_amd_plan_create_decompress(mscomp_amd_ctx* ctx, MSCompFormat format, size_t n_units,
                                               const uint64_t* in_off, const uint64_t* in_len,
                                               const uint64_t* out_off, const uint64_t* out_cap, mscomp_amd_plan** plan);
MSCompStatus mscomp_amd_decompress_batch(mscomp_amd_ctx* ctx, MSCompFormat format, size_t n_units,
                                         const uint8_t* d_in, const uint64_t* in_off, const uint64_t* in_len,
                                         uint8_t* d_out, const uint64_t* out_off, const uint64_t* out_cap,
                                         uint64_t* d_out_len, int32_t* d_status);

/* Decompressed-size query: what a decompress plan would report, without decoding. Unit i is d_in + in_off[i], in_len[i] bytes, and
 * limit[i] (host, n_units entries; limit = NULL means UINT64_MAX for every unit) is the capacity L it is judged at. For every unit
 *   d_status[i]   the status of ms_decompress(format, unit, in_len[i], out, &cap) with cap = L -- the same status a decompress plan with
 *                 out_cap[i] = L reports (MSCOMP_OK / MSCOMP_BUF_ERROR / MSCOMP_DATA_ERROR)
 *   d_out_len[i]  the *out_len of that call on MSCOMP_OK, 0 otherwise (64-bit: an Xpress stream can stand for more than 4 GiB)
 *   d_need[i]     on MSCOMP_OK the smallest capacity at which that call returns MSCOMP_OK, 0 otherwise. It is d_out_len[i], except for an
 *                 LZNT1 stream that ends in the End_of_buffer header 00 00 (which ms_compress writes, uncounted, whenever there is room):
 *                 the decoder reads a header only while output room is left, so such a stream needs d_out_len[i] + 1.
 * The capacities at which a unit decodes form the interval [need, infinity), with the same output at each. A unit that is MSCOMP_BUF_ERROR
 * at L is NOT promised to decode at a larger L (an LZNT1 stream cut inside a chunk is BUF_ERROR at every capacity; some damaged streams
 * are BUF_ERROR at small capacities and DATA_ERROR at large ones). d_out_len / d_need (uint64) and d_status (int32) are device arrays.
 * Argument checks are those of mscomp_amd_plan_create_decompress (MSCOMP_ARG_ERROR for a bad format, null arrays, an in_len above
 * 0xFFFFF000). Scratch and host work scale with the input bytes and the number of units, never with the limits. A size plan is executed
 * only with mscomp_amd_plan_execute_size (asynchronous on the ctx stream, allocates nothing, does not synchronize), and that function takes
 * nothing else: either one given the other kind of plan returns MSCOMP_ARG_ERROR. mscomp_amd_plan_destroy frees both kinds.
 * mscomp_amd_decompressed_size_batch = create + execute + stream-synchronize + destroy. */
MSCompStatus mscomp_amd_plan_create_size(mscomp_amd_ctx* ctx, MSCompFormat format, size_t n_units,
                                         const uint64_t* in_off, const uint64_t* in_len, const uint64_t* limit, mscomp_amd_plan** plan);
MSCompStatus mscomp_amd_plan_execute_size(mscomp_amd_plan* plan, const uint8_t* d_in, uint64_t* d_out_len, uint64_t* d_need, int32_t* d_status);
MSCompStatus mscomp_amd_decompressed_size_batch(mscomp_amd_ctx* ctx, MSCompFormat format, size_t n_units, const uint8_t* d_in,
                                                const uint64_t* in_off, const uint64_t* in_len, const uint64_t* limit,
                                                uint64_t* d_out_len, uint64_t* d_need, int32_t* d_status);

/* Decompress plans with device tables: created once from bounds, executed many times with unit tables that GPU work earlier on the ctx stream
 * has written (the d_out_len of a compress plan or dev plan, the d_need of a size dev plan or of the size query, the offsets of
 * mscomp_amd_layout_dev, mscomp_amd_compact_dev or mscomp_amd_compact_batch). n_units is fixed when the plan is created. Two caps apply to the units, summed in unit order:
 *   total in_len  <= in_total_max   (across all units)
 *   total out_cap <= out_total_max  (across all units)
 * d_in_off, d_in_len, d_out_off, d_out_cap: device arrays of n_units uint64, read when the work runs on the ctx stream.
 *   Per-unit results: for every unit that passes the checks below, d_status[i] and d_out_len[i], and the bytes on MSCOMP_OK, are exactly those
 *                 of a decompress plan (mscomp_amd_plan_create_decompress) with the same values -- what one ms_decompress call returns.
 *   Units that fail the checks: a unit gets MSCOMP_ARG_ERROR, d_out_len = 0, and nothing is read or written for it, if its in_len is above
 *                 0xFFFFF000, or the running total of in_len up to and including it is above in_total_max, or the running total of out_cap up
 *                 to and including it is above out_total_max. The other units are unaffected. Offsets are the caller's responsibility.
 *   Execution:    mscomp_amd_plan_execute_dev is asynchronous on the ctx stream; it allocates nothing, does not synchronize and reads nothing back
 *                 to the host. It may run while the ctx stream is being captured into a graph (it then enqueues plain launches). Outside
 *                 capture it replays a graph of its own from its second execution on, captured again whenever one of its pointers changes.
 *                 MSCOMP_ARG_ERROR for a null plan or array (d_in / d_out may be null when the matching bound is 0).
 *   Plan kinds:   mscomp_amd_plan_execute and mscomp_amd_plan_execute_size return MSCOMP_ARG_ERROR for a dev plan, mscomp_amd_plan_execute_dev
 *                 for any other plan (a size dev plan included), without enqueueing anything. mscomp_amd_plan_destroy frees every kind.
 *   Creation:     the argument checks of mscomp_amd_plan_create_decompress (MSCOMP_ARG_ERROR for a null ctx or plan pointer or a bad format);
 *                 MSCOMP_MEM_ERROR when the scratch for the bounds cannot be reserved. The scratch is reserved for the bounds, once.
 * Dev plans decode without the optional paths that need tables chosen on the host (DESIGN_DECODERS.md): below 512 KiB of Xpress input and
 * 1 MiB of capacity per unit they run the same kernels as a host plan; larger units decode to the same bytes, more slowly
 * (mscomp_amd_plan_create_decompress_dev_ex below builds those tables on the device). */
MSCompStatus mscomp_amd_plan_create_decompress_dev(mscomp_amd_ctx* ctx, MSCompFormat format, size_t n_units,
                                                   uint64_t in_total_max, uint64_t out_total_max, mscomp_amd_plan** plan);
MSCompStatus mscomp_amd_plan_execute_dev(mscomp_amd_plan* plan, const uint8_t* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len,
                                         uint8_t* d_out, const uint64_t* d_out_off, const uint64_t* d_out_cap,
                                         uint64_t* d_out_len, int32_t* d_status);
/* Exclusive running sum of d_cap[i] rounded up to `align` (0 counts as 1), written to d_off[0..n_units] (d_off[n_units] = total; a sum beyond
 * 2^64 - 1 stays there), on the ctx stream: it turns d_need of the size query, or d_out_len of a compress plan, into a packed layout without
 * leaving the GPU. d_cap and d_off are device arrays (uint64). Asynchronous; allocates nothing. */
MSCompStatus mscomp_amd_layout_dev(mscomp_amd_ctx* ctx, size_t n_units, const uint64_t* d_cap, uint64_t align, uint64_t* d_off);

/* Size plans with device tables: the decompressed-size query (mscomp_amd_plan_create_size) of a batch whose tables GPU work has written -- the
 * d_out_len of a compress dev plan with the offsets of mscomp_amd_plan_layout_dev or mscomp_amd_compact_dev, say. Created once from bounds;
 * n_units is fixed when the plan is created. One cap applies to the units, summed in unit order:
 *   total in_len  <= in_total_max   (across all units)
 * A size plan's scratch follows the input alone (no token slots, no candidate token scratch): there is no output bound.
 * d_in_off, d_in_len, d_limit: device arrays of n_units uint64, read when the work runs on the ctx stream. d_limit = NULL means no limit
 * (UINT64_MAX for every unit), as for the host form.
 *   Per-unit results: for every unit that passes the checks below, d_status[i], d_out_len[i] and d_need[i] are exactly those of a size plan
 *                 (mscomp_amd_plan_create_size) with the same offset, length and limit -- LZNT1's need = length + 1 for a stream that ends in
 *                 the End_of_buffer header included.
 *   Units that fail the checks: a unit gets MSCOMP_ARG_ERROR, d_out_len = d_need = 0, and nothing is read for it, if its in_len is above
 *                 0xFFFFF000, or the running total of in_len up to and including it is above in_total_max (running totals stay at
 *                 2^64 - 1 once they get there). The other units are unaffected. Offsets are the caller's responsibility.
 *   Execution:    mscomp_amd_plan_execute_size_dev is asynchronous on the ctx stream; it allocates nothing, does not synchronize and reads nothing
 *                 back to the host. Its launches are kernels only (d_need too is written by a kernel). It may run while the ctx stream is being
 *                 captured into a graph (it then enqueues plain launches). Outside capture it replays a graph of its own from its second
 *                 execution on, captured again whenever one of its pointers changes. MSCOMP_ARG_ERROR for a null plan or array (d_in may be
 *                 null when in_total_max is 0, d_limit always).
 *   Plan kinds:   mscomp_amd_plan_execute, mscomp_amd_plan_execute_size and mscomp_amd_plan_execute_dev return MSCOMP_ARG_ERROR for a size dev
 *                 plan, mscomp_amd_plan_execute_size_dev for any other plan, without enqueueing anything. mscomp_amd_plan_destroy frees it.
 *   Creation:     the argument checks of mscomp_amd_plan_create_decompress_dev (MSCOMP_ARG_ERROR for a null ctx or plan pointer, a bad format,
 *                 n_units above 0x7FFFFFF0); MSCOMP_MEM_ERROR when the bounds exceed what the scratch can address or the scratch cannot be
 *                 reserved. The scratch is reserved for (n_units, in_total_max), once, and never grows.
 * As decompress dev plans, size dev plans take only the paths that need no tables chosen on the host (DESIGN_DECODERS.md): an Xpress stream of
 * 512 KiB or more is sized by the one-wave walk instead of by segments -- the same answers, more slowly
 * (mscomp_amd_plan_create_size_dev_ex below builds the segment tables on the device). */
MSCompStatus mscomp_amd_plan_create_size_dev(mscomp_amd_ctx* ctx, MSCompFormat format, size_t n_units,
                                             uint64_t in_total_max, mscomp_amd_plan** plan);
MSCompStatus mscomp_amd_plan_execute_size_dev(mscomp_amd_plan* plan, const uint8_t* d_in,
                                              const uint64_t* d_in_off, const uint64_t* d_in_len, const uint64_t* d_limit,
                                              uint64_t* d_out_len, uint64_t* d_need, int32_t* d_status);

/* Dev plans for batches with large units. The two creators above leave the optional paths of a host plan out, because a host plan chooses
 * them from its host tables. With MSCOMP_AMD_DEV_LARGE_UNITS the plan builds those paths' tables on the device too, at every execution, by
 * the arithmetic a host plan uses (csrc/common.h), and takes the host plan's decisions for the same per-unit values:
 *   Xpress, decompress and size plans:  streams of 512 KiB input or more are walked by segments;
 *   both Xpress formats, decompress:    units with room for 1 MiB or more get their bytes from all CUs -- for no unit of the batch when one
 *                                       has room for 0xFFFFFF00 bytes or more, or when the stage does not pay for the batch's capacities;
 *   Xpress+Huffman, decompress:         units with room for more than 64 KiB keep their candidates' tokens in scratch (no second walk).
 * flags = 0 is exactly the creator without _ex; any other bit is MSCOMP_ARG_ERROR; LZNT1 accepts the flag and is unchanged by it. The
 * other creation checks and statuses, execution (mscomp_amd_plan_execute_dev / _execute_size_dev, same arguments), per-unit results,
 * rejects and plan kinds are those of the creators above: asynchronous, nothing allocated, nothing read back, kernels only, a launch
 * sequence fixed by the creation bounds. A rejected unit is an empty unit and takes no path.
 * The flag is opt-in for what it costs whether or not a batch holds a large unit:
 *   scratch    the all-CU stage reserves 4 bytes per byte of out_total_max (+ 64 per possible unit) when the plan is created, the token
 *              scratch 256 KiB per possible candidate of the units it could take. Both are optional: above MSCOMP_AMD_LZG_MAX_MB /
 *              MSCOMP_AMD_XHC_SCR_MAX_MB or half of the free device memory, or not to be had, the path is off for the life of the plan --
 *              creation succeeds, and the block-per-unit kernel / the second walk take the units, as in a host plan;
 *   launches   the stages' launches are in the sequence every time (Xpress: the segment walk with its 8 redo rounds; both: the path pass,
 *              the directory, the expansion and 33 pointer passes of the all-CU stage), gridded by the bounds; their blocks return at once
 *              when the batch has no unit for them. Measured on 3 239 units of 64 KiB (1 x MI355X, DESIGN_DECODERS.md, "Plans with device
 *              tables"): + 8.5 % for Xpress (0.24 ms), + 2.2 % for Xpress+Huffman against the plan without the flag; one 27 MB Xpress
 *              stream: 7.07 ms with the flag, 659 ms without, 6.98 ms for a host plan. */
#define MSCOMP_AMD_DEV_LARGE_UNITS 1u
MSCompStatus mscomp_amd_plan_create_decompress_dev_ex(mscomp_amd_ctx* ctx, MSCompFormat format, size_t n_units,
                                                      uint64_t in_total_max, uint64_t out_total_max, uint32_t flags, mscomp_amd_plan** plan);
MSCompStatus mscomp_amd_plan_create_size_dev_ex(mscomp_amd_ctx* ctx, MSCompFormat format, size_t n_units,
                                                uint64_t in_total_max, uint32_t flags, mscomp_amd_plan** plan);

/* Compress plans with device tables: the compressing half of the same pipeline. Created once from bounds and executed with
 * mscomp_amd_plan_execute_dev (the same nine arguments) on unit tables that GPU work has written -- the d_out_len of a decompress dev plan, say,
 * with the offsets of mscomp_amd_plan_layout_dev. n_units is fixed when the plan is created. Two caps apply to the units:
 *   in_len of one unit <= in_unit_max
 *   total in_len       <= in_total_max   (summed in unit order)
 * Compression scratch depends on the input alone: there is no output bound.
 *   Per-unit results: for every unit that passes the checks below, d_status[i] and d_out_len[i], and the bytes on MSCOMP_OK, are exactly those
 *                 of a compress plan (mscomp_amd_plan_create) with the same values: MSCOMP_BUF_ERROR for a short capacity, LZNT1's uncounted
 *                 00 00 when two bytes of room are left.
 *   Units that fail the checks: a unit gets MSCOMP_ARG_ERROR, d_out_len = 0, and nothing is read or written for it, if its in_len is above
 *                 in_unit_max, or the running total of in_len up to and including it is above in_total_max. The other units are unaffected.
 *                 Offsets and capacities are the caller's responsibility.
 *   Execution:    as for decompress dev plans (asynchronous, no allocation, no synchronisation, nothing read back; plain launches while the ctx
 *                 stream is being captured, a graph of its own from the second execution on otherwise). MSCOMP_ARG_ERROR for a null plan or
 *                 array (d_in may be null when in_total_max is 0; d_out is needed whenever n_units > 0).
 *   Plan kinds:   mscomp_amd_plan_execute and mscomp_amd_plan_execute_size return MSCOMP_ARG_ERROR for it without enqueueing anything.
 *   Creation:     the argument checks of mscomp_amd_plan_create (MSCOMP_ARG_ERROR for a null ctx or plan pointer, a bad format, n_units above
 *                 0x7FFFFFF0), and MSCOMP_ARG_ERROR for in_unit_max 0 or above 0xFFFFF000; MSCOMP_MEM_ERROR when the bounds exceed what the
 *                 scratch can address or the scratch cannot be reserved. The scratch is reserved for the bounds, once.
 *   Fixed at creation, as for host plans: the LZNT1 dictionary flavour (mscomp_amd_ctx_set_lznt1_sa_dict), and the Xpress match finder, chosen
 *                 by in_unit_max as a host plan chooses it by its largest unit. */
MSCompStatus mscomp_amd_plan_create_compress_dev(mscomp_amd_ctx* ctx, MSCompFormat format, size_t n_units,
                                                 uint64_t in_total_max, uint64_t in_unit_max, mscomp_amd_plan** plan);
/* The device form of mscomp_amd_plan_layout: d_out_cap[i] = the largest output of one unit of d_in_len[i] bytes (that of
 * mscomp_amd_plan_layout; d_out_cap may be NULL), d_out_off[0..n_units] = the exclusive running sum of the capacities rounded up to `align`
 * (0 counts as 1), d_out_off[n_units] = total, saturating as mscomp_amd_layout_dev. One launch on the ctx stream; allocates nothing.
 * MSCOMP_ARG_ERROR for a bad format, a null ctx or d_out_off, or a null d_in_len with n_units > 0. */
MSCompStatus mscomp_amd_plan_layout_dev(mscomp_amd_ctx* ctx, MSCompFormat format, size_t n_units, const uint64_t* d_in_len,
                                        uint64_t align, uint64_t* d_out_off, uint64_t* d_out_cap);

/* Batch helpers.
 * Capacity planning: out_cap[i] = what one ms_compress call needs at most for in_len[i] bytes (ms_max_compressed_size, + 2 for the LZNT1
 * End_of_buffer), out_off[i] = running offset rounded up to `align`; returns the total size of the output buffer ((uint64_t)-1: bad format).
 * Either output array may be NULL.
 * Compaction: the outputs of a batch sit at out_off[i] with gaps up to their capacities; this packs them back to back, in unit order,
 * into d_packed and writes the n_units + 1 offsets (uint64, device memory) to d_packed_off; out_off / out_cap are the host arrays given to
 * the plan, d_out_len the device array plan_execute filled (units with a status other than MSCOMP_OK have length 0). Enqueued on the ctx
 * stream after one small synchronous table upload. */
uint64_t     mscomp_amd_plan_layout(MSCompFormat format, size_t n_units, const uint64_t* in_len, uint64_t align, uint64_t* out_off, uint64_t* out_cap);
MSCompStatus mscomp_amd_compact_batch(mscomp_amd_ctx* ctx, size_t n_units, const uint8_t* d_out, const uint64_t* out_off, const uint64_t* out_cap,
                                      const uint64_t* d_out_len, uint8_t* d_packed, uint64_t* d_packed_off);

/* Compaction with device tables: packs n_units byte ranges of d_src back to back into d_packed without the host knowing where they are or
 * how long -- the outputs of a compress dev plan, say (d_src_off = the offsets of mscomp_amd_plan_layout_dev, d_len = the plan's d_out_len;
 * a unit that is not MSCOMP_OK has length 0 there). d_src_off, d_len: device arrays of n_units uint64; d_packed_off: n_units + 1.
 *   d_packed_off[0..n_units] = the exclusive running sum of d_len[i] rounded up to `align` (0 counts as 1), d_packed_off[n_units] = total,
 *                 a sum beyond 2^64 - 1 stays there: exactly what mscomp_amd_layout_dev(ctx, n_units, d_len, align, ...) writes.
 *   d_packed:     the d_len[i] bytes at d_src + d_src_off[i] go to d_packed + d_packed_off[i]; the padding between two units is written as
 *                 zero, so the packed bytes [0, total) are reproducible. Source addresses may have any alignment. d_packed must not overlap
 *                 the source ranges.
 *   packed_cap:   nothing is written at or behind d_packed + packed_cap. A unit whose end d_packed_off[i] + d_len[i] lies beyond packed_cap is
 *                 not copied at all (no partial unit); the caller learns of it from d_packed_off[n_units] > packed_cap, on the device.
 * Asynchronous on the ctx stream: two kernel launches whose geometry depends on n_units and the device only; no host table, no upload, no
 * synchronisation, no allocation, no scratch -- it may run while the ctx stream is being captured into a graph. MSCOMP_ARG_ERROR for a null
 * ctx or d_packed_off, for a null d_src, d_src_off, d_len or d_packed with n_units > 0, and for n_units above 0x7FFFFFF0. n_units = 0 writes
 * d_packed_off[0] = 0 (from a kernel). */
MSCompStatus mscomp_amd_compact_dev(mscomp_amd_ctx* ctx, size_t n_units, const uint8_t* d_src, const uint64_t* d_src_off,
                                    const uint64_t* d_len, uint64_t align, uint8_t* d_packed, uint64_t packed_cap, uint64_t* d_packed_off);

/* CRC-32 of a batch in HBM, from device tables: d_crc[i] = the CRC-32 of zlib, PNG and Ethernet (reflected polynomial 0xEDB88320, initial value
 * and final XOR 0xFFFFFFFF; 0 for an empty unit, 0xCBF43926 for "123456789") of the d_in_len[i] bytes at d_in + d_in_off[i]. Created once from
 * bounds, as the other plans with device tables; n_units is fixed when the plan is created. Units may have any alignment, may overlap and may
 * come in any order: they are only read. d_in_off, d_in_len: device arrays of n_units uint64; d_crc: n_units uint32; d_status: n_units int32.
 *   Units that fail the check: a unit whose running total of d_in_len, up to and including it, exceeds in_total_max gets MSCOMP_ARG_ERROR and
 *                 d_crc = 0, and nothing is read for it. Every other unit gets MSCOMP_OK. (Running totals stay at 2^64 - 1 once they get there.)
 *   Execution:    asynchronous on the ctx stream: three kernel launches whose geometry is fixed by n_units and the device -- one block that
 *                 checks and sums the lengths, a thread per unit that seeds d_crc, and a grid of 4 blocks per CU that cuts the batch's bytes into equal slices, so that one unit of
 *                 50 MB is spread over every CU and 100 000 units of 40 bytes over the same grid; the parts of a unit are folded into d_crc[i]
 *                 with atomic XORs, in any order, to the same bits. No memset or copy node, no allocation, no synchronisation, nothing read
 *                 back. Plain launches while the ctx stream is being captured; otherwise a graph of its own from the second execution on.
 *                 MSCOMP_ARG_ERROR for a null plan or array (d_in may be null when in_total_max is 0).
 *   Plan kinds:   mscomp_amd_plan_execute, _execute_dev, _execute_size and _execute_size_dev return MSCOMP_ARG_ERROR for a CRC plan,
 *                 mscomp_amd_plan_execute_crc_dev for any other plan, without enqueueing anything. mscomp_amd_plan_destroy frees it.
 *   Creation:     MSCOMP_ARG_ERROR for a null ctx or plan pointer, n_units above 0x7FFFFFF0, or in_total_max of 2^50 or more (a unit's length
 *                 times 8 is an exponent of 53 bits at most; a container's in_total_max is below 2^50 by its own checks); MSCOMP_MEM_ERROR when the tables (16 bytes per
 *                 unit) cannot be reserved. They are reserved here, once.
 * The kernel's sizes, for tests and for callers who lay out their units: a wave takes MSCOMP_AMD_CRC_ROW_BYTES per step (64 lanes with a run of
 * 64 bytes each), in rows that end at the last 16-byte boundary of a unit's part; a slice is a multiple of MSCOMP_AMD_CRC_SLICE_BYTES. */
#define MSCOMP_AMD_CRC_ROW_BYTES   4096u
#define MSCOMP_AMD_CRC_SLICE_BYTES 16384u
MSCompStatus mscomp_amd_plan_create_crc_dev(mscomp_amd_ctx* ctx, size_t n_units, uint64_t in_total_max, mscomp_amd_plan** plan);
MSCompStatus mscomp_amd_plan_execute_crc_dev(mscomp_amd_plan* plan, const uint8_t* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len,
                                             uint32_t* d_crc, int32_t* d_status);

/* Block containers: the shape in which these codecs are deployed (WIM resources, WOF-compressed files, NTFS compression units). A resource
 * (one caller buffer) is cut into blocks of block_size bytes, every block is compressed on its own, a block that does not shrink is stored
 * raw, the stored blocks are packed back to back, and a table of offsets says where each one is -- so a reader who wants a range of a
 * resource decodes only the blocks that hold it. One call handles a batch of n_res resources; all tables are device arrays, written and
 * read by kernels on the ctx stream. (A block is the container's piece; the codecs' own 4 KiB / 64 KiB chunks keep their name.)
 * The payloads are this library's ms_compress bytes and the tables plain uint64 arrays beside the data: byte compatibility with a particular
 * WIM, WOF or NTFS writer is not claimed, and serialising to one of those on-disk headers is the caller's.
 *   Creation:     block_size = B is a power of two from 4096 to 524288; flags must be 0. n_blocks_max = n_res + in_total_max / B
 *                 (mscomp_amd_blocks_bound) bounds the blocks of any batch whose lengths sum to at most in_total_max. All scratch is
 *                 reserved here, once, and never grows: a compress and a decompress dev plan for n_blocks_max units (of at most B bytes;
 *                 within in_total_max bytes in and out), the staging area of the compressed blocks -- 1 byte per byte of in_total_max + 16
 *                 per resource --, and 68 bytes of tables per possible block + 28 per resource. MSCOMP_ARG_ERROR for a null ctx or bk, a bad
 *                 format, a bad block_size, non-zero flags, n_res above 0x7FFFFFF0; MSCOMP_MEM_ERROR when n_blocks_max exceeds 0x7FFFFFF0 or
 *                 the scratch cannot be reserved. The LZNT1 dictionary flavour is fixed here, as for a compress dev plan.
 *   Compress:     d_res_off, d_res_len, d_status: n_res entries; d_block_first: n_res + 1; d_block_off: n_blocks_max + 1.
 *                 Resource r is the d_res_len[r] bytes at d_in + d_res_off[r]. It is rejected -- MSCOMP_ARG_ERROR, no blocks, nothing read --
 *                 when the running total of d_res_len up to and including it exceeds in_total_max. An accepted resource has
 *                 ceil(len / B) blocks (an empty one none), block j being its bytes [j B, min(len, (j + 1) B)).
 *                 d_block_first = the exclusive running count of blocks, d_block_first[n_res] = their number nb.
 *                 Stored form of a block: c = the bytes one ms_compress(format, block) call writes with ample capacity (the counted length:
 *                 LZNT1's uncounted trailing 00 00 is not stored) when len(c) < len(block), the raw block otherwise -- never longer than
 *                 its data. d_block_off[0..nb] = the exclusive running sum of the stored lengths, without padding; the entries
 *                 nb + 1 .. n_blocks_max repeat d_block_off[nb]. d_packed[0 .. d_block_off[nb]) holds the stored blocks in order.
 *                 Nothing is written at or behind d_packed + packed_cap: a block that would end beyond it is not written at all and its
 *                 resource gets MSCOMP_BUF_ERROR, the tables still holding the full layout (the rule of mscomp_amd_compact_dev). Every
 *                 other resource gets MSCOMP_OK.
 *   Decompress:   d_range = NULL means every block; otherwise 2 n_res uint64, per resource a first block f and a count c, both clipped to the
 *                 resource's block count. want = min(len, (f + c) B) - f B bytes (0 for c = 0) go to d_out + d_out_off[r]. Per resource, in
 *                 this order, each leaving the other resources alone:
 *                   1. MSCOMP_ARG_ERROR, nothing read or written: the running total of d_res_len up to and including it exceeds
 *                      in_total_max, or d_block_first[r] or d_block_first[r + 1] exceeds n_blocks_max;
 *                   2. MSCOMP_DATA_ERROR: d_block_first[r + 1] - d_block_first[r] is not ceil(len / B);
 *                   3. MSCOMP_BUF_ERROR, nothing written: want > d_out_cap[r];
 *                   4. every block in range, by its stored length s = off[j + 1] - off[j] and its data length e: s = e is copied;
 *                      0 < s < e is decoded exactly as ms_decompress with capacity e, and must give MSCOMP_OK and e bytes; anything
 *                      else -- s > e, s = 0, a decreasing table, an end beyond packed_len, another decoder status or length -- is
 *                      MSCOMP_DATA_ERROR for the resource. A block that fails a table check is never read.
 *                 MSCOMP_OK: d_out_len[r] = want and the bytes are that slice of the resource. Otherwise d_out_len[r] = 0, the bytes
 *                 inside the resource's capacity are unspecified and nothing is written outside it. Blocks outside the range are not
 *                 decoded and cost nothing but their share of the fixed launches.
 *   Execution:    as mscomp_amd_plan_execute_dev: asynchronous on the ctx stream, kernels only (no memset or copy node), no allocation, no
 *                 synchronisation, nothing read back, a launch sequence fixed by the creation bounds, all on the one stream. Legal while
 *                 the caller captures the ctx stream, the first execution included (plain launches then); outside capture each of the two
 *                 calls replays a graph of its own from its second execution on, captured again when an argument changes.
 *                 MSCOMP_ARG_ERROR for a null bk or a null required array (d_in, d_packed and d_out may be null when in_total_max is 0,
 *                 d_range always).
 *   Checksums:    the decoders check structure only, and a raw block is not checked at all: a flipped byte can decode to MSCOMP_OK. The two
 *                 calls below keep a CRC-32 (as mscomp_amd_plan_execute_crc_dev's) per block beside the container and hold decoded data to it.
 *                 The checksum is over the DATA, not the stored form: re-encoding a container with another codec or with another block size
 *                 keeps every resource CRC, and with the same block size every block CRC. They use the container's tables and 4 bytes more
 *                 per possible block, reserved at creation.
 *                 Crc: d_data, d_res_off, d_res_len as compress's input -- run it on that input before compress, or on anything else of the
 *                 same lengths. Resources are accepted and rejected as compress does it (MSCOMP_ARG_ERROR, no blocks, nothing read), blocks
 *                 numbered by the same running count: d_block_crc[j] (n_blocks_max entries) belongs to the block compress puts at
 *                 d_block_off[j]; the entries at or behind the real count are 0. d_res_crc (n_res entries, may be NULL): the CRC-32 of every
 *                 whole resource, 0 for a rejected one -- from the same pass over the bytes, every part of a block being folded in a second
 *                 time at its distance to the resource's end. d_status (n_res): MSCOMP_OK or MSCOMP_ARG_ERROR.
 *                 Check: after decompress, with the same d_res_len, d_block_first, d_range and d_out_off, and decompress's d_out_len and
 *                 d_status (in and out). A resource whose d_status is not MSCOMP_OK on entry is left alone and nothing of it is read. A
 *                 resource that is MSCOMP_OK is held to checks 1 and 2 above (the same statuses, d_out_len = 0); then block k of its clipped
 *                 range is read at d_out + d_out_off[r] + k B and its CRC-32 compared with d_block_crc[d_block_first[r] + f + k]. Any
 *                 mismatch: MSCOMP_DATA_ERROR, d_out_len[r] = 0. A resource that passes is not written, nor is any other resource.
 *                 Both run as the other two calls do (a fixed launch sequence of kernels; legal inside a capture from the first execution;
 *                 a graph of their own otherwise). MSCOMP_ARG_ERROR for a null bk or a null required array (d_data / d_out may be null when
 *                 in_total_max is 0; d_res_crc and d_range always). */
typedef struct mscomp_amd_blocks mscomp_amd_blocks;
MSCompStatus mscomp_amd_blocks_create(mscomp_amd_ctx* ctx, MSCompFormat format, uint32_t block_size, size_t n_res, uint64_t in_total_max,
                                      uint32_t flags, mscomp_amd_blocks** bk);
void         mscomp_amd_blocks_destroy(mscomp_amd_blocks* bk);
uint64_t     mscomp_amd_blocks_bound(const mscomp_amd_blocks* bk);   /* n_blocks_max; 0 for NULL */
MSCompStatus mscomp_amd_blocks_compress(mscomp_amd_blocks* bk, const uint8_t* d_in, const uint64_t* d_res_off, const uint64_t* d_res_len,
                                        uint8_t* d_packed, uint64_t packed_cap,
                                        uint64_t* d_block_first, uint64_t* d_block_off, int32_t* d_status);
MSCompStatus mscomp_amd_blocks_decompress(mscomp_amd_blocks* bk, const uint8_t* d_packed, uint64_t packed_len,
                                          const uint64_t* d_block_first, const uint64_t* d_block_off, const uint64_t* d_res_len,
                                          const uint64_t* d_range,
                                          uint8_t* d_out, const uint64_t* d_out_off, const uint64_t* d_out_cap,
                                          uint64_t* d_out_len, int32_t* d_status);
MSCompStatus mscomp_amd_blocks_crc(mscomp_amd_blocks* bk, const uint8_t* d_data, const uint64_t* d_res_off, const uint64_t* d_res_len,
                                   uint32_t* d_block_crc /* n_blocks_max */, uint32_t* d_res_crc /* n_res, may be NULL */, int32_t* d_status);
MSCompStatus mscomp_amd_blocks_check(mscomp_amd_blocks* bk, const uint8_t* d_out, const uint64_t* d_out_off, const uint64_t* d_res_len,
                                     const uint64_t* d_block_first, const uint64_t* d_range, const uint32_t* d_block_crc,
                                     uint64_t* d_out_len, int32_t* d_status /* in and out */);

/* Salvage: the container's fifth call. Decompress and check answer per resource -- one flipped byte in one block of a 50 MB resource is
 * MSCOMP_DATA_ERROR, d_out_len = 0 and unspecified bytes for all of it, and nothing says which block is bad. Salvage decodes everything
 * that can be decoded and gives a verdict per BLOCK, so that damage costs the damaged blocks and nothing else, and so that a second copy of
 * the container need be looked at only where this one is bad (d_only).
 *   Creation:     none of its own: any container serves (mscomp_amd_blocks_create).
 *   Scratch:      none of its own either. Every column of the container's tables is a temporary of one call, and the existing ones
 *                 suffice: 68 bytes per possible block + 28 per resource, as stated above.
 *   Sources:      d_packed, packed_len, d_block_first, d_block_off, d_res_len, d_out, d_out_off, d_out_cap as decompress takes them;
 *                 d_block_crc (n_blocks_max entries, may be NULL) as check takes it; d_only (n_blocks_max entries, may be NULL): a mask over
 *                 the container's rows -- in practice the d_verdict array another salvage wrote for a copy of the same shape.
 *   Notation:     L = d_res_len[r]; row j = d_block_first[r] + k is block k of resource r, with data length e = min(B, L - k B).
 *   Rules:        in this order, each resource leaving the others alone:
 *                   1. decompress's per-resource checks 1-3 with d_range = NULL (bounds: MSCOMP_ARG_ERROR; block count: MSCOMP_DATA_ERROR;
 *                      L > d_out_cap[r]: MSCOMP_BUF_ERROR). Such a resource has d_out_len = 0 and d_bad = 0, every one of its rows that can
 *                      be named is SKIPPED, and nothing of it is read or written.
 *                   2. Row j of an accepted resource is judged unless d_only is given and d_only[j] == MSCOMP_AMD_BLOCK_GOOD. An unjudged
 *                      row is SKIPPED: nothing of it is read, and its bytes in d_out are not touched.
 *                   3. A judged row's verdict is the first that applies of TABLE (decompress's step 4 refuses the row by its table
 *                      entries: a decreasing table, an end beyond packed_len, s > e, s = 0; the row is never read), DECODE (the decoder's
 *                      status is not MSCOMP_OK, or its length is not e) and CRC (only with d_block_crc: the e bytes, copied or decoded,
 *                      do not have the CRC-32 d_block_crc[j]); else GOOD.
 *                   4. The e bytes of a GOOD row at d_out + d_out_off[r] + k B are the block's data. The e bytes of a judged bad row are
 *                      ZERO: a failed decoder may have written inside its capacity, so the row is zero-filled after the verdict. Nothing
 *                      is written outside [d_out_off[r], d_out_off[r] + L).
 *                   5. Per accepted resource d_out_len[r] = L WHATEVER ITS ROWS SAY -- this is the point of the call, and it differs from
 *                      decompress, where a bad block leaves d_out_len[r] = 0 --, d_bad[r] = its judged bad rows, and d_status[r] is
 *                      MSCOMP_OK when d_bad[r] is 0, MSCOMP_DATA_ERROR otherwise.
 *                   6. d_verdict: all n_blocks_max entries are written; those at and behind d_block_first[n_res], and every entry not
 *                      named above, are SKIPPED. (Two accepted resources can name the same row only when d_block_first is damaged; the
 *                      row then holds the verdict of either.)
 *                   7. d_count[0..3] = rows judged, rows bad, data bytes zero-filled, accepted resources with d_bad > 0: the same from
 *                      run to run.
 *   Consequence:  where d_status[r] is MSCOMP_OK and d_only is NULL, the L bytes are what decompress + check write, and salvage replaces
 *                 the two. The d_verdict arrays of a container and its copies are what mscomp_amd_deduper_repair takes.
 *   Checksums:    as check's: over the data, read back from d_out. Without d_block_crc no row is CRC, and a raw block is never bad but
 *                 by its table entries. A damaged CRC word and damaged data give the same verdict.
 *   Execution:    as the container's other calls: a launch sequence fixed by the creation bounds -- the decompress table pass with the mask,
 *                 the inner decompress plan, the raw copy, a units pass, the CRC passes (left out, as a launch-time decision, when
 *                 d_block_crc is NULL), the verdicts, the zero-fill, the fold --, kernels only, vector stores only, no memset or copy
 *                 node, nothing allocated, nothing read back; legal inside a capture from the first execution, a graph of its own
 *                 otherwise. MSCOMP_ARG_ERROR for a null bk or a null required array (d_packed and d_out may be null when in_total_max
 *                 is 0, d_block_crc and d_only always). With n_res = 0 the call returns MSCOMP_OK and writes nothing, d_count included.
 *   Left out:     telling a damaged CRC word from damaged data; byte-granular salvage inside a block (a bad row is all zeros); repairing
 *                 the d_block_first of a refused resource; fusing salvage, repair and splice in one call. */
#define MSCOMP_AMD_BLOCK_GOOD    0u
#define MSCOMP_AMD_BLOCK_TABLE   1u   /* failed a table check of decompress step 4; never read */
#define MSCOMP_AMD_BLOCK_DECODE  2u   /* decoder status other than MSCOMP_OK, or a length other than e */
#define MSCOMP_AMD_BLOCK_CRC     3u   /* copied or decoded to e bytes, CRC-32 differs from d_block_crc[row] */
#define MSCOMP_AMD_BLOCK_SKIPPED 4u   /* not judged: nothing read, nothing written */
MSCompStatus mscomp_amd_blocks_salvage(mscomp_amd_blocks* bk, const uint8_t* d_packed, uint64_t packed_len,
                                       const uint64_t* d_block_first, const uint64_t* d_block_off, const uint64_t* d_res_len,
                                       const uint32_t* d_block_crc /* may be NULL */, const uint32_t* d_only /* n_blocks_max, may be NULL */,
                                       uint8_t* d_out, const uint64_t* d_out_off, const uint64_t* d_out_cap,
                                       uint64_t* d_out_len, uint32_t* d_bad /* n_res */, uint32_t* d_verdict /* n_blocks_max */,
                                       uint64_t* d_count /* 4 */, int32_t* d_status);

/* Block readers: byte-range reads from a block container, batched. A request q = (r, off, len) asks for the bytes [off, off + len) of
 * resource r, as pread does; one call serves n_req of them, scattered over any resources in any order, and writes exactly those bytes. The
 * reader is an object of its own, sized by what one call READS: it needs no mscomp_amd_blocks object, only the tables a container wrote and
 * the packed bytes. A block that several requests touch is decoded once, and checked once.
 *   Creation:     block_size = B and format as the container's; flags must be 0. n_res resources, whose tables are d_block_first (n_res + 1
 *                 entries), d_block_off (n_blocks_table + 1: the container's n_blocks_max + 1) and d_res_len (n_res). n_req requests per
 *                 call, fixed here. blocks_max bounds the blocks one call may touch (rule 5). All scratch is reserved here, once, and never
 *                 grows: a block cache of blocks_max B bytes, one decompress dev plan for blocks_max units within blocks_max B bytes in and
 *                 out, and the reader's tables: 88 bytes per unit of blocks_max, 44 per request, 4 per entry of the block table.
 *                 MSCOMP_ARG_ERROR for a null ctx or rd, a bad format, a bad block_size, non-zero flags, or any of n_res, n_blocks_table,
 *                 n_req, blocks_max above 0x7FFFFFF0; MSCOMP_MEM_ERROR when the scratch cannot be reserved, or blocks_max B bytes are more
 *                 than a decompress dev plan can address. Every check comes before the context is used; *rd is cleared on failure.
 *   Read:         d_req = 3 n_req uint64: resource, offset, length. d_out_off, d_out_cap, d_out_len, d_status: n_req entries. With
 *                 L = d_res_len[r], per request, in this order, each leaving every other request alone:
 *                   1. MSCOMP_ARG_ERROR, nothing read: r >= n_res, or d_block_first[r] or d_block_first[r + 1] exceeds n_blocks_table;
 *                   2. MSCOMP_DATA_ERROR: d_block_first[r + 1] - d_block_first[r] is not ceil(L / B);
 *                   3. the range is clipped: off' = min(off, L), want = min(len, L - off') -- no sum of off and len is formed, a len of
 *                      2^64 - 1 means "to the end". want = 0 is MSCOMP_OK with no blocks;
 *                   4. MSCOMP_BUF_ERROR: want > d_out_cap[q];
 *                   5. the budget: the request covers cnt = the blocks off' / B .. (off' + want - 1) / B of the resource. The running
 *                      total of cnt over all requests that passed 1-4, in request order and including this one, must not exceed
 *                      blocks_max; otherwise MSCOMP_ARG_ERROR (the dev plans' rule for bounds). The total counts covering blocks BEFORE
 *                      any sharing: two requests into one block count 2. So admission is a running sum that does not depend on which
 *                      requests share blocks, and a caller who sizes blocks_max by the sum of its requests' blocks is never refused;
 *                   6. every covering block passes the container's table checks (mscomp_amd_blocks_decompress, step 4; a block that fails
 *                      one is never read): s = e is raw and read where it lies, 0 < s < e is decoded exactly as ms_decompress with capacity
 *                      e and must give MSCOMP_OK and e bytes; with d_block_crc non-null (the array mscomp_amd_blocks_crc wrote), the CRC-32
 *                      of the whole block, decoded or raw, must equal d_block_crc[block]. Any failure is MSCOMP_DATA_ERROR for every
 *                      request that covers that block, and for no other.
 *                 MSCOMP_OK: d_out_len[q] = want and exactly the bytes [off', off' + want) of the resource lie at d_out + d_out_off[q], at
 *                 any alignment; nothing outside these want bytes is written. Otherwise d_out_len[q] = 0 and nothing is written for the
 *                 request at all: the verdicts are folded before the bytes move. Requests may repeat and overlap on the input side;
 *                 overlap on the output side is the caller's responsibility.
 *   Sharing:      a unit is one (request, covering block) pair of an admitted request; the lowest unit that covers a block owns it. Only
 *                 owners are decoded (into cache slot `unit`) or, raw, read in d_packed, and only owners' blocks are checksummed; every
 *                 unit gathers from its owner. mscomp_amd_reader_counts gives, for the last execution, out[0] = units, out[1] = distinct
 *                 blocks, out[2] = those that were decoded rather than raw (a block that failed a table check is neither). It
 *                 synchronises the stream, works without MSCOMP_AMD_TEST_HOOKS and returns -1 on error, 0 otherwise.
 *   Execution:    as the container's calls: asynchronous on the ctx stream, kernels only (no memset or copy node), no allocation, no
 *                 synchronisation, nothing read back, a launch sequence fixed by the creation bounds. Legal while the caller captures the
 *                 ctx stream, the first execution included; outside capture the call replays a graph of its own from its second execution
 *                 on, captured again when an argument changes. MSCOMP_ARG_ERROR for a null rd or a null required array (d_packed and d_out
 *                 may be null when blocks_max is 0, d_res_len when n_res is 0, the request arrays when n_req is 0, d_block_crc always).
 *                 n_req = 0 returns MSCOMP_OK. */
typedef struct mscomp_amd_reader mscomp_amd_reader;
MSCompStatus mscomp_amd_reader_create(mscomp_amd_ctx* ctx, MSCompFormat format, uint32_t block_size, size_t n_res, uint64_t n_blocks_table,
                                      size_t n_req, uint64_t blocks_max, uint32_t flags, mscomp_amd_reader** rd);
void         mscomp_amd_reader_destroy(mscomp_amd_reader* rd);
MSCompStatus mscomp_amd_reader_read(mscomp_amd_reader* rd, const uint8_t* d_packed, uint64_t packed_len,
                                    const uint64_t* d_block_first, const uint64_t* d_block_off, const uint64_t* d_res_len,
                                    const uint32_t* d_block_crc /* may be NULL */,
                                    const uint64_t* d_req /* 3 n_req: resource, offset, length */,
                                    uint8_t* d_out, const uint64_t* d_out_off, const uint64_t* d_out_cap,
                                    uint64_t* d_out_len, int32_t* d_status);
int          mscomp_amd_reader_counts(mscomp_amd_reader* rd, uint32_t out[3]);

/* Block writers: byte-range writes into a block container, batched and out of place. A request q = (r, off, len) overwrites the bytes
 * [off, off + len) of resource r, as pwrite does within a file's length; one call applies n_req of them and writes a NEW container -- packed
 * bytes, offset table and, when the old one has them, block checksums -- in which only the blocks the writes touched were decoded, patched
 * and encoded again, and every other block is carried over as it was stored. A writer is an object of its own, sized by what one call
 * WRITES; like a reader it needs only the tables a container wrote and the packed bytes. A write never changes a resource's length.
 *   Creation:     exactly as mscomp_amd_reader_create: the same arguments, the same checks in the same order before the context is used
 *                 (MSCOMP_ARG_ERROR; MSCOMP_MEM_ERROR where blocks_max B bytes are more than a dev plan can address), flags 0, *wr cleared
 *                 on failure. All scratch is reserved here, once, and never grows: a block cache of blocks_max B bytes, a staging area of
 *                 blocks_max B bytes, a decompress and a compress dev plan for blocks_max units within blocks_max B bytes each, and the
 *                 writer's tables: 96 bytes per unit of blocks_max, 44 per request, 16 per entry of the block table and -- for
 *                 mscomp_amd_writer_resize -- 12 per resource + 8. The LZNT1 dictionary flavour is fixed here, as for
 *                 mscomp_amd_blocks_create.
 *   Out of place: the old container is d_packed (packed_len valid bytes), d_block_off (n_blocks_table + 1) and d_block_crc (n_blocks_table,
 *                 may be NULL); it is only read. The new one goes to d_new_packed (nothing at or behind new_cap), d_new_block_off
 *                 (n_blocks_table + 1) and d_new_block_crc (n_blocks_table; NULL exactly when d_block_crc is), which must not overlap the
 *                 old arrays. d_block_first (n_res + 1) and d_res_len (n_res) serve both. A caller ping-pongs two sets of buffers.
 *   Write:        d_req = 3 n_req uint64: resource, offset, length; the bytes of request q are read at d_src + d_src_off[q], at any
 *                 alignment. d_written, d_status: n_req entries; d_res_status: n_res. The rules, in this order:
 *                   0. the table as a whole: nb = d_block_first[n_res] must not exceed n_blocks_table and d_block_first must not decrease
 *                      anywhere. Otherwise every request and every resource gets MSCOMP_ARG_ERROR, every d_written is 0, d_new_block_off
 *                      and d_new_block_crc are all 0, and nothing else is written;
 *                   1. MSCOMP_ARG_ERROR: r >= n_res (the reader's rule 1);
 *                   2. MSCOMP_DATA_ERROR: d_block_first[r + 1] - d_block_first[r] is not ceil(L / B), L = d_res_len[r];
 *                   3. the range is clipped as the reader clips it: off' = min(off, L), want = min(len, L - off'); no sum of off and len
 *                      is formed. want = 0 is MSCOMP_OK with no blocks. There is no capacity rule: the source is the want bytes;
 *                   4. the budget, the reader's rule 5 unchanged: the running total of covering blocks over the requests that passed 1-3,
 *                      before any sharing, must not exceed blocks_max; otherwise MSCOMP_ARG_ERROR;
 *                   5. every covering block must be readable: it passes the container's table checks, decodes exactly as ms_decompress
 *                      with capacity e to e bytes, and -- with d_block_crc -- has the CRC-32 the table says (the reader's rule 6). Any
 *                      failure is MSCOMP_DATA_ERROR for every request that covers that block, and for no other. A block is decoded and
 *                      checked once, however many requests touch it; in this version also when the requests overwrite all of it;
 *                   6. verdicts before bytes: d_status[q] = MSCOMP_OK and d_written[q] = want only if every rule passed; otherwise
 *                      d_written[q] = 0 and none of the request's bytes are applied to any block;
 *                   7. the data of a touched block is its old data with the MSCOMP_OK requests applied in request order: where two
 *                      requests cover the same byte, the later one wins, whatever order the hardware runs them in;
 *                   8. the new container: a block is dirty when at least one MSCOMP_OK request covers it. A dirty block's stored form is
 *                      the rule of mscomp_amd_blocks_compress on its new data (ms_compress's counted bytes when shorter, the raw block
 *                      otherwise) and its CRC-32 is computed again. A clean block -- one that only failed requests touched included --
 *                      keeps its stored bytes and its checksum verbatim; a clean block whose old entries are not
 *                      d_block_off[j] <= d_block_off[j + 1] <= packed_len was unreadable and gets the stored length 0 (it stays
 *                      unreadable). d_new_block_off[0 .. nb] is the exclusive running sum of the new stored lengths, the entries above nb
 *                      repeat the total; d_new_block_crc is 0 at and above nb; d_new_packed[0 .. total) holds the blocks in order;
 *                   9. capacity, the rule of mscomp_amd_blocks_compress: a block that would end beyond new_cap is not written and its
 *                      resource gets d_res_status = MSCOMP_BUF_ERROR, the tables still hold the full layout; every other resource gets
 *                      MSCOMP_OK. A stored block is never longer than its data, so new_cap = the sum of the data lengths never refuses.
 *                 Consequence: when the old container was written by mscomp_amd_blocks_compress and all its blocks are healthy, the new
 *                 one is byte for byte what mscomp_amd_blocks_compress and mscomp_amd_blocks_crc write for the patched data.
 *                 A write never changes a resource's length: mscomp_amd_writer_resize below does. Resource checksums
 *                 (mscomp_amd_blocks_crc's d_res_crc) are not maintained: mscomp_amd_res_crc_dev derives them from the block checksums.
 *   Counts:       mscomp_amd_writer_counts gives, for the last execution, out[0] = units (as a reader's), out[1] = distinct blocks touched,
 *                 out[2] = blocks encoded again (the dirty ones); all 0 after a refused table. Otherwise as mscomp_amd_reader_counts.
 *   Execution:    as the reader's: asynchronous on the ctx stream, kernels only, no allocation, no synchronisation, nothing read back, a
 *                 launch sequence fixed by the creation bounds; legal inside a caller's capture from the first execution, a graph of its
 *                 own from the second. MSCOMP_ARG_ERROR for a null wr or a null required array (d_src may be null when blocks_max is 0,
 *                 d_packed and d_new_packed when blocks_max and n_blocks_table are 0, d_res_len and d_res_status when n_res is 0, the
 *                 request arrays when n_req is 0), or when exactly one of d_block_crc and d_new_block_crc is null. n_req = 0 is legal and
 *                 copies the container unchanged (unreadable entries become empty ones). */
typedef struct mscomp_amd_writer mscomp_amd_writer;
MSCompStatus mscomp_amd_writer_create(mscomp_amd_ctx* ctx, MSCompFormat format, uint32_t block_size, size_t n_res, uint64_t n_blocks_table,
                                      size_t n_req, uint64_t blocks_max, uint32_t flags, mscomp_amd_writer** wr);
void         mscomp_amd_writer_destroy(mscomp_amd_writer* wr);
MSCompStatus mscomp_amd_writer_write(mscomp_amd_writer* wr, const uint8_t* d_packed, uint64_t packed_len,
                                     const uint64_t* d_block_first, const uint64_t* d_block_off, const uint64_t* d_res_len,
                                     const uint32_t* d_block_crc /* may be NULL */,
                                     const uint64_t* d_req /* 3 n_req: resource, offset, length */,
                                     const uint8_t* d_src, const uint64_t* d_src_off,
                                     uint8_t* d_new_packed, uint64_t new_cap, uint64_t* d_new_block_off /* n_blocks_table + 1 */,
                                     uint32_t* d_new_block_crc /* NULL exactly when d_block_crc is */,
                                     uint64_t* d_written /* n_req */, int32_t* d_status /* n_req */, int32_t* d_res_status /* n_res */);
int          mscomp_amd_writer_counts(mscomp_amd_writer* wr, uint32_t out[3]);

/* Resize: the writer's second call, ftruncate beside pread and pwrite. Every resource r gets the length d_want_len[r]: cut there, or
 * extended with zeros. Out of place as write is: the old container (d_packed, d_block_first, d_block_off, d_res_len, d_block_crc) is only
 * read, and a new one is written -- d_new_packed (nothing at or behind new_cap), d_new_block_first (n_res + 1), d_new_block_off
 * (n_blocks_table + 1), d_new_block_crc (n_blocks_table; NULL exactly when d_block_crc is) and d_new_res_len (n_res) --, which must not
 * overlap the old arrays. Only the block whose data length changes is decoded, and only it and the blocks that did not exist are encoded;
 * every other kept block is carried as it was stored, at its new place in the table. Appending is resize, then write: two passes over the
 * container.
 *   Scratch:      what the writer reserved when it was created: the cache and the staging area (blocks_max B each), both inner dev plans,
 *                 and the table buffer, of which 12 bytes per resource + 8 serve this call alone.
 *   Notation:     B the block size, L = d_res_len[r], W = d_want_len[r], n = d_block_first[r + 1] - d_block_first[r] the old block count,
 *                 n' = W / B + (W % B != 0) the wanted one (no sum is formed that can overflow). For a block k < min(n, n') the old data
 *                 length is e = min(B, L - k B) and the new one e' = min(B, W - k B); the block is CHANGED when e != e' -- at most one per
 *                 resource, k = min(n, n') - 1. The blocks n <= k < n' are FRESH, the blocks k >= n' are dropped. The resource costs
 *                 cnt = (1 if it has a changed block) + max(0, n' - n).
 *   Rules:        in this order:
 *                   0. the table as a whole, the writer's rule 0: d_block_first[n_res] must not exceed n_blocks_table and d_block_first
 *                      must not decrease anywhere. Otherwise every d_res_status is MSCOMP_ARG_ERROR, d_new_block_first, d_new_block_off,
 *                      d_new_block_crc and d_new_res_len are all 0, and nothing else is written;
 *                   1. block count: MSCOMP_DATA_ERROR when n is not ceil(L / B). The resource is carried as it is;
 *                   2. no change: W = L is MSCOMP_OK and costs nothing;
 *                   3. the budget: the running total of cnt over the resources that passed rules 1 and 2, in resource order, including
 *                      this one and including refused ones, must not exceed blocks_max; otherwise MSCOMP_ARG_ERROR. A plain prefix sum,
 *                      as the reader's budget is: once it is exceeded, every later resource that changes is refused, a free cut included;
 *                   4. readable: a changed block must be readable exactly as the writer's rule 5 demands -- the container's table checks,
 *                      a decode to e bytes, and with d_block_crc the CRC-32 the table says; otherwise MSCOMP_DATA_ERROR. Fresh blocks
 *                      need no read;
 *                   5. a resource refused by rule 1, 3 or 4 is CARRIED: its length stays L, its count stays n, all its blocks are clean;
 *                   6. new data: a changed block's is the first min(e, e') bytes of its old data, then zeros up to e'; a fresh block's is
 *                      e' zero bytes. Both are dirty: their stored form follows the rule of mscomp_amd_blocks_compress (every fresh block
 *                      goes through the compress plan like any other unit) and their CRC-32 is computed again when the arrays are given;
 *                   7. every other kept block is clean: old entry d_block_first[r] + k becomes new entry d_new_block_first[r] + k with
 *                      its stored bytes and checksum verbatim; an unreadable clean entry gets the stored length 0 (the writer's rule 8);
 *                   8. room in the table: nb' = the sum of the final counts, n' for an accepted resource and n for a carried one. When
 *                      nb' exceeds n_blocks_table the whole call is refused as under rule 0. (Checked where the layout is made, behind
 *                      rule 4: a carried truncation counts with its old n.)
 *                   9. the tables: d_new_block_first is the exclusive running count of blocks, d_new_block_first[n_res] = nb';
 *                      d_new_block_off[0 .. nb'] the running sum of the stored lengths, the entries above nb' repeat the total;
 *                      d_new_block_crc is 0 at and above nb'; d_new_res_len[r] is W for an accepted resource and L for a carried one;
 *                  10. capacity, the writer's rule 9: a block that would end beyond new_cap is not written and its resource gets
 *                      MSCOMP_BUF_ERROR, which replaces whatever status the resource had; the tables still hold the full layout.
 *                 Consequence: when the old container was written by mscomp_amd_blocks_compress and _crc, is healthy, and every resource
 *                 is accepted, the new packed bytes, d_new_block_first, d_new_block_off and d_new_block_crc are byte for byte what those
 *                 two calls write for the resized data. W = 0 drops every block and decodes nothing; L = 0 makes every block fresh.
 *   Counts:       mscomp_amd_writer_counts after a resize: out[0] = the units (the admitted resources' changed and fresh blocks), out[1] =
 *                 the blocks decoded (the admitted changed blocks: each is decoded, or read where it lies when stored raw, once), out[2] =
 *                 the blocks encoded (the accepted resources' units); all 0 after a refused table.
 *   Execution:    as write: asynchronous on the ctx stream, kernels only (no memset or copy node), no allocation, no synchronisation,
 *                 nothing read back, a launch sequence fixed by the creation bounds; legal inside a caller's capture from the first
 *                 execution, a graph of its own -- not write's -- from the second. MSCOMP_ARG_ERROR for a null wr, d_block_first,
 *                 d_block_off, d_new_block_first or d_new_block_off, a null d_res_len, d_want_len, d_new_res_len or d_res_status when
 *                 n_res > 0, a null d_packed or d_new_packed unless blocks_max and n_blocks_table are 0, or when exactly one of
 *                 d_block_crc and d_new_block_crc is null.
 *   Left out:     resize and write fused in one call; one shared encoding for runs of fresh zero blocks (each is encoded on its own);
 *                 growth beyond blocks_max B bytes per call. */
MSCompStatus mscomp_amd_writer_resize(mscomp_amd_writer* wr, const uint8_t* d_packed, uint64_t packed_len,
                                      const uint64_t* d_block_first, const uint64_t* d_block_off, const uint64_t* d_res_len,
                                      const uint32_t* d_block_crc /* may be NULL */,
                                      const uint64_t* d_want_len /* n_res */,
                                      uint8_t* d_new_packed, uint64_t new_cap,
                                      uint64_t* d_new_block_first /* n_res + 1 */, uint64_t* d_new_block_off /* n_blocks_table + 1 */,
                                      uint32_t* d_new_block_crc /* NULL exactly when d_block_crc is */,
                                      uint64_t* d_new_res_len /* n_res */, int32_t* d_res_status /* n_res */);

/* Splice: a new container made of a list of picks (source, resource) out of up to MSCOMP_AMD_SPLICE_SRC_MAX source containers, without
 * decoding a byte. Deleting, reordering, duplicating and appending resources and merging containers are all pick lists. The stored form of
 * a block depends only on its data, the format and B, so a block is carried verbatim -- no format argument: the stored bytes are never
 * interpreted. Carrying them only makes sense between containers of ONE format and ONE block size: that is the caller's duty, nothing
 * here can check it. The only pass over the data is one move at copy speed.
 *   Creation:     MSCOMP_ARG_ERROR, all checked before the context is used and with *sp cleared, for a null ctx or sp, a block_size that is
 *                 not a power of two from 4096 to 524288, n_src of 0 or above MSCOMP_AMD_SPLICE_SRC_MAX, non-zero flags, or n_pick or
 *                 n_blocks_table (the rows of the NEW container's table) above 0x7FFFFFF0; MSCOMP_MEM_ERROR when the scratch cannot be
 *                 reserved.
 *   Scratch:      reserved once, at creation: 8 n_blocks_table + 64 bytes (the address of every new row's stored bytes).
 *   Sources:      src is a HOST array of n_src views, each a source container as its writer left it. The views are read on the host and
 *                 travel by value in the kernel arguments; nothing is uploaded. The sources are only read; the new arrays must not overlap
 *                 any source array.
 *   Notation:     pick p = (s, r) = d_pick[2 p], d_pick[2 p + 1] becomes resource p of the new container. B the block size,
 *                 L = src[s].d_res_len[r], first / off = src[s].d_block_first / d_block_off, n = first[r + 1] - first[r].
 *   Rules:        per pick, in this order:
 *                   1. MSCOMP_ARG_ERROR, nothing of the pick read further, when s >= n_src, r >= src[s].n_res, first[r] > first[r + 1]
 *                      or first[r + 1] > src[s].n_blocks_table;
 *                   2. block count: MSCOMP_DATA_ERROR when n is not L / B + (L % B != 0) (no sum is formed that can overflow);
 *                   3. room in the table: the running total of n over the picks that passed rules 1 and 2, in pick order, including this
 *                      pick and including picks refused here, must not exceed n_blocks_table; otherwise MSCOMP_ARG_ERROR. A saturating
 *                      prefix sum, as the reader's budget and resize's rule 3: once it is crossed every later pick with blocks is
 *                      refused; a pick without blocks is never refused here;
 *                   4. a refused pick is an EMPTY resource of the new container: d_new_res_len[p] = 0 and no rows. The pick index is
 *                      always the resource index;
 *                   5. an accepted pick: d_new_res_len[p] = L, and new row d_new_block_first[p] + k takes source row first[r] + k: its
 *                      stored bytes verbatim and, when checksums are carried, its CRC word verbatim. A source entry j that is not
 *                      off[j] <= off[j + 1] <= packed_len of its source has the stored length 0 and is never read (the writer's rule 8).
 *                      Nothing else about a block is judged: a damaged block stays damaged and is found by whoever decodes it;
 *                   6. the tables: d_new_block_first is the exclusive running count of rows, d_new_block_first[n_pick] = nb';
 *                      d_new_block_off[0 .. nb'] the running sum of the stored lengths, the entries above nb' repeat the total;
 *                      d_new_block_crc is 0 at and above nb';
 *                   7. capacity, the writer's rule 9: a block that would end beyond new_cap is not written and its pick gets
 *                      MSCOMP_BUF_ERROR, which replaces MSCOMP_OK; the tables still hold the full layout, and nothing at or behind
 *                      new_cap is ever written.
 *                 Picks may repeat (the resource is duplicated). n_pick = 0 is legal and writes an empty container.
 *                 Consequence: when every source was written by mscomp_amd_blocks_compress and _crc with one format and one B and is
 *                 healthy, and every pick is accepted, the new packed bytes, d_new_block_first, d_new_block_off and d_new_block_crc are
 *                 byte for byte what those two calls write for the picked resources' data in pick order, in a container with
 *                 n_blocks_max = n_blocks_table.
 *   Checksums:    with a non-null d_new_block_crc every view must have a d_block_crc (otherwise MSCOMP_ARG_ERROR); with a null one the
 *                 views' arrays are ignored.
 *   Execution:    as the writer's: asynchronous on the ctx stream, kernels only (no memset or copy node), no allocation, no
 *                 synchronisation, nothing read back, two launches fixed by the creation bounds (the layout, one workgroup; the move, a
 *                 fixed grid); legal inside a caller's capture from the first execution, a graph of its own from the second outside one,
 *                 captured again when an argument changes -- a field of a view counts as an argument. MSCOMP_ARG_ERROR for a null sp or
 *                 src, a null d_pick, d_new_res_len or d_status when n_pick > 0, a null d_new_block_first or d_new_block_off, a null
 *                 d_new_packed unless n_blocks_table is 0, or a view with a null table (or null d_packed with packed_len > 0) while its
 *                 n_res > 0.
 *   Left out:     a layout pass tiled over several workgroups (one workgroup scans the picks and the rows: the floor of the call on
 *                 tables of tens of thousands of rows); splice and write or resize fused in one call; more than four sources per call
 *                 (splice twice). */
#define MSCOMP_AMD_SPLICE_SRC_MAX 4u
typedef struct mscomp_amd_blocks_view {     /* one source container as its writer left it; only read */
    const uint8_t*  d_packed;  uint64_t packed_len;
    const uint64_t* d_block_first;          /* n_res + 1 */
    const uint64_t* d_block_off;            /* n_blocks_table + 1 */
    const uint64_t* d_res_len;              /* n_res */
    const uint32_t* d_block_crc;            /* n_blocks_table, may be NULL */
    uint64_t n_res, n_blocks_table;
} mscomp_amd_blocks_view;
typedef struct mscomp_amd_splicer mscomp_amd_splicer;
MSCompStatus mscomp_amd_splicer_create(mscomp_amd_ctx* ctx, uint32_t block_size, uint32_t n_src, size_t n_pick,
                                       uint64_t n_blocks_table /* of the NEW container */, uint32_t flags, mscomp_amd_splicer** sp);
void         mscomp_amd_splicer_destroy(mscomp_amd_splicer* sp);
MSCompStatus mscomp_amd_splicer_splice(mscomp_amd_splicer* sp, const mscomp_amd_blocks_view* src /* host array, n_src */,
                                       const uint64_t* d_pick /* 2 n_pick: source, resource */,
                                       uint8_t* d_new_packed, uint64_t new_cap,
                                       uint64_t* d_new_block_first /* n_pick + 1 */, uint64_t* d_new_block_off /* n_blocks_table + 1 */,
                                       uint32_t* d_new_block_crc /* n_blocks_table, may be NULL */,
                                       uint64_t* d_new_res_len /* n_pick */, int32_t* d_status /* n_pick */);

/* Splice by block extents: the splicer's second call. A new resource is the concatenation of EXTENTS -- block-aligned runs of blocks of
 * source resources -- instead of one whole resource, so joining resources, splitting one at a block boundary, cutting a block-aligned
 * range out (FALLOC_FL_COLLAPSE_RANGE), inserting blocks of another resource (FALLOC_FL_INSERT_RANGE) and keeping the first k blocks are
 * all extent lists, and none decodes a byte: the stored form of a block depends only on its data, the format and B, and that holds per
 * block. One format and one block size are the caller's duty, as for splice.
 *   Creation:     mscomp_amd_splicer_create_extents makes a mscomp_amd_splicer (destroyed by mscomp_amd_splicer_destroy) for n_res new
 *                 resources made of at most n_ext extents in all. Errors and bounds as mscomp_amd_splicer_create, all checked before the
 *                 context is used and with *sp cleared; n_res and n_ext each have the bound of n_pick (0x7FFFFFF0). Such a splicer also
 *                 serves mscomp_amd_splicer_splice with n_pick = n_res (its scratch is a superset; the two calls keep separate graphs). A
 *                 splicer made by mscomp_amd_splicer_create answers mscomp_amd_splicer_splice_extents with MSCOMP_ARG_ERROR and launches
 *                 nothing.
 *   Scratch:      reserved once, at creation: 8 n_blocks_table + 8 n_ext + 8 ceil(n_blocks_table / MSCOMP_AMD_SPLICE_ROW_TILE) + 80 bytes
 *                 (the address of every new row's stored bytes; one word per extent, + 1, for the extent's first new row; the stored
 *                 bytes of every tile of rows; the flag word of rule 0; 64 bytes of slack).
 *   Sources:      as splice's: a HOST array of n_src views, read on the host, passed by value, only read.
 *   Meaning:      new resource q is the concatenation of its extents e = d_ext_first[q] .. d_ext_first[q + 1] - 1, in that order. Extent
 *                 e = (s, r, k0, c) = d_ext[4 e .. 4 e + 3] stands for the blocks k0 .. k0 + c - 1 of resource r of source s;
 *                 c = 0xFFFFFFFFFFFFFFFF means "through the resource's last block", that is n - k0.
 *   Notation:     as splice's: B the block size, L = src[s].d_res_len[r], first / off = src[s].d_block_first / d_block_off,
 *                 n = first[r + 1] - first[r].
 *   Rules:        in this order:
 *                   0. the extent table as a whole: d_ext_first must not decrease anywhere and d_ext_first[n_res] must not exceed n_ext.
 *                      Otherwise every d_status is MSCOMP_ARG_ERROR, d_new_block_first, d_new_block_off, d_new_block_crc and
 *                      d_new_res_len are all 0, and nothing else is written (resize's rule 0). d_ext_first[n_res] is the count n_e of
 *                      extents in use; the entries of d_ext at and behind n_e -- and those in front of d_ext_first[0] -- are never read;
 *                   1. per extent, source and resource: MSCOMP_ARG_ERROR, nothing of the extent read further, when s >= n_src,
 *                      r >= src[s].n_res, first[r] > first[r + 1] or first[r + 1] > src[s].n_blocks_table;
 *                   2. per extent, block count: MSCOMP_DATA_ERROR when n is not L / B + (L % B != 0);
 *                   3. per extent, the range: MSCOMP_ARG_ERROR when k0 > n, or when c is not all-ones and c > n - k0 (no sum is formed
 *                      that can overflow). c = 0, or all-ones with k0 = n, is a legal EMPTY extent. The extent's data length len_e is
 *                      L - k0 B when it reaches block n - 1 and c B otherwise; 0 for an empty extent, and for one refused by rules 1-3;
 *                   4. per resource, alignment: every extent of the resource except its last non-empty one must have len_e % B == 0 -- a
 *                      short block can only be the last block of the new resource; otherwise MSCOMP_ARG_ERROR, for the extent that ends
 *                      short;
 *                   5. refusal: a resource with an extent refused by rules 1-4 is refused, with the status of its lowest-indexed refused
 *                      extent;
 *                   6. room in the table, splice's rule 3 over resources: the saturating running total of the block counts of the
 *                      resources that passed rules 1-5, in resource order, including this resource and including resources refused here,
 *                      must not exceed n_blocks_table; otherwise MSCOMP_ARG_ERROR. A resource without blocks is never refused here;
 *                   7. a refused resource is an EMPTY resource of the new container: d_new_res_len[q] = 0 and no rows. Resource indices
 *                      never shift;
 *                   8. an accepted resource: d_new_res_len[q] is the sum of its len_e, and its rows are its extents' source rows in
 *                      order -- new row (first new row of extent e) + i takes source row first[r] + k0 + i: its stored bytes verbatim and,
 *                      when checksums are carried, its CRC word verbatim. An unreadable source entry becomes an empty row (splice's rule
 *                      5). Nothing else about a block is judged;
 *                   9. the tables, the capacity and the checksum arrays: splice's rules 6 and 7 and its "Checksums" paragraph, unchanged,
 *                      with d_new_block_first[n_res] = nb'.
 *                 Extents may repeat and overlap (the blocks are duplicated). A resource with no extents is an empty resource with
 *                 MSCOMP_OK. n_res = 0 is legal and writes an empty container.
 *                 Consequence: when every source was written by mscomp_amd_blocks_compress and _crc with one format and one B and is
 *                 healthy, and every resource is accepted, the new packed bytes, d_new_block_first, d_new_block_off and d_new_block_crc
 *                 are byte for byte what those two calls write for the concatenated extent data, in a container with
 *                 n_blocks_max = n_blocks_table; mscomp_amd_res_crc_dev over the new tables gives the CRC-32 of each new resource's data.
 *   Execution:    as the splicer's: asynchronous on the ctx stream, kernels only (no memset or copy node), no allocation, no
 *                 synchronisation, nothing read back, five launches fixed by the creation bounds (one when n_blocks_table is 0): the
 *                 extent pass, one workgroup; the row passes in tiles of MSCOMP_AMD_SPLICE_ROW_TILE rows of the new table -- the tiles'
 *                 sums, their running sum (one workgroup), the rows --; the move, a fixed grid. The verdict of rule 0 is one flag word in
 *                 the scratch: the extent pass writes it, every later pass reads it, the launches are the same either way. Legal inside a
 *                 caller's capture from the first execution, a graph of its own from the second outside one, captured again when an
 *                 argument changes -- a field of a view counts as an argument. MSCOMP_ARG_ERROR for a null sp or src, a splicer made for
 *                 picks, a null d_ext_first, a null d_ext when n_ext > 0, a null d_new_res_len or d_status when n_res > 0, a null
 *                 d_new_block_first or d_new_block_off, a null d_new_packed unless n_blocks_table is 0, or a view with a null table (or
 *                 null d_packed with packed_len > 0) while its n_res > 0.
 *   Left out:     extents that start or end inside a block (they need a decode of the edge blocks: a writer's job); moving
 *                 mscomp_amd_splicer_splice onto the tiled layout; more than four sources per call. */
#define MSCOMP_AMD_SPLICE_ROW_TILE 1024u
MSCompStatus mscomp_amd_splicer_create_extents(mscomp_amd_ctx* ctx, uint32_t block_size, uint32_t n_src, size_t n_res /* of the NEW container */,
                                               size_t n_ext, uint64_t n_blocks_table /* of the NEW container */, uint32_t flags,
                                               mscomp_amd_splicer** sp);
MSCompStatus mscomp_amd_splicer_splice_extents(mscomp_amd_splicer* sp, const mscomp_amd_blocks_view* src /* host array, n_src */,
                                               const uint64_t* d_ext_first /* n_res + 1 */,
                                               const uint64_t* d_ext /* 4 n_ext: source, resource, first block k0, block count c */,
                                               uint8_t* d_new_packed, uint64_t new_cap,
                                               uint64_t* d_new_block_first /* n_res + 1 */, uint64_t* d_new_block_off /* n_blocks_table + 1 */,
                                               uint32_t* d_new_block_crc /* n_blocks_table, may be NULL */,
                                               uint64_t* d_new_res_len /* n_res */, int32_t* d_status /* n_res */);

/* Dedup: which resources of up to MSCOMP_AMD_SPLICE_SRC_MAX source containers hold the same bytes, without decoding a byte, answered as
 * the pick list mscomp_amd_splicer_splice takes -- "merge these containers and keep one copy of everything" is dedup, then splice, with no
 * host round trip between them. The stored form of a block depends only on its data, the format and B, so between containers of ONE format
 * and ONE block size (the caller's duty, as for splice) equal data means equal stored bytes, and equality is decided on the stored form.
 * Candidates are found from the tables and 32 bytes per row; the only pass over the data is the compare that confirms a candidate, which
 * reads the duplicates, and what they duplicate, once.
 *   Creation:     MSCOMP_ARG_ERROR, all checked before the context is used and with *dd cleared, for a null ctx or dd, a block_size that is
 *                 not a power of two from 4096 to 524288, n_src of 0 or above MSCOMP_AMD_SPLICE_SRC_MAX, non-zero flags, or n_res_total or
 *                 n_blocks_total above 0x7FFFFFF0; MSCOMP_MEM_ERROR when the scratch cannot be reserved.
 *   Scratch:      reserved once, at creation, and never grown: 56 n_res_total + 840 bytes (per resource its first row in the call's row
 *                 numbering, its key, its slot, its candidate, its flag and its place in the list of the refuted; a key table of
 *                 2 n_res_total + 64 slots of 12 bytes). n_blocks_total bounds the tables a call may bring and sizes the grids; nothing is
 *                 kept per row.
 *   Sources:      src is a HOST array of n_src views, handled as splice handles them: read on the host, passed by value, only read. The
 *                 output arrays must not overlap any source array.
 *   Numbering:    resource r of source s is g = src[0].n_res + ... + src[s - 1].n_res + r; N = the sum of all n_res must not exceed
 *                 n_res_total and the sum of all n_blocks_table must not exceed n_blocks_total: otherwise MSCOMP_ARG_ERROR from the call,
 *                 on the host, with nothing launched.
 *   Notation:     as splice's: B the block size, L = src[s].d_res_len[r], first / off = src[s].d_block_first / d_block_off,
 *                 n = first[r + 1] - first[r]; the stored length of row j is off[j + 1] - off[j].
 *   Rules:        per resource g = (s, r), in this order:
 *                   1. MSCOMP_ARG_ERROR when first[r] > first[r + 1] or first[r + 1] > src[s].n_blocks_table;
 *                   2. MSCOMP_DATA_ERROR when n is not L / B + (L % B != 0);
 *                   3. MSCOMP_DATA_ERROR when any of its rows j is not off[j] <= off[j + 1] <= packed_len of its source. No byte of
 *                      such a resource is read;
 *                   4. a resource refused by rules 1-3 is its own representative and nobody else's: d_rep[g] = g, it counts as unique
 *                      and is picked -- splice judges it again by its own rules;
 *                   5. two accepted resources are EQUAL when their L are equal and, row by row, their stored lengths are equal, their
 *                      stored bytes are equal and -- when checksums take part -- their CRC words are equal. Two empty resources are equal;
 *                   6. d_rep[g] is the smallest accepted h <= g equal to g, d_status[g] = MSCOMP_OK;
 *                   7. g is unique when d_rep[g] == g. d_pick holds the unique resources in ascending g as (s, r) pairs; every entry at or
 *                      behind 2 n_unique, up to 2 n_res_total, is 0xFFFFFFFFFFFFFFFF -- splice's rule 1 makes an empty resource of such a
 *                      pick, so a splicer created for n_res_total picks takes the array as it is. d_new_index[g] is the rank of d_rep[g]
 *                      among the unique resources. The entries of d_rep, d_new_index and d_status at and behind N are not written.
 *                      d_count[0] = n_unique, d_count[1] = N, d_count[2] = the stored bytes of all resources that are not unique -- what a
 *                      splice of the picks saves --, d_count[3] = the refuted (below).
 *                 N = 0 is legal and writes d_count = {0, 0, 0, 0} (and the padding of d_pick when one is given).
 *                 Consequence: splicing d_pick[0 .. 2 n_unique) out of the same views gives a container whose resource d_new_index[g] has
 *                 the length, the rows, the stored bytes and the CRC words of g, for every accepted g.
 *   Key:          the KEY TUPLE of an accepted resource is L and, per row, the stored length s, the CRC word when checksums take part,
 *                 the first min(16, s) and the last min(16, s) stored bytes. Equal resources have equal tuples. The tuple is mixed into
 *                 64 bits; the candidate of a resource is the smallest accepted resource with the same key. REFUTED, d_count[3], is the
 *                 number of accepted resources that share their key with a smaller accepted resource but are not equal to the smallest
 *                 such one -- they are still answered exactly, by rule 6. (Two different tuples that meet in their 64 bits would count
 *                 here too: about N^2 / 2^65 of all calls.) The four counts are the same from run to run.
 *   Checksums:    they take part exactly when every view has a non-null d_block_crc; otherwise all the arrays are ignored.
 *   Execution:    as the splicer's: asynchronous on the ctx stream, kernels only (no memset or copy node), no allocation, no
 *                 synchronisation, nothing read back, eight launches fixed by the creation bounds (two of one workgroup: rules 1 and 2
 *                 with the row numbering, and settle with emit); legal inside a caller's capture from the first execution, a graph of
 *                 its own from the second outside one, captured again when an argument changes -- a field of a view counts as an
 *                 argument. MSCOMP_ARG_ERROR for a null dd, src or d_count, any other null output array when N > 0, or a view with a
 *                 null table (or null d_packed with packed_len > 0) while its n_res > 0.
 *   Left out:     (block-level sharing inside one container is mscomp_amd_deduper_match with no store, below: a container of the unique
 *                 blocks and a recipe of extents say what the running-sum offset table cannot;) a tiled settle stage -- the refuted are settled by ONE workgroup, each against the earlier unique ones of its key, whole
 *                 resources compared one after the other: the floor of the call on adversarial inputs, as is the one workgroup that
 *                 scans the resources; tables whose resources overlap (damaged ones that still pass rules 1-3) are read once per
 *                 resource that claims a row, so the work follows the sum of n, not the table; dedup fused with splice in one call; more
 *                 than four sources per call. */
typedef struct mscomp_amd_deduper mscomp_amd_deduper;
MSCompStatus mscomp_amd_deduper_create(mscomp_amd_ctx* ctx, uint32_t block_size, uint32_t n_src, size_t n_res_total,
                                       uint64_t n_blocks_total, uint32_t flags, mscomp_amd_deduper** dd);
void         mscomp_amd_deduper_destroy(mscomp_amd_deduper* dd);
MSCompStatus mscomp_amd_deduper_dedup(mscomp_amd_deduper* dd, const mscomp_amd_blocks_view* src /* host array, n_src */,
                                      uint64_t* d_rep       /* n_res_total */,
                                      uint64_t* d_new_index /* n_res_total */,
                                      uint64_t* d_pick      /* 2 n_res_total: source, resource */,
                                      uint64_t* d_count     /* 4 */,
                                      int32_t*  d_status    /* n_res_total */);

/* Diff: the deduper's second call. Which blocks of the resources of a container differ from the blocks AT THE SAME INDEX of the resources of
 * its previous version (the base), without decoding a byte, answered as two extent lists mscomp_amd_splicer_splice_extents takes: the DELTA
 * list, which cuts the changed blocks out of the new container, and the PATCH list, which puts base and delta together again -- "keep
 * yesterday's container and what changed since" is diff, then one splice; "restore today's" is one more. The stored form of a block depends
 * only on its data, the format and B, so between containers of ONE format and ONE block size (the caller's duty, as for splice) equal data
 * means equal stored bytes, and equality is decided on the stored form. The tables tell most changed blocks; the only pass over the data is
 * the compare that confirms the others, which reads the stored bytes of the blocks that did NOT change, in both versions, once.
 *   Creation:     mscomp_amd_deduper_create_diff makes a mscomp_amd_deduper (destroyed by mscomp_amd_deduper_destroy, reported by the
 *                 scratch hooks under MSCOMP_AMD_SCRATCH_DEDUPER) for n_pair pairs whose new resources have at most n_blocks_new blocks in
 *                 all. Errors as mscomp_amd_deduper_create (there is no n_src), all checked before the context is used and with *dd
 *                 cleared; n_pair and n_blocks_new are bounded by 0x7FFFFFF0. Such a deduper answers mscomp_amd_deduper_dedup with
 *                 MSCOMP_ARG_ERROR and launches nothing, and a deduper made by mscomp_amd_deduper_create answers mscomp_amd_deduper_diff
 *                 the same way.
 *   Scratch:      reserved once, at creation, and never grown: 32 n_pair + 4 n_blocks_new + 64 ceil(n_blocks_new /
 *                 MSCOMP_AMD_SPLICE_ROW_TILE) + 72 bytes (per pair its first row in the call's row numbering and the three counts in front
 *                 of it; per new row a verdict word; eight words per tile of rows; 64 bytes of slack).
 *   Sources:      base and next are HOST views, read on the host, passed by value, only read. The output arrays must not overlap a source
 *                 array.
 *   Notation:     pair p = (a, b) = d_pair[2 p], d_pair[2 p + 1]: resource a of base (MSCOMP_AMD_DIFF_NO_BASE: none) and resource b of
 *                 next. B the block size; L_a, n_a and L_b, n_b the lengths and block counts (first[r + 1] - first[r]) of the two. Block k
 *                 of a resource of length L has the data length e(k) = min(B, L - k B) and the stored length off[first + k + 1] -
 *                 off[first + k].
 *   Rules:        in this order:
 *                   1. per pair, indices: MSCOMP_ARG_ERROR, no table entry of the pair read, when b >= next->n_res, or when a is not
 *                      MSCOMP_AMD_DIFF_NO_BASE and a >= base->n_res;
 *                   2. per pair, tables: dedup's rules 1-3 on resource b of next and, unless a is MSCOMP_AMD_DIFF_NO_BASE, on resource a of
 *                      base; the pair gets the status of the first rule that refuses, b judged before a under each. Of base resource a the
 *                      rows in front of n_b are judged by dedup's rule 3: the others are dropped (rule 5) and never looked at. No byte of a
 *                      refused pair is read;
 *                   3. room, the shape of splice-extents' rule 6: the saturating running total of n_b over the pairs that passed rule 1
 *                      and dedup's rules 1 and 2, in pair order, including this pair and including pairs refused here, must not exceed
 *                      n_blocks_new; otherwise MSCOMP_ARG_ERROR. (It is checked where the rows are numbered, in front of dedup's rule 3: a
 *                      pair that rule refuses has counted.) A pair with n_b = 0 is never refused here;
 *                   4. a refused pair has no extents in either list and d_changed[p] = 0. Pair indices never shift;
 *                   5. equality: block k of an accepted pair is UNCHANGED when a is not MSCOMP_AMD_DIFF_NO_BASE, k < n_a, the data lengths
 *                      e(k) are equal on both sides, the stored lengths are equal, the CRC words are equal -- when checksums take part --
 *                      and the stored bytes are equal. Otherwise it is CHANGED. Base blocks at and behind n_b are dropped;
 *                   6. runs: a RUN is a maximal stretch of consecutive blocks of one pair with the same verdict; every accepted pair with
 *                      n_b > 0 is a sequence of runs. The PATCH extents of pair p are its runs in order: an unchanged run [k0, k0 + c) is
 *                      (0, a, k0, c), a changed run is (1, p, i0, c) with i0 the number of changed blocks of the pair in front of k0. The
 *                      DELTA extents of pair p are its changed runs in order, (0, b, k0, c). Counts are always explicit, never all-ones.
 *                      d_delta_ext_first and d_patch_ext_first are the exclusive running counts of extents over the pairs, dense, entry
 *                      n_pair the number of extents in use; the entries of d_delta_ext and d_patch_ext at and behind that number are not
 *                      written. A run has at least one row, so neither list exceeds n_blocks_new extents;
 *                   7. counts: d_changed[p] = the changed blocks of the pair; d_count[0] = the changed blocks of all accepted pairs,
 *                      d_count[1] = the sum of n_b over the accepted pairs, d_count[2] = the stored bytes of all changed blocks -- the
 *                      packed length of the delta container --, d_count[3] = the REFUTED: the blocks whose data length, stored length and
 *                      -- when they take part -- CRC word agree but whose stored bytes differ. The four are the same from run to run.
 *                 n_pair = 0 is legal and writes d_count = {0, 0, 0, 0} and entry 0 of the two running counts (where given).
 *                 Consequence: mscomp_amd_splicer_splice_extents over the one source {next} with the delta lists writes a container D of
 *                 n_pair resources whose resource p is the changed blocks of b in order. The same call over the sources {base, D} with the
 *                 patch lists writes a container whose resource p has the length, the rows, the stored bytes and the CRC words of new
 *                 resource b, for every accepted pair; when the pairs are (., 0), (., 1), ... (., next->n_res - 1) and all are accepted,
 *                 its packed bytes and tables are byte for byte those of next. Splice-extents' rule 4 (only the last non-empty extent of
 *                 a resource may end short) holds by construction: a short block is the last block of b, so it ends D's resource p when
 *                 changed, and by the data-length clause of rule 5 a base block that is short where the new one is not is never carried.
 *   Checksums:    they take part exactly when both views have a non-null d_block_crc; otherwise both arrays are ignored.
 *   Execution:    as the deduper's: asynchronous on the ctx stream, kernels only (no memset or copy node), no allocation, no
 *                 synchronisation, nothing read back, seven launches fixed by the creation bounds (two when n_pair or n_blocks_new is 0):
 *                 the seed, one workgroup -- rules 1-3 and the row numbering --; the rows' verdicts from the tables and the compare that
 *                 confirms them, fixed grids; the runs in tiles of MSCOMP_AMD_SPLICE_ROW_TILE rows -- the tiles' sums, their running
 *                 values (one workgroup), the rows --; the counts. Legal inside a caller's capture from the first execution, a graph of
 *                 its own from the second outside one, captured again when an argument changes -- a field of a view counts as an
 *                 argument. MSCOMP_ARG_ERROR for a null dd, base, next or d_count, a deduper made for dedup, any other null array when
 *                 n_pair > 0 (d_delta_ext and d_patch_ext may be null while n_blocks_new is 0), or a view with a null table (or null
 *                 d_packed with packed_len > 0) while its n_res > 0.
 *   Left out:     (content-addressed matching -- a block that moved to another index or another resource counts as changed HERE -- is
 *                 mscomp_amd_deduper_match, below;) byte-granular deltas inside a block; more than one base per call; diff fused with the two splices in one call. */
#define MSCOMP_AMD_DIFF_NO_BASE 0xFFFFFFFFFFFFFFFFull
MSCompStatus mscomp_amd_deduper_create_diff(mscomp_amd_ctx* ctx, uint32_t block_size, size_t n_pair, uint64_t n_blocks_new, uint32_t flags,
                                            mscomp_amd_deduper** dd);
MSCompStatus mscomp_amd_deduper_diff(mscomp_amd_deduper* dd,
                                     const mscomp_amd_blocks_view* base, const mscomp_amd_blocks_view* next /* host, by value, only read */,
                                     const uint64_t* d_pair            /* 2 n_pair: base resource a, new resource b */,
                                     uint64_t* d_delta_ext_first       /* n_pair + 1 */,
                                     uint64_t* d_delta_ext             /* 4 n_blocks_new */,
                                     uint64_t* d_patch_ext_first       /* n_pair + 1 */,
                                     uint64_t* d_patch_ext             /* 4 n_blocks_new */,
                                     uint64_t* d_changed               /* n_pair: changed blocks of the pair */,
                                     uint64_t* d_count                 /* 4 */,
                                     int32_t*  d_status                /* n_pair */);

/* Match: the deduper's third call. For every block of the resources of a container (next), whether an EQUAL block already lies in one of
 * up to three store containers, earlier in next itself, or nowhere -- wherever that block lies: another index, another resource, another
 * container --, without decoding a byte, answered as two extent lists mscomp_amd_splicer_splice_extents takes: the DELTA list, which cuts
 * the blocks seen for the first time out of next, and the PATCH list, which puts the stores and the delta together again. "Keep what the
 * stores do not have yet" is match, then one splice; "restore today's" is one more. With no store at all the call single-instances the
 * blocks of ONE container into (D, recipe): the running-sum offset table cannot hold two rows at one address, a container of the unique
 * blocks and a list of extents can. The stored form of a block depends only on its data, the format and B, so between containers of ONE
 * format and ONE block size (the caller's duty, as for splice) equal data means equal stored bytes, and equality is decided on the stored
 * form. Candidates come from the tables and 32 bytes per row; the only pass over the data is the compare that confirms a candidate.
 *   Creation:     mscomp_amd_deduper_create_match makes a mscomp_amd_deduper (destroyed by mscomp_amd_deduper_destroy, reported by the
 *                 scratch hooks under MSCOMP_AMD_SCRATCH_DEDUPER) for n_src stores and one next container with at most n_res_total
 *                 resources and n_blocks_total table rows in all views together, of which next brings at most n_blocks_new.
 *                 MSCOMP_ARG_ERROR, all checked before the context is used and with *dd cleared, for a null ctx or dd, a block_size that is
 *                 not a power of two from 4096 to 524288, n_src above 3 (0 is legal: no store), non-zero flags, n_res_total or
 *                 n_blocks_total above 0x7FFFFFF0, or n_blocks_new above n_blocks_total; MSCOMP_MEM_ERROR when the scratch cannot be
 *                 reserved. Such a deduper answers mscomp_amd_deduper_dedup and mscomp_amd_deduper_diff with MSCOMP_ARG_ERROR and launches
 *                 nothing, and a deduper made by either other create answers mscomp_amd_deduper_match the same way.
 *   Scratch:      reserved once, at creation, and never grown: 48 n_res_total + 40 n_blocks_total + 4 n_blocks_new + 64 ceil(n_blocks_new /
 *                 MSCOMP_AMD_SPLICE_ROW_TILE) + 848 bytes (per resource its first row in the call's row numbering and the five counts in
 *                 front of it; per row its slot, its flag, its representative and its place in the list of the refuted, and a key table
 *                 of 2 n_blocks_total + 64 slots of 12 bytes; per row of next its rank among the fresh rows of its tile; eight words per
 *                 tile; the refuted count; 64 bytes of slack). No context buffer is used.
 *   Sources:      store is a HOST array of n_src views (may be null when n_src is 0), next a HOST view; read on the host, passed by value,
 *                 only read. The output arrays must not overlap a source array. The sum of all n_res must not exceed n_res_total, the
 *                 sum of all n_blocks_table must not exceed n_blocks_total and next->n_blocks_table must not exceed n_blocks_new:
 *                 otherwise MSCOMP_ARG_ERROR from the call, on the host, with nothing launched.
 *   Notation:     the resources are numbered as dedup numbers them, the stores' back to back and then next's: resource r of store s is
 *                 g = store[0].n_res + ... + store[s - 1].n_res + r, resource q of next is g = N_store + q; d_status has one entry per g.
 *                 B, L, first, off and n as for dedup. Block k of a resource has the data length e(k) = min(B, L - k B) and the stored
 *                 length off[first + k + 1] - off[first + k]. The ROWS of a call are the blocks of the accepted resources numbered densely
 *                 in the order of g, block by block: every row of a store is smaller than every row of next.
 *   Rules:        in this order:
 *                   1.-3. dedup's rules 1-3 per resource g, store and next alike;
 *                   4. room, the shape of diff's rule 3, because the scratch is per row: the saturating running total of n over the
 *                      resources that passed rules 1 and 2, in the order of g, including this resource and including resources refused
 *                      here, must not exceed n_blocks_total, and the same total over the resources of next alone must not exceed
 *                      n_blocks_new; otherwise MSCOMP_ARG_ERROR. (It is checked where the rows are numbered, in front of rule 3: a
 *                      resource that rule refuses has counted.) A resource with n = 0 is never refused here;
 *                   5. a refused resource of a store contributes no rows: nothing is found in it, and no byte of it is read. A refused
 *                      resource q of next has no extents in either list and d_class[3 q .. 3 q + 2] = 0: an empty resource of D and of
 *                      the rebuilt container. Resource indices never shift;
 *                   6. equality: two rows are EQUAL when their data lengths e(k) are equal, their stored lengths are equal, their CRC
 *                      words are equal -- when checksums take part -- and their stored bytes are equal. rep(u) is the smallest row equal
 *                      to u (u itself when there is none below it). A row u of next is FOUND when rep(u) is a row of a store, SHARED when
 *                      rep(u) is a smaller row of next, FRESH when rep(u) = u;
 *                   7. runs: a RUN is a maximal stretch of consecutive blocks of one resource of next with one class whose representatives
 *                      are consecutive blocks of one resource (fresh blocks are their own); every accepted resource with n > 0 is a
 *                      sequence of runs. The DELTA extents of resource q are its fresh runs [k0, k0 + c) in order, (0, q, k0, c), over
 *                      the one source {next}: D has next->n_res resources, resource q of D the fresh blocks of q in order. The PATCH
 *                      extents of resource q, over the sources {store[0], ..., store[n_src - 1], D}, are its runs in order: a found run
 *                      is (s, r, k0, c), where its representatives lie; a fresh run is (n_src, q, i0, c) with i0 the number of fresh
 *                      blocks of q in front of it; a shared run is (n_src, q', i', c) with q' the resource of next that holds its
 *                      representatives and i' the number of fresh blocks of q' in front of the first of them. Counts are always
 *                      explicit, never all-ones. d_delta_ext_first and d_patch_ext_first are the exclusive running counts of extents
 *                      over the resources of next, dense, entry next->n_res the number of extents in use; the entries of d_delta_ext and
 *                      d_patch_ext at and behind that number are not written. A run has at least one row, so neither list exceeds
 *                      n_blocks_new extents;
 *                   8. counts: d_class[3 q], [3 q + 1], [3 q + 2] = the found, shared and fresh blocks of resource q; d_count[0 .. 2] =
 *                      their sums, d_count[3] = the rows of next looked at (the sum of n over its accepted resources), d_count[4] = the
 *                      stored bytes of the fresh blocks -- the packed length of D --, d_count[5] = the refuted (below). All six and
 *                      every extent are the same from run to run.
 *                 A call whose views hold no resource writes d_count = {0, ...} and entry 0 of the two running counts (where given).
 *                 Consequence: mscomp_amd_splicer_splice_extents over {next} with the delta lists writes D; the same call over
 *                 {store..., D} with the patch lists writes a container whose resource q has the length, the rows, the stored bytes and
 *                 the CRC words of resource q of next, for every accepted q; when every resource of next is accepted its packed bytes and
 *                 tables are byte for byte those of next. Splice-extents' rule 4 (only the last non-empty extent of a resource may end
 *                 short) holds by construction: a block with e(k) < B is the last block of its resource -- in next, in a store, and, when
 *                 fresh, in D, whose resource q keeps the order of q. By the data-length clause of rule 6 a short block is only ever
 *                 represented by a short block of the SAME data length, so an extent ends short exactly when it carries the last block of
 *                 resource q, which only the last extent of q does; and no full block is ever represented by a short one.
 *   Key:          the KEY TUPLE of a row is its data length, its stored length s, its CRC word when checksums take part, and its first
 *                 min(16, s) and last min(16, s) stored bytes. Equal rows have equal tuples. The tuple is mixed into 64 bits; the
 *                 candidate of a row is the smallest row with the same key. REFUTED, d_count[5], is the number of rows of accepted
 *                 resources, stores included, that share their key with a smaller row but are not equal to the smallest such one. They
 *                 are still answered exactly: rep is the smallest EQUAL row, whatever shares its key -- equal rows share a key, so a
 *                 refuted row can only equal an earlier refuted row of its slot. (Two different tuples that meet in their 64 bits would
 *                 count here too.)
 *   Checksums:    they take part exactly when every view has a non-null d_block_crc; otherwise all the arrays are ignored.
 *   Execution:    as the deduper's: asynchronous on the ctx stream, kernels only (no memset or copy node), no allocation, no
 *                 synchronisation, nothing read back, ten launches fixed by the creation bounds (three when n_blocks_total is 0, seven
 *                 when n_blocks_new is 0): the key table cleared; the seed, one workgroup -- rules 1, 2 and 4 and the row numbering --;
 *                 rule 3, the keys into the table, and the compare that confirms a row against its candidate, fixed grids over the rows;
 *                 the settle, one workgroup; the runs in tiles of MSCOMP_AMD_SPLICE_ROW_TILE rows of next -- the tiles' sums, their
 *                 running values (one workgroup), the rows --; the counts. The walk along the key table is bounded by its slot count: a
 *                 damaged state may cost time and never spins. Minima are taken with atomics whose result does not depend on the order
 *                 of arrival, everything is counted in scans. Legal inside a caller's capture from the first execution, a graph of its
 *                 own from the second outside one, captured again when an argument changes -- a field of a view counts as an argument.
 *                 MSCOMP_ARG_ERROR for a null dd, next or d_count, a null store when n_src > 0, a deduper made for dedup or diff, any
 *                 other null array when n_res_total > 0 (d_delta_ext and d_patch_ext may be null while n_blocks_new is 0), or a view
 *                 with a null table (or null d_packed with packed_len > 0) while its n_res > 0.
 *   Left out:     a choice of representative that prefers longer runs -- the smallest equal row always wins, so a container full of equal
 *                 blocks (zeros, say) gets one extent per block; byte-granular or shifted (not block-aligned) matches; a tiled settle --
 *                 the refuted are settled by ONE workgroup, in ascending order, each against the earlier ones of its slot: the floor of
 *                 the call on adversarial inputs, as is the one workgroup that lists them; match fused with its two splices in one
 *                 call; more than three stores per call. */
MSCompStatus mscomp_amd_deduper_create_match(mscomp_amd_ctx* ctx, uint32_t block_size, uint32_t n_src /* 0 .. 3 stores */, size_t n_res_total,
                                             uint64_t n_blocks_total, uint64_t n_blocks_new, uint32_t flags, mscomp_amd_deduper** dd);
MSCompStatus mscomp_amd_deduper_match(mscomp_amd_deduper* dd,
                                      const mscomp_amd_blocks_view* store /* host array, n_src; may be NULL when n_src is 0 */,
                                      const mscomp_amd_blocks_view* next  /* host, by value, only read */,
                                      uint64_t* d_delta_ext_first       /* next->n_res + 1 */,
                                      uint64_t* d_delta_ext             /* 4 n_blocks_new */,
                                      uint64_t* d_patch_ext_first       /* next->n_res + 1 */,
                                      uint64_t* d_patch_ext             /* 4 n_blocks_new */,
                                      uint64_t* d_class                 /* 3 next->n_res: found, shared, fresh blocks of the resource */,
                                      uint64_t* d_count                 /* 6: found, shared, fresh, rows looked at, fresh stored bytes, refuted */,
                                      int32_t*  d_status                /* one per resource: the stores' back to back, then next's */);

/* Repair: the deduper's fourth call. From the verdicts mscomp_amd_blocks_salvage gave for a container (the primary, src[0]) and for up to
 * three copies of it (the mirrors: a mirror, the previous full container, the container a patch was built from), the extent list that
 * takes every bad row of the primary from the first mirror whose row is good. A table-only call: no stored byte is read. With salvage in
 * front and mscomp_amd_splicer_splice_extents behind, damage is found, located and mended on the device with no host between the stages.
 *   Creation:     block_size as everywhere; n_src = 1 .. MSCOMP_AMD_SPLICE_SRC_MAX sources, the primary first; n_res = the resources of
 *                 the answer (those of the primary); n_blocks_new bounds their rows; flags must be 0. MSCOMP_ARG_ERROR, before the context
 *                 is used and with *dd cleared, for a null ctx or dd, a bad block_size, n_src of 0 or above 4, non-zero flags, or a count
 *                 above 0x7FFFFFF0. A deduper made here answers dedup, diff and match with MSCOMP_ARG_ERROR, and dedupers made for those
 *                 answer repair the same way.
 *   Scratch:      reserved at creation under MSCOMP_AMD_SCRATCH_DEDUPER, once: diff's formula with n_res for n_pair -- 32 bytes per
 *                 resource, 4 per row of n_blocks_new and 64 per MSCOMP_AMD_SPLICE_ROW_TILE of them, + 72.
 *   Sources:      views as a splicer takes them, only read; d_verdict[s] (host array of n_src device arrays) has src[s].n_blocks_table
 *                 entries, as salvage wrote them for source s (a mirror salvaged with d_only = the primary's verdicts serves: SKIPPED is
 *                 not GOOD, and only the rows the primary lacks are asked for).
 *   Notation:     diff's. first_s, off_s, L_s, crc_s: the tables of source s; n = the rows of resource r of the primary; B = block_size.
 *   Rules:          0. r >= src[0].n_res: MSCOMP_ARG_ERROR, no table entry read.
 *                   1. Resource r of the primary is held to dedup's rules 1-2: first_0[r] > first_0[r + 1] or first_0[r + 1] >
 *                      n_blocks_table: MSCOMP_ARG_ERROR; first_0[r + 1] - first_0[r] != ceil(L_0 / B): MSCOMP_DATA_ERROR. A refused
 *                      resource has no extents and d_fixed = d_lost = 0.
 *                   2. Room, diff's rule 3: the saturating running total of n over the resources that passed rule 1, in order and
 *                      including this one, must not exceed n_blocks_new: MSCOMP_ARG_ERROR otherwise.
 *                   3. Choice. For row k of an accepted resource, c(k) is the lowest s whose copy is usable. s = 0 is usable when
 *                      d_verdict[0][first_0[r] + k] == MSCOMP_AMD_BLOCK_GOOD. s >= 1 is usable when r < src[s].n_res, resource r of
 *                      source s passes rule 1, L_s == L_0, d_verdict[s][first_s[r] + k] == MSCOMP_AMD_BLOCK_GOOD and -- when checksums
 *                      take part -- crc_s[first_s[r] + k] == crc_0[first_0[r] + k]. If no source is usable the row is LOST and
 *                      c(k) = 0: the primary's row is carried as it is, so repair never makes a container worse, and indices and
 *                      lengths never shift.
 *                   4. Runs. The extents of r are the maximal stretches of equal c, in order, written as (c, r, k0, count) with explicit
 *                      counts; d_ext_first (n_res + 1) is dense, as diff's: d_ext_first[n_res] extents in all.
 *                   5. d_fixed[r] = rows with c > 0, d_lost[r] = lost rows; d_status[r] is MSCOMP_OK when nothing is lost,
 *                      MSCOMP_DATA_ERROR otherwise.
 *                   6. d_count[0..3] = rows fixed, rows lost, stored bytes of the fixed rows in their mirrors, accepted resources with a
 *                      lost row.
 *   Consequence:  mscomp_amd_splicer_splice_extents over the same views with these lists writes a container of the primary's shape.
 *                 Assume every source was written by mscomp_amd_blocks_compress + _crc from the same data with one format and B, and was
 *                 then damaged in stored bytes, offset-table entries or CRC words: if no row is lost, the new packed bytes, tables and
 *                 checksums are BYTE FOR BYTE the undamaged container. Splice-extents' rule 4 holds by construction: equal L means equal
 *                 e at equal k.
 *   Checksums:    take part when every view brings d_block_crc: a mirror's row whose CRC word differs from the primary's is not usable.
 *                 (The word compared is the table's, not the data's: salvage held the data to it.)
 *   Execution:    as diff's: asynchronous on the ctx stream, kernels only, six launches fixed by the creation bounds -- seed, choice, the
 *                 three run passes in tiles of MSCOMP_AMD_SPLICE_ROW_TILE rows (the middle one is diff's), counts; two, seed and counts,
 *                 when n_res or n_blocks_new is 0 --, nothing allocated or read back; legal inside a capture from the first execution,
 *                 a graph of its own otherwise. MSCOMP_ARG_ERROR for a null dd, src, d_verdict or d_count, a view pack refuses, a null
 *                 d_verdict[s] of a source with rows, or a null required array (d_ext may be null when n_blocks_new is 0, every array
 *                 per resource when n_res is 0).
 *   Left out:     telling a damaged CRC word from damaged data (a primary row with a damaged word is replaced only by a mirror row
 *                 that carries the same damaged word; else it is lost); byte-granular salvage inside a block; repairing a refused
 *                 resource's block_first; fusing salvage, repair and splice in one call; more than three mirrors. */
MSCompStatus mscomp_amd_deduper_create_repair(mscomp_amd_ctx* ctx, uint32_t block_size, uint32_t n_src /* 1 .. 4 */, size_t n_res,
                                              uint64_t n_blocks_new, uint32_t flags, mscomp_amd_deduper** dd);
MSCompStatus mscomp_amd_deduper_repair(mscomp_amd_deduper* dd, const mscomp_amd_blocks_view* src /* host array, n_src; src[0] is the primary */,
                                       const uint32_t* const* d_verdict /* host array of n_src device arrays, src[s].n_blocks_table entries each */,
                                       uint64_t* d_ext_first /* n_res + 1 */, uint64_t* d_ext /* 4 n_blocks_new */,
                                       uint64_t* d_fixed /* n_res */, uint64_t* d_lost /* n_res */, uint64_t* d_count /* 4 */,
                                       int32_t* d_status /* n_res */);

/* Block transcoders: a container brought to another block size, another codec, or both. Every call that combines containers -- splice,
 * splice by extents, dedup, diff, match, delta, patch -- asks for one format and one block size; a transcoder is what gets a container there.
 * It is out of place, like a writer: it reads a container of format F1 cut at B1 and writes a NEW one of format F2 cut at B2. Resource
 * lengths do not change, and neither does any resource CRC-32 (mscomp_amd_res_crc_dev gives the same values for both containers).
 * Between two LZNT1 containers most blocks are CARRIED -- their stored bytes move as they lie, nothing is decoded or encoded --, because
 * an LZNT1 stream is the plain concatenation of its 4 KiB chunks' images and each image depends on that chunk's bytes alone.
 *   Creation:     (ctx, F1, B1, F2, B2, n_res, n_blocks_table, n_blocks_new, groups_max, flags = 0). The checks of the other block objects
 *                 for either (format, block size) pair and for the four counts (at most 0x7FFFFFF0), in the same order, before the
 *                 context is used: MSCOMP_ARG_ERROR, also for F1 = F2 with B1 = B2 (nothing to change: that is a splice);
 *                 MSCOMP_MEM_ERROR where groups_max G bytes are more than a dev plan can address. *tc is cleared on failure. A GROUP is
 *                 an aligned span of G = max(B1, B2) bytes of a resource: on a join (B2 > B1) one new block with its G / B1 source
 *                 members, on a split one source block with its G / B2 new blocks, with equal sizes one block of each. All scratch is
 *                 reserved here, once, and never grows: a cache and a staging area of groups_max G bytes each, a decompress dev plan for
 *                 F1 (groups_max G / B1 units) and a compress dev plan for F2 (groups_max G / B2 units) within groups_max G bytes each,
 *                 and the transcoder's tables: 92 bytes per decode unit, 72 per encode unit, 4 per group of groups_max, 12 per entry of
 *                 the coarser block table, 48 per entry of the new block table + 8 per MSCOMP_AMD_SPLICE_ROW_TILE of them, and 20 per
 *                 resource + 48. The LZNT1 dictionary flavour is fixed here, as for mscomp_amd_writer_create.
 *   Contract:     for a source written by mscomp_amd_blocks_compress with the same dictionary flavour whose blocks are healthy, the new
 *                 container is byte for byte -- packed bytes, d_new_block_first, d_new_block_off and, with checksums, d_new_block_crc of
 *                 every accepted resource -- what mscomp_amd_blocks_compress(F2, data, B2) and mscomp_amd_blocks_crc write for the data.
 *   Rules:        per resource, in this order, each leaving the other resources alone (L = d_res_len[r]):
 *                   0. the table as a whole, as the writer's rule 0: d_block_first[n_res] must not exceed n_blocks_table and
 *                      d_block_first must not decrease anywhere. Otherwise every resource gets MSCOMP_ARG_ERROR, the new tables are all
 *                      0, and nothing else is written;
 *                   1. MSCOMP_DATA_ERROR: d_block_first[r + 1] - d_block_first[r] is not ceil(L / B1);
 *                   2. MSCOMP_ARG_ERROR: the running total of ceil(L / B2) over ALL resources up to and including this one exceeds
 *                      n_blocks_new;
 *                   3. classes. A source block with stored length s and data length e is compressed-stored when 0 < s < e and raw-stored
 *                      when s = e; any other entry (a decreasing table, an end beyond packed_len included) makes its resource
 *                      MSCOMP_DATA_ERROR, unread.
 *                      F1 = F2 = LZNT1, join: a new block whose members are all compressed-stored is carried: its stored bytes are the
 *                      members', which lie adjacent. Any other new block is WORKED: its compressed-stored members are decoded into the
 *                      cache, its raw-stored members are copied there, and it is encoded from the cache under the rule of
 *                      mscomp_amd_blocks_compress (the counted bytes when shorter than the data, the raw block otherwise).
 *                      F1 = F2 = LZNT1, split, raw-stored source block: every new block of it is encoded from the bytes where they lie.
 *                      F1 = F2 = LZNT1, split, compressed-stored source block: its chunk headers are walked -- a little-endian uint16 h,
 *                      image length (h & 0x0FFF) + 3. The images must tile the s stored bytes into exactly ceil(e / 4096) chunks, and
 *                      no byte at or behind s is read; otherwise MSCOMP_DATA_ERROR. A new block whose chunks' images sum to less than
 *                      its data length is carried as those images. When any new block of the source block is not carried, the source
 *                      block is decoded once and those new blocks are stored raw from the decoded bytes; nothing is encoded.
 *                      Every other pair of formats and sizes: every compressed-stored source block is decoded, every raw-stored one
 *                      copied (read in place when its group has one source block), and every new block is encoded.
 *                      Checksums: on a join a carried block's CRC-32 is its members' folded by x^(8 d), as mscomp_amd_res_crc_dev folds
 *                      them; no data is read. Every DECODED source block is held to its old CRC-32 (MSCOMP_DATA_ERROR on a mismatch);
 *                      a worked block's new CRC-32 is computed from its data. On a split with checksums every compressed-stored source
 *                      block is decoded (its group is worked), held to its CRC-32, and the new blocks' CRC-32s are computed from the
 *                      decoded bytes; raw-stored source blocks are read in place. Carrying still happens: only the decode is added.
 *                      What carrying trusts: a carried block is not verified beyond the table checks and the header walk, exactly as
 *                      splice carries bytes: damage inside it is carried along. And a carried block is only valid at its new size when
 *                      every chunk but a resource's last holds 4096 bytes, as every LZNT1 stream of this library does;
 *                   4. the budget: a group is worked when anything in it is decoded or encoded. The running total of worked groups
 *                      over the resources that passed rules 1-3, up to and including this one, must not exceed groups_max; otherwise
 *                      MSCOMP_ARG_ERROR (the reader's rule 5). groups_max = the group count of the whole container never refuses;
 *                   5. verdicts before bytes: a source block that does not decode exactly as ms_decompress with capacity e to e bytes,
 *                      or not to its checksum, makes its resource MSCOMP_DATA_ERROR. A resource that failed any rule has NO blocks in
 *                      the new container, as a resource mscomp_amd_blocks_compress rejects: d_new_block_first[r + 1] =
 *                      d_new_block_first[r]. d_new_block_off is the exclusive running sum of the new stored lengths, the entries above
 *                      the count repeat the total; d_new_block_crc is 0 at and above the count;
 *                   6. capacity, the rule of mscomp_amd_blocks_compress: a block that would end beyond new_cap is not written and its
 *                      resource gets MSCOMP_BUF_ERROR; the tables still hold the full layout.
 *   Counts:       mscomp_amd_transcoder_counts gives, for the last execution, out[0] = new blocks carried (of the accepted resources),
 *                 out[1] = source blocks decoded, out[2] = new blocks encoded (both of the resources that passed rule 4); all 0 after
 *                 a refused table. It synchronises the ctx stream; returns 0, or -1 for a null argument or a failed read.
 *   Execution:    as the writer's: asynchronous on the ctx stream, kernels only, no allocation, no synchronisation, nothing read back, a
 *                 launch sequence fixed by the creation bounds; legal inside a caller's capture from the first execution, a graph of its
 *                 own from the second, captured again when an argument changes. d_new_block_first: n_res + 1, d_new_block_off:
 *                 n_blocks_new + 1, d_status: n_res; the new arrays must not overlap the old ones. MSCOMP_ARG_ERROR for a null tc or a
 *                 null required array (d_packed may be null when n_blocks_table is 0, d_new_packed when n_blocks_new is 0, d_res_len and
 *                 d_status when n_res is 0), or when exactly one of d_block_crc and d_new_block_crc is null. */
typedef struct mscomp_amd_transcoder mscomp_amd_transcoder;
MSCompStatus mscomp_amd_transcoder_create(mscomp_amd_ctx* ctx, MSCompFormat format, uint32_t block_size, MSCompFormat new_format,
                                          uint32_t new_block_size, size_t n_res, uint64_t n_blocks_table, uint64_t n_blocks_new,
                                          uint64_t groups_max, uint32_t flags, mscomp_amd_transcoder** tc);
void         mscomp_amd_transcoder_destroy(mscomp_amd_transcoder* tc);
MSCompStatus mscomp_amd_transcoder_transcode(mscomp_amd_transcoder* tc, const uint8_t* d_packed, uint64_t packed_len,
                                             const uint64_t* d_block_first, const uint64_t* d_block_off, const uint64_t* d_res_len,
                                             const uint32_t* d_block_crc /* may be NULL */,
                                             uint8_t* d_new_packed, uint64_t new_cap, uint64_t* d_new_block_first /* n_res + 1 */,
                                             uint64_t* d_new_block_off /* n_blocks_new + 1 */,
                                             uint32_t* d_new_block_crc /* NULL exactly when d_block_crc is */, int32_t* d_status /* n_res */);
int          mscomp_amd_transcoder_counts(mscomp_amd_transcoder* tc, uint32_t out[3]);

/* Sync: find the blocks of ONE store container at ANY byte offset of raw new data. diff compares blocks at the same index, match blocks
 * by content at any index; both decide on the stored form and see only block-aligned data: one byte inserted at the front of a resource
 * and every block behind it differs. The store's d_block_crc -- zlib's CRC-32 of every block's data -- is the signature rsync would send,
 * and CRC-32 rolls: with raw(M) the register after M from 0,
 *   crc32(M[p : p + B]) = raw(M[: p + B]) ^ raw(M[: p]) x^(8B) ^ seed(B)          (mod the CRC polynomial)
 * so a syncer evaluates the checksum of the B-byte window at every byte position of a batch of raw units in HBM against a key table of the
 * store's block checksums, confirms the candidates byte for byte against the decoded store blocks, and answers with a recipe the reader
 * applies: hits -- requests of mscomp_amd_reader_read with their output offsets -- and the literal runs between them.
 *   Creation:     (ctx, format, block_size, n_res, n_blocks_table, n_units, in_total_max, n_cand_max, flags = 0): the store's format, block
 *                 size B and table bounds as for mscomp_amd_reader_create; at most n_units raw units of in_total_max bytes together per
 *                 call; at most n_cand_max candidates are kept, confirmed and answered per call. The checks of every other create, in
 *                 their order, before the context is used and with *sy cleared: MSCOMP_ARG_ERROR for a null ctx or sy, a format or
 *                 block_size no container takes, non-zero flags, or n_res, n_blocks_table, n_units or n_cand_max above 0x7FFFFFF0;
 *                 MSCOMP_MEM_ERROR for in_total_max of 2^50 or more, in_total_max / MSCOMP_AMD_SYNC_TILE + n_units above 0x7FFFFFF0,
 *                 or where n_cand_max B bytes are more than a dev plan can address.
 *   Scratch:      all reserved here, once, and never grown; no context buffer and no scratch-hook kind. The reader core -- what
 *                 mscomp_amd_reader_create reserves for n_req = blocks_max = n_cand_max: an inner decompress dev plan, a cache of
 *                 n_cand_max B bytes, 88 + 44 bytes of tables per candidate and 4 per block-table entry -- and the syncer's own tables:
 *                   8 n_res + 12 slots + 40 n_units + 56 n_cand_max + 68 tiles + 4 pieces + 38064 bytes,
 *                   slots = 2 n_blocks_table + 64 rounded up to a power of two,
 *                   tiles = in_total_max / MSCOMP_AMD_SYNC_TILE + n_units, pieces = in_total_max / 64 + n_units
 *                 (a key table of `slots` slots of 12 bytes; the units' numberings; per tile of the scan eight words and
 *                 a register; per 64 bytes of input one register, raw(unit[: 64 j]); per candidate its position, unit, row, flag and
 *                 the reader core's request, length and status; a bitmap of 2^18 bits, two per word of the table, and 5 KiB of constants of B: the table that takes
 *                 a byte out of a window and four that multiply a register by x^(8B), written at creation).
 *   Sources:      store is ONE HOST view, read on the host, passed by value, only read; store->n_res and store->n_blocks_table must not
 *                 exceed the creation bounds and d_block_crc is required: otherwise MSCOMP_ARG_ERROR from the call, nothing launched.
 *                 Several stores: splice them first. Unit u is the d_in_len[u] bytes at d_in + d_in_off[u], at any alignment.
 *   Rules:        in this order (B, L, first, off as for dedup; M = a unit, len = its length):
 *                   1. store: dedup's rules 1 and 2 per resource and match's rule 3 per row, into d_res_status (store->n_res entries):
 *                      MSCOMP_ARG_ERROR for a first entry beyond n_blocks_table or decreasing, MSCOMP_DATA_ERROR for a block count other
 *                      than ceil(L / B) or a row that is not off[j] <= off[j + 1] <= packed_len. A refused resource contributes no
 *                      rows. The rows of the accepted resources are numbered densely in resource order. An ELIGIBLE row has B bytes
 *                      of data; a resource's short last block never takes part. A slot of the key table holds one CRC word and the
 *                      SMALLEST eligible row that has it (the claim-and-minimum scheme of match's key table);
 *                   2. units: the dev plans' bounds rule. A unit whose running total of d_in_len, itself included, exceeds in_total_max
 *                      gets MSCOMP_ARG_ERROR in d_status, no hits and no literal runs; every other unit MSCOMP_OK;
 *                   3. raw candidates: position p of unit u is one when p + B <= len and the table holds crc32(M[p : p + B]); its row
 *                      c(u, p) is that slot's row;
 *                   4. thinning: of a maximal run of consecutive positions p0, p0 + 1, ... that are all raw candidates with the same
 *                      row, only p0 + i B survive. (Without it a stretch of zeros longer than 2 B makes every position a candidate;
 *                      thinning leaves the positions a greedy walk would take.) Runs cross every seam of the scan;
 *                   5. the cap: the thinned candidates, ordered by (unit, position), are ranked by counts and scans, not by atomics;
 *                      the first n_cand_max are KEPT, the rest dropped. A capped call still answers with a valid recipe, only a
 *                      poorer one;
 *                   6. confirm: the rows of the kept candidates are decoded once each, however many candidates share a row, by the
 *                      reader's own passes over requests (r, k B, B), held to d_block_crc. A kept candidate is CONFIRMED when its row's
 *                      request is MSCOMP_OK -- decoded (or, stored raw, read) to B bytes with the right CRC-32 -- AND the B bytes of the
 *                      unit at p equal those bytes, compared in pieces of 16 KiB. Anything else is refuted: a miss, no other row is
 *                      tried;
 *                   7. selection, rsync's greedy walk: per unit, over its kept candidates in order of p, a confirmed one with
 *                      p >= end is a HIT and sets end = p + B; end starts at 0;
 *                   8. output: hits in (unit, position) order. d_hit_first (n_units + 1) is the exclusive running count of hits per
 *                      unit, entry n_units the total. For hit i, d_req[3 i ..] = (r, k B, B) and d_req_off[i] = d_in_off[u] + p: the
 *                      d_req and d_out_off of mscomp_amd_reader_read. The literal runs are the gaps: per unit, in order,
 *                      d_lit[2 i ..] = (d_in_off[u] + p, length) for every maximal stretch no hit covers; a run of length 0 is not
 *                      written. d_lit_first (n_units + 1) is indexed as d_hit_first. A unit shorter than B is one literal run, an empty
 *                      unit has none. Entries of d_req, d_req_off and d_lit at and behind the totals are not written. There are at most
 *                      n_cand_max hits and at most n_cand_max + n_units literal runs: size d_req (3 n_cand_max), d_req_off (n_cand_max)
 *                      and d_lit (2 (n_cand_max + n_units)) so;
 *                   9. counts: d_count[0 .. 7] = raw candidates, thinned, kept, confirmed, hits, literal runs, literal bytes, distinct
 *                      rows the reader core was asked for. All are the same from run to run.
 *   Consequence:  fill a buffer with the literal runs copied to their offsets, then run mscomp_amd_reader_read on the store with
 *                 d_req, d_req_off as d_out_off and capacities of B: the buffer then holds every accepted unit byte for byte at
 *                 d_in_off[u].
 *   Counts:       mscomp_amd_syncer_counts gives, for the last execution, out[0] = kept candidates, out[1] = distinct rows,
 *                 out[2] = hits. It synchronises the ctx stream; returns 0, or -1 for a null argument or a failed read.
 *   Execution:    asynchronous on the ctx stream, kernels only (no memset or copy node), no allocation, no synchronisation, nothing
 *                 read back, a launch sequence fixed by the creation bounds: the table and bitmap cleared, the seed (one workgroup),
 *                 rule 3 and the keys (fixed grids over the rows); the units' table pass (one workgroup); the boundary registers --
 *                 raw() of every 64-byte piece and every tile of MSCOMP_AMD_SYNC_TILE bytes, the tiles' running values (one
 *                 workgroup), the pieces' --; the scan, a wave per tile and 64 positions per lane, twice -- a tile pass that counts, a
 *                 tile scan (one workgroup), a runs pass that writes the kept candidates --; the requests; the reader's admission,
 *                 inner plan, CRC kernels and fold; the compare; the selection with the lists (one workgroup, a thread per unit).
 *                 No array is stored per position. The walk along the key table is bounded by its slot count. Legal inside a
 *                 caller's capture from the first execution, a graph of its own from the second outside one, captured again when an
 *                 argument changes -- a field of the view counts as an argument. MSCOMP_ARG_ERROR for a null sy, store, d_hit_first,
 *                 d_lit_first or d_count, and for any other null array the creation bounds give a size above 0.
 *   Left out:     several stores per call; a second row behind a refuted candidate (a forged or damaged row hides an equal healthy one
 *                 behind it); short last blocks; non-constant periodic data with a period below B floods the thinned list -- the cap
 *                 bounds it, and the candidates behind the cap are lost, not retried; hits written as a container. */
#define MSCOMP_AMD_SYNC_TILE 4096u
typedef struct mscomp_amd_syncer mscomp_amd_syncer;
MSCompStatus mscomp_amd_syncer_create(mscomp_amd_ctx* ctx, MSCompFormat format, uint32_t block_size, size_t n_res, uint64_t n_blocks_table,
                                      size_t n_units, uint64_t in_total_max, uint64_t n_cand_max, uint32_t flags, mscomp_amd_syncer** sy);
void         mscomp_amd_syncer_destroy(mscomp_amd_syncer* sy);
MSCompStatus mscomp_amd_syncer_sync(mscomp_amd_syncer* sy, const mscomp_amd_blocks_view* store /* host, by value, only read */,
                                    const uint8_t* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len,
                                    uint64_t* d_hit_first /* n_units + 1 */, uint64_t* d_req /* 3 per hit */, uint64_t* d_req_off /* 1 per hit */,
                                    uint64_t* d_lit_first /* n_units + 1 */, uint64_t* d_lit /* 2 per run */, uint64_t* d_count /* 8 */,
                                    int32_t* d_res_status /* store->n_res */, int32_t* d_status /* n_units */);
int          mscomp_amd_syncer_counts(mscomp_amd_syncer* sy, uint32_t out[3]);

/* Digests: a strong hash per block beside the CRC-32, and a syncer that confirms by it. The CRC-32 column is the weak half of rsync's
 * signature -- it rolls, and finds candidates --; a syncer made by mscomp_amd_syncer_create has to confirm each of them byte for byte and
 * so decodes the store's rows. The digest column is the strong half: 128 bits per block over the block's DATA, like the CRCs, so it
 * survives a transcode to another codec or a move to another container. digest(D) of a block D of 1 <= e <= 524288 bytes is BLAKE2s in
 * its tree mode (RFC 7693, parameter block): leaf size MSCOMP_AMD_DIGEST_LEAF = 1024, two levels (depth 2), unlimited fan-out (0), inner
 * and final length 16, no key, salt or personalisation; leaf i = the bytes [1024 i, 1024 i + 1024) of D with node_offset i, node_depth 0,
 * the last leaf with last_node; the root hashes the leaves' 16-byte digests back to back with node_offset 0, node_depth 1, last_node --
 * also over a single leaf. Python's hashlib.blake2s takes these parameters by name (tests/digest_model.py). On the device a digest is four
 * uint32 words h0 .. h3; as bytes, little-endian words in order, they are the 16 bytes of the hash. A digest column is
 * uint32_t[4 n_blocks_table], entry j for the block at d_block_off[j].
 *   Creation:     digester (ctx, block_size, n_res, in_total_max, flags = 0): the bounds of mscomp_amd_blocks_create without a format,
 *                 n_blocks_max = n_res + in_total_max / block_size. Digest syncer (ctx, block_size, n_res, n_blocks_table, n_units,
 *                 in_total_max, n_cand_max, flags = 0): the arguments of mscomp_amd_syncer_create without a format. The checks of every
 *                 other create, in their order, before the context is used and with the out pointer cleared: MSCOMP_ARG_ERROR for a
 *                 null ctx or out pointer, a block_size that is not a power of two from 4096 to 524288, non-zero flags, or a count
 *                 (n_res; a syncer's n_blocks_table, n_units, n_cand_max) above 0x7FFFFFF0; MSCOMP_MEM_ERROR for in_total_max of 2^50 or
 *                 more, a digester's n_blocks_max above 0x7FFFFFF0, a syncer's in_total_max / MSCOMP_AMD_SYNC_TILE + n_units above
 *                 0x7FFFFFF0.
 *   Scratch:      all reserved at creation, once, and never grown; no context buffer and no scratch-hook kind. A digester, with
 *                 m = n_blocks_max:
 *                   m (16 block_size / 1024 + 56) + 20 n_res + 72 bytes
 *                 (16 bytes per possible leaf; per possible block its offset, length and three more table words and a digest for
 *                 check; the per-resource words of the container's table passes). The container's own scratch does not change. A
 *                 digest syncer has NO reader core -- no inner plan, no cache of n_cand_max B bytes, no reader's tables --: the
 *                 syncer's own tables as stated for mscomp_amd_syncer_create, and
 *                   n_cand_max (16 block_size / 1024 + 32) + 64 bytes
 *                 (per kept candidate a unit-table entry of 16 bytes, block_size / 1024 leaf digests and one window digest).
 *   Sources:      blocks takes the resources as mscomp_amd_blocks_crc does, check the decoded output and the tables as
 *                 mscomp_amd_blocks_check does. sync_digest takes the store as mscomp_amd_syncer_sync does, and d_block_digest
 *                 (4 store->n_blocks_table words) as an argument of its own: mscomp_amd_blocks_view is not changed. d_block_crc is
 *                 still required -- the scan's key table is built from it -- and store->d_packed is never dereferenced and may be NULL.
 *   Rules:        blocks answers word for word as mscomp_amd_blocks_crc, a digest for a CRC word: the same acceptance of resources
 *                 (MSCOMP_ARG_ERROR past in_total_max, no blocks), the same numbering of blocks; entries at and behind the real block
 *                 count are four zero words; there is no resource digest. check follows mscomp_amd_blocks_check exactly: a resource
 *                 that is not MSCOMP_OK on entry is left alone, checks 1 and 2 and the clipped range are the same, the digest of block
 *                 k of the range (first block f) is compared with d_block_digest[4 (d_block_first[r] + f + k) ..], and a mismatch gives
 *                 MSCOMP_DATA_ERROR with d_out_len[r] = 0; nothing else is written. sync_digest: rules 1-5 and 7-9 of
 *                 mscomp_amd_syncer_sync, unchanged, and
 *                   6. a kept candidate (u, p, row) is CONFIRMED when digest(M_u[p : p + B]) equals the four words at the table row
 *                      of `row`; anything else is refuted. Every kept window is hashed once: d_count[7] and counts()[1] are the kept
 *                      count.
 *                 Kinds: mscomp_amd_syncer_sync on a digest syncer, and mscomp_amd_syncer_sync_digest on a syncer made by
 *                 mscomp_amd_syncer_create, return MSCOMP_ARG_ERROR with nothing launched. Destroy and counts are the existing calls.
 *   Consequence:  on a healthy store every output of sync_digest but d_count[7] equals what mscomp_amd_syncer_sync writes for the same
 *                 arguments, and the recipe rebuilds the units as stated there. A stored byte that was damaged after the digests were
 *                 taken does not change the answer: the reader that later applies the recipe holds the row to its CRC-32.
 *   Execution:    as the container's and the syncer's calls: asynchronous on the ctx stream, kernels only (no memset or copy node), no
 *                 allocation, nothing read back, a launch sequence fixed by the creation bounds; legal inside a caller's capture from
 *                 the first execution, a graph of its own from the second outside one. blocks: the container's table pass (two
 *                 launches), the leaf pass -- a fixed grid dealt over the leaf slots, a lane per leaf of up to 16 compressions, every
 *                 64-byte message block read with four 16-byte loads at any alignment --, the root pass -- a lane per block over its
 *                 16 ceil(e / 1024) bytes of leaf digests: 1 compression at 4096, 128 at 524288, the latency floor of a call --, which
 *                 also writes the statuses. check: the check's table pass, the leaves, the roots, the fold (a wave per resource).
 *                 sync_digest: the syncer's passes 1-4 and 6, and for pass 5 the requests, the kept windows as a unit table, the
 *                 leaves, the roots, a compare of 16 bytes per candidate. MSCOMP_ARG_ERROR for a null object and for any null array
 *                 the creation bounds give a size above 0 (d_block_digest: n_blocks_max, n_blocks_table). n_res = 0: blocks and check
 *                 return MSCOMP_OK and launch nothing.
 *   Left out:     units above 524288 bytes and a resource digest (a tree over the block digests is a later step); dedup, diff and
 *                 match confirming by digest, or matching across codecs by digest; salvage verdicts by digest; writers, resize,
 *                 splice and transcode carrying the digest column (recompute it with the digester); keyed digests. A digest syncer
 *                 never reads the store: a row damaged after its digest was taken is still offered as a hit, and it is the reader
 *                 applying the recipe, held to d_block_crc, that refuses it. */
#define MSCOMP_AMD_DIGEST_LEAF 1024u
typedef struct mscomp_amd_digester mscomp_amd_digester;
MSCompStatus mscomp_amd_digester_create(mscomp_amd_ctx* ctx, uint32_t block_size, size_t n_res, uint64_t in_total_max, uint32_t flags,
                                        mscomp_amd_digester** dg);
void         mscomp_amd_digester_destroy(mscomp_amd_digester* dg);
MSCompStatus mscomp_amd_digester_blocks(mscomp_amd_digester* dg, const uint8_t* d_data, const uint64_t* d_res_off, const uint64_t* d_res_len,
                                        uint32_t* d_block_digest /* 4 n_blocks_max */, int32_t* d_status);
MSCompStatus mscomp_amd_digester_check(mscomp_amd_digester* dg, const uint8_t* d_out, const uint64_t* d_out_off, const uint64_t* d_res_len,
                                       const uint64_t* d_block_first, const uint64_t* d_range, const uint32_t* d_block_digest,
                                       uint64_t* d_out_len, int32_t* d_status /* in and out */);
MSCompStatus mscomp_amd_syncer_create_digest(mscomp_amd_ctx* ctx, uint32_t block_size, size_t n_res, uint64_t n_blocks_table,
                                             size_t n_units, uint64_t in_total_max, uint64_t n_cand_max, uint32_t flags, mscomp_amd_syncer** sy);
MSCompStatus mscomp_amd_syncer_sync_digest(mscomp_amd_syncer* sy, const mscomp_amd_blocks_view* store,
                                           const uint32_t* d_block_digest /* 4 store->n_blocks_table */,
                                           const uint8_t* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len,
                                           uint64_t* d_hit_first, uint64_t* d_req, uint64_t* d_req_off, uint64_t* d_lit_first, uint64_t* d_lit,
                                           uint64_t* d_count, int32_t* d_res_status, int32_t* d_status);

/* Parity: Reed-Solomon parity rows beside a container, and lost rows back from them without a mirror. Salvage says which rows are bad and
 * repair mends them from a second full copy; a parity object closes the gap for the user who keeps ONE container: m parity rows for every
 * k stored rows -- m / k extra space instead of 100 % --, from which up to m lost rows per group are rebuilt. Like splice and dedup it
 * works on the STORED bytes: no format, no decoder. The code is RAID-6's, extended to three parities: GF(2^8) with polynomial 0x11D and
 * alpha = 2, P_p[x] = XOR_i alpha^(p i) D_i[x] for parity p < m over the members i < k of a group, D_i[x] = stored byte x of member i and 0
 * at and behind its stored length. The matrix alpha^(p i) is a Vandermonde one in distinct non-zero points, and for m <= 3 every choice of
 * e <= m missing members and ANY e of the parities is solvable (squaring is injective in characteristic 2; cubing is not, hence the cap).
 * Rebuild does not write a mended container: it writes a SPARSE MIRROR -- a view of the primary's shape in which every row it did not
 * rebuild has stored length 0 -- and the verdicts of that view, which mscomp_amd_deduper_repair and mscomp_amd_splicer_splice_extents take
 * as they take any mirror.
 *   Creation:     block_size as everywhere; n_blocks_table = the rows of the tables of every view the object will see; k = 1 ..
 *                 MSCOMP_AMD_PARITY_K_MAX members per group, m = 1 .. MSCOMP_AMD_PARITY_M_MAX parity rows per group; flags must be 0.
 *                 MSCOMP_ARG_ERROR, before the context is used and with *pr cleared, for a null ctx or pr, a block_size that is not a
 *                 power of two from 4096 to 524288, k of 0 or above 255, m of 0 or above 3, non-zero flags, or n_blocks_table above
 *                 0x7FFFFFF0; MSCOMP_MEM_ERROR when m G_max exceeds 0x7FFFFFF0 or the scratch cannot be reserved. G_max =
 *                 ceil(n_blocks_table / k). mscomp_amd_parity_bound: out[0] = m G_max parity rows, out[1] = m G_max block_size parity
 *                 bytes, the most a build writes; 0, or -1 for a null argument.
 *   Scratch:      reserved at creation, once, and never grown: 28 bytes per parity row of m G_max (its length, the bytes and the running
 *                 sum the CRC unit kernels read, its CRC-32), 12 per row of n_blocks_table (rebuild: the length it rebuilds, a flag),
 *                 24 per group of G_max (rebuild: the list of damaged groups with their inverse matrices), + 72. No inner plan: the
 *                 parity rows are units of the CRC kernels of mscomp_amd_blocks_crc, launched directly. The scratch hooks do not list it.
 *   Sources:      src: a view as a splicer takes one, only read; d_block_crc is not read. build writes the parity SET: d_par (16-byte
 *                 aligned, par_cap bytes), d_par_off (m G_max + 1), d_par_crc (m G_max), d_row_len (n_blocks_table), d_par_head (4).
 *                 rebuild reads the set and d_verdict (n_blocks_table entries, as mscomp_amd_blocks_salvage wrote them for src).
 *   Notation:     off = src.d_block_off, B = block_size, nb = src.d_block_first[src.n_res] (a device value), G = ceil(nb / k). GROUPS ARE
 *                 INTERLEAVED: row j is member i = j / G of group g = j % G, so a burst that destroys up to G consecutive rows costs
 *                 every group one member. Parity row q = g m + p. plen_g = the largest d_row_len of group g, rounded up to 16.
 *   Rules:        build --
 *                   0. nb > n_blocks_table, or src.n_blocks_table != n_blocks_table: d_status = MSCOMP_ARG_ERROR, d_par_head all zero,
 *                      every d_par_off 0, and nothing else is written.
 *                   1. d_row_len[j] = off[j + 1] - off[j] when j < nb, off[j] <= off[j + 1] <= packed_len and the length is at most B;
 *                      0 otherwise (such a row is never read) and at and behind nb.
 *                   2. Parity row q has plen_g bytes; d_par_off[0 .. m G] is the running sum, the entries above it, up to m G_max,
 *                      repeat the total. Every offset is a multiple of 16.
 *                   3. The bytes are the code's; pad bytes are the XOR of zeros, 0. No byte of d_packed outside a row's [off[j], off[j]
 *                      + d_row_len[j]) is read: tails are masked.
 *                   4. A parity row that would end beyond par_cap is not written at all, nothing at or behind par_cap ever is, and
 *                      d_status = MSCOMP_BUF_ERROR; the tables hold the full layout (the rule of mscomp_amd_compact_dev).
 *                   5. d_par_crc[q] = the CRC-32 (zlib's) of the plen_g bytes of row q; 0 at and behind m G and for a row rule 4 did
 *                      not write.
 *                   6. d_par_head = {nb, G, k, m}; d_status = MSCOMP_OK when rules 0 and 4 did not speak.
 *                 rebuild --
 *                   0. Build's rule 0 holds, with MSCOMP_ARG_ERROR; a d_par_head other than {nb, ceil(nb / k), k, m} -- parity of
 *                      another container or of another shape -- answers MSCOMP_DATA_ERROR. In both cases d_fix_block_off is all 0,
 *                      d_fix_verdict all MSCOMP_AMD_BLOCK_SKIPPED and d_count all 0.
 *                   1. Row j < nb is PRESENT when d_verdict[j] == MSCOMP_AMD_BLOCK_GOOD, off[j] <= off[j + 1] <= packed_len and
 *                      off[j + 1] - off[j] == d_row_len[j]; every other row j < nb is MISSING.
 *                   2. Parity row q is USABLE when d_par_off[q] <= d_par_off[q + 1] <= par_len, d_par_off[q] is a multiple of 16, its
 *                      length is plen_g as recomputed from d_row_len, and its CRC-32 equals d_par_crc[q]. An unusable row is never used.
 *                   3. Group g has e missing members and u usable parity rows. e = 0: nothing to do. 0 < e <= u: every missing member
 *                      is rebuilt with the e lowest-numbered usable parity rows -- the syndromes, the Horner pass over the present
 *                      members XOR the parity rows, times the inverse of the e x e matrix alpha^(p_a i_b). e > u: the group is
 *                      UNRECOVERABLE and none of its rows is rebuilt.
 *                   4. d_fix_block_off[0 .. nb] is the running sum of d_row_len[j] over the rebuilt rows j and of 0 over all others;
 *                      the entries above nb repeat the total. d_fix_packed holds the rebuilt rows' d_row_len[j] bytes in row order.
 *                   5. A rebuilt row that would end beyond fix_cap is not written: its verdict is SKIPPED and d_status is
 *                      MSCOMP_BUF_ERROR. (It still has its place in the tables and is counted as rebuilt.)
 *                   6. All n_blocks_table entries of d_fix_verdict are written: MSCOMP_AMD_BLOCK_GOOD for a row rebuilt and written,
 *                      MSCOMP_AMD_BLOCK_SKIPPED for every other row.
 *                   7. d_count[0..5] = rows missing, rows rebuilt, groups with a missing row, groups unrecoverable, parity rows
 *                      unusable (of the m G there are), stored bytes rebuilt. They are sums: the same from run to run.
 *                   8. d_status is the first that applies of rule 0, MSCOMP_BUF_ERROR (rule 5), MSCOMP_DATA_ERROR (some group
 *                      unrecoverable), MSCOMP_OK.
 *   Consequence:  the view {d_fix_packed, d_fix_block_off[nb], src.d_block_first, d_fix_block_off, src.d_res_len, src.d_block_crc} with
 *                 d_fix_verdict is a mirror as mscomp_amd_deduper_repair takes one, and parity composes with real mirrors: it is one
 *                 more source. Assume the container was written by mscomp_amd_blocks_compress + _crc, parity was built from it, and it
 *                 was then damaged in stored bytes or offset-table entries; assume the verdicts are salvage's with checksums. If no
 *                 group is unrecoverable, repair over {primary, fix view} followed by mscomp_amd_splicer_splice_extents writes BYTE FOR
 *                 BYTE the undamaged container: packed bytes, tables and checksums. Salvaging the fix view with d_only = the primary's
 *                 verdicts holds every rebuilt row to its CRC-32; a row that was not rebuilt has stored length 0 there and comes out
 *                 MSCOMP_AMD_BLOCK_TABLE, hence lost.
 *   Checksums:    d_par_crc guards the parity rows, by the CRC unit kernels over (d_par, d_par_off, plen) as a unit table; the
 *                 container's d_block_crc takes part only through the verdicts. Without d_block_crc salvage cannot see a flipped raw
 *                 byte, and a present row that is silently wrong makes every row rebuilt from its group wrong: parity is as good as
 *                 the verdicts.
 *   Execution:    as every other object's: asynchronous on the ctx stream, kernels only (no memset or copy node), no allocation,
 *                 nothing read back, a launch sequence fixed by the creation bounds; legal inside a caller's capture from the first
 *                 execution, a graph of its own from the second outside one, captured again when an argument or a view field changes.
 *                 build, nine launches: the row lengths, the groups' maxima, their running sum (one workgroup, in tiles), the CRC
 *                 units, the parity pass -- a fixed grid dealt over (group, column tile of 4096 bytes) items, a lane owning 16 bytes
 *                 of the column, 16-byte loads at any alignment with several in flight, m aligned 16-byte stores --, the three CRC
 *                 launches, the header. rebuild, nine: the groups' maxima, the parity rows' table check, the three CRC launches, the
 *                 damage pass (a lane per group: presence, counts, the damaged-group list and its inverse matrices), the fix table's
 *                 running sum, the solve pass over the listed groups only, the verdicts and counts. Healthy groups cost nothing but
 *                 their share of the fixed launches. MSCOMP_ARG_ERROR for a null object, a null view, a view pack refuses, a d_par
 *                 that is not 16-byte aligned, or any null array whose size by the creation bounds is above 0 (d_par_head, d_count
 *                 and d_status always). With n_blocks_table = 0 both calls return MSCOMP_OK and write only the header, the counts
 *                 and the status, in one and two launches.
 *   Left out:     damage to the parity set's own tables (d_par_off, d_par_crc, d_row_len, d_par_head) and to d_block_first / d_res_len
 *                 -- small metadata the caller keeps twice; telling a damaged CRC word from damaged data (as in repair, a row whose
 *                 CRC word is damaged is rebuilt to the same bytes and is still refused by a later salvage); m > 3, which is not
 *                 solvable in general; updating parity in place after a write -- build again; parity over the data instead of the
 *                 stored form; fusing salvage, rebuild, repair and splice in one call. */
#define MSCOMP_AMD_PARITY_K_MAX 255u
#define MSCOMP_AMD_PARITY_M_MAX 3u
typedef struct mscomp_amd_parity mscomp_amd_parity;
MSCompStatus mscomp_amd_parity_create(mscomp_amd_ctx* ctx, uint32_t block_size, uint64_t n_blocks_table, uint32_t k, uint32_t m,
                                      uint32_t flags, mscomp_amd_parity** pr);
void         mscomp_amd_parity_destroy(mscomp_amd_parity* pr);
int          mscomp_amd_parity_bound(const mscomp_amd_parity* pr, uint64_t out[2]);   /* parity rows m*G_max, parity bytes m*G_max*block_size */
MSCompStatus mscomp_amd_parity_build(mscomp_amd_parity* pr, const mscomp_amd_blocks_view* src,
                                     uint8_t* d_par, uint64_t par_cap, uint64_t* d_par_off /* m*G_max + 1 */, uint32_t* d_par_crc /* m*G_max */,
                                     uint32_t* d_row_len /* n_blocks_table */, uint64_t* d_par_head /* 4 */, int32_t* d_status /* 1 */);
MSCompStatus mscomp_amd_parity_rebuild(mscomp_amd_parity* pr, const mscomp_amd_blocks_view* src, const uint32_t* d_verdict /* n_blocks_table */,
                                       const uint8_t* d_par, uint64_t par_len, const uint64_t* d_par_off, const uint32_t* d_par_crc,
                                       const uint32_t* d_row_len, const uint64_t* d_par_head,
                                       uint8_t* d_fix_packed, uint64_t fix_cap, uint64_t* d_fix_block_off /* n_blocks_table + 1 */,
                                       uint32_t* d_fix_verdict /* n_blocks_table */, uint64_t* d_count /* 6 */, int32_t* d_status /* 1 */);

/* Resource checksums from block checksums. After a write or a resize the block CRC-32s are current and the resource CRC-32s that
 * mscomp_amd_blocks_crc once wrote are stale; the block checksums determine them, and no data has to be read:
 *   d_res_crc[r] = XOR over the resource's blocks j of d_block_crc[j] x^(8 d_j)  (mod the CRC polynomial), d_j = the resource's bytes behind block j
 * -- zlib's crc32_combine applied along the resource; 0 for an empty resource. d_block_first (n_res + 1, never decreasing: the table a
 * container wrote), d_res_len (n_res), d_block_crc (n_blocks_table). Per resource: MSCOMP_ARG_ERROR when d_block_first[r] or
 * d_block_first[r + 1] exceeds n_blocks_table, MSCOMP_DATA_ERROR when the block count is not ceil(L / B); d_res_crc[r] is 0 in both cases.
 * Two launches: a seed kernel over the resources, then a fixed grid dealt over the BLOCKS of the table -- one resource of a million blocks
 * spreads over every CU --, each block folded into its resource's word with an atomic XOR. Asynchronous on the ctx stream, no scratch, no
 * allocation, nothing read back; may be captured. MSCOMP_ARG_ERROR, before the context is used, for a null ctx, a block_size that is not
 * a power of two from 4096 to 524288, n_res or n_blocks_table above 0x7FFFFFF0, or a null array when n_res > 0. n_res = 0 returns MSCOMP_OK. */
MSCompStatus mscomp_amd_res_crc_dev(mscomp_amd_ctx* ctx, uint32_t block_size, size_t n_res, uint64_t n_blocks_table,
                                    const uint64_t* d_block_first, const uint64_t* d_res_len, const uint32_t* d_block_crc,
                                    uint32_t* d_res_crc /* n_res */, int32_t* d_status /* n_res */);

/* ---- measurement hooks (bench.py / profiles) ---- */
/* When enabled, every kernel launch of plan_execute is bracketed by hipEvents on the ctx stream. */
void         mscomp_amd_profile_enable(mscomp_amd_ctx* ctx, int on);
/* Synchronizes the stream, then returns the number of distinct kernels seen since the last reset and fills
 * up to cap entries: name (static string), accumulated milliseconds, launch count. Resets the counters. */
int          mscomp_amd_profile_read(mscomp_amd_ctx* ctx, const char** names, double* ms, uint64_t* launches, int cap);
/* Stage-level test hook: per-position matches (len-3 capped at 45, offset; 0 = no match) of ONE device-resident buffer as
 * found by the HIP hash-chain match finder. max_off = 0x2000 (Xpress) / 0xFFFF with clip=1 (Xpress+Huffman). */
MSCompStatus mscomp_amd_debug_xpress_matches(mscomp_amd_ctx* ctx, const uint8_t* d_in, size_t in_len, uint32_t max_off, int clip,
                                             uint16_t* h_len3, uint16_t* h_off);
/* Stage-level test hook: the code lengths HuffmanEncoder<15,512>::CreateCodes (include/mscomp/HuffmanEncoder.h:58-107, the heap build with
 * its > 15-bit rescale loop) gives for n histograms of 512 counts; h_counts (n x 512 uint32) and h_lens (n x 512 bytes) are host arrays. */
MSCompStatus mscomp_amd_debug_huff_lengths(mscomp_amd_ctx* ctx, const uint32_t* h_counts, size_t n, uint8_t* h_lens);
/* Stage-level test hook: the same for HuffmanEncoder<15,512>::CreateCodesSlow (HuffmanEncoder.h:129-226, package-merge), run by the device
 * function the literals-only fallback of Xpress+Huffman runs. A fallback chunk has literals and the end-of-stream symbol only and the kernel's
 * package pool is sized for these 257 leaves: a histogram with a count on a symbol above 0x100 is MSCOMP_ARG_ERROR. */
MSCompStatus mscomp_amd_debug_huff_lengths_slow(mscomp_amd_ctx* ctx, const uint32_t* h_counts, size_t n, uint8_t* h_lens);
/* The mscomp_amd_debug_set_* hooks below choose between BIT-IDENTICAL kernels for the tests and are process-wide; the library ignores them unless
 * MSCOMP_AMD_TEST_HOOKS=1 was in the environment when it was loaded (1 = they work). A deployment never sets it. */
int          mscomp_amd_debug_hooks_enabled(void);
/* Test hook: the Xpress parse/emit stage has two bit-identical kernels (one wave per unit; four
 * or sixteen waves per unit with speculative segments). 0 = chosen by batch size (default), 1 / 2 / 3 = force. Process-wide. */
void         mscomp_amd_debug_set_xpress_emit(int mode);
/* The reference has two LZNT1 dictionaries, chosen when it is BUILT (/root/reference/include/mscomp/config.h:83-88): the default one and,
 * with -DMSCOMP_WITH_LZNT1_SA_DICT, a suffix-array one (/root/reference/include/mscomp/LZNT1Dictionary_SA.h) whose matches have the same
 * lengths but other offsets -- so the compressed bytes differ. A deployment that replaces such a build selects the same flavour here.
 * The flavour is a property of a PLAN, fixed when the plan is created: from its context's setting (mscomp_amd_ctx_set_lznt1_sa_dict: 1 / 0, -1 =
 * follow the process default) or else from the process default (mscomp_amd_set_lznt1_sa_dict, or MSCOMP_AMD_LZNT1_SA_DICT=1 in the environment
 * when the library loads). Changing a setting never touches a plan that exists. The entries without a context argument (ms_compress, ms_deflate,
 * mscomp_amd_compress_units_host) make their plans per call and follow the process default of that moment. Decompression is not affected. */
void         mscomp_amd_set_lznt1_sa_dict(int on);
int          mscomp_amd_get_lznt1_sa_dict(void);
MSCompStatus mscomp_amd_ctx_set_lznt1_sa_dict(mscomp_amd_ctx* ctx, int on);
/* Test hook: Xpress decompression has two bit-identical paths: 0 = default (32-bit tokens, a flag word per step, then the copy kernels that
 * Xpress+Huffman uses), 1 = one wave per stream taking a token per step and moving the bytes itself (round 1's kernel). Process-wide. */
void         mscomp_amd_debug_set_xpress_decoder(int mode);
/* Test hook: after a decompression whose large units (capacity >= 1 MiB) got their bytes from csrc/lzglobal.hip: out[0..32] = words still
 * pointing after each pointer pass (`words` = sum over those units of capacity + 64; not used when a dev plan with
 * MSCOMP_AMD_DEV_LARGE_UNITS ran last: the library knows where that plan keeps them). 0 = read. */
int          mscomp_amd_debug_lzg_open(mscomp_amd_ctx* ctx, uint64_t words, uint32_t* out);
/* Test hook: how the Xpress match finder runs. 1 = default: batches whose units are at most 64 KiB run Find only where a greedy parse can
 * start a token (csrc/xpress_lazy.hip); 2 = Find for every position everywhere (xp_find_kernel, what longer streams and Xpress+Huffman
 * always use). The parse kernels get the same answers on every path they walk. Process-wide. */
void         mscomp_amd_debug_set_finder(int mode);
/* Test hook: how a host-pointer ms_compress(MSCOMP_LZNT1) of a large buffer (>= 36 MiB) runs. 0 = default (the caller's buffers are mapped
 * into the GPU's address space, one launch; falls back to 1 when the mapping fails), 1 = always in slices on three streams
 * (csrc/oneshot.hip lznt1_compress_pipelined; the same as MSCOMP_AMD_ONE_ZEROCOPY=0 in the environment). Same bytes and statuses. Process-wide. */
void         mscomp_amd_debug_set_one_shot(int mode);
/* Test hook: the LZNT1 chunk stage has two bit-identical kernels (one wave / four waves per 4 KiB chunk). 0 = default, 1 / 2 = force. */
void         mscomp_amd_debug_set_lznt1(int mode);
/* Test hook: the LZNT1 chunk images are moved to their places by a grid that is fixed by the device, every block taking tiles of 64 chunks
 * b, b + grid, ...; n > 0 = at most n blocks (a block's second tile then runs in a batch of 65 chunks and more), 0 = default. Same bytes. */
void         mscomp_amd_debug_set_place_blocks(int n);
/* Test hook: LZNT1 decompression finds the chunk headers by walking speculated chains per 48 KiB segment of the input; a segment
 * whose speculation held nothing usable is walked again by one lane. Returns how many segments that happened to since the last call
 * (synchronizes the stream). */
uint32_t     mscomp_amd_debug_lzd_walked(mscomp_amd_ctx* ctx);
/* Test hook: which path the last decompress or size execution on ctx took, per unit (synchronizes the stream). Xpress+Huffman: one word per
 * unit, 2 = its chunks were decoded in parallel from speculated chunk starts, 1 = the serial walk. Xpress: one word per unit of at least
 * 512 KiB input, in unit order, 2 = walked by segments, 0 = the one-wave walk; none when the plan does not take the segment path. LZNT1:
 * none. Writes min(count, cap) words to out and returns the count, -1 on error. */
int          mscomp_amd_debug_decode_modes(mscomp_amd_ctx* ctx, uint32_t* out, size_t cap);
/* Test hook: what the plan's last execution put on the optional decoding paths (synchronizes the stream): out[0] = units walked by
 * segments, out[1] = units on the all-CU byte stage, out[2] = candidate slots with token scratch. A host plan: the counts chosen when it
 * was created; a dev plan with MSCOMP_AMD_DEV_LARGE_UNITS: read back from the tables its last execution built (0 before the first); any
 * other dev plan: 0. Returns 0, -1 on error. Works with or without MSCOMP_AMD_TEST_HOOKS (it switches nothing). */
int          mscomp_amd_debug_plan_paths(mscomp_amd_plan* plan, uint32_t out[3]);
/* Test hooks for the scratch contract: what an execution reads from scratch it has written itself, and no kernel touches
 * the slack behind the bytes a buffer was reserved for. A target is (kind, object): a context (NULL = the calling thread's context of the
 * one-shot entries, if it has one yet) with its scratch buffers; a plan with its tables; a block container, reader, writer, splicer or
 * deduper with its own buffers and those of the dev plans inside it (names "cplan.*", "dplan.*"). All three need MSCOMP_AMD_TEST_HOOKS=1 and
 * return -1 without it, for a null object, an unknown kind or a failed device call; then nothing is touched. */
#define MSCOMP_AMD_SCRATCH_CTX     0
#define MSCOMP_AMD_SCRATCH_PLAN    1
#define MSCOMP_AMD_SCRATCH_BLOCKS  2
#define MSCOMP_AMD_SCRATCH_READER  3
#define MSCOMP_AMD_SCRATCH_WRITER  4
#define MSCOMP_AMD_SCRATCH_SPLICER 5
#define MSCOMP_AMD_SCRATCH_DEDUPER 6
typedef struct mscomp_amd_scratch_rec {
	const char* name;                /* static string: the buffer's name in the library's source */
	uint64_t asked, cap, changed;    /* the most bytes it was reserved for, the bytes it has, bytes of [asked, cap) that differ from `byte` */
} mscomp_amd_scratch_rec;
/* The names of a context's scratch buffers, in the order of a report on a context: min(count, cap) of them to names, returns the count.
 * Needs no device. */
int          mscomp_amd_debug_scratch_names(const char** names, int cap);
/* Fills, on the context's stream, every buffer of the target over all its bytes (slack_only 0) or over its slack [asked, cap) alone
 * (slack_only 1) with `byte`; captured graphs stay valid (no buffer moves). The tables of a plan with HOST tables hold what its creation
 * uploaded: such a plan refuses slack_only 0 (-1). Returns the number of buffers filled. */
int          mscomp_amd_debug_scratch_poison(int kind, void* object, int slack_only, int byte);
/* Synchronizes the stream, then one record per buffer of the target, min(count, cap) of them; returns the count. */
int          mscomp_amd_debug_scratch_report(int kind, void* object, int byte, mscomp_amd_scratch_rec* recs, int cap);
/* Hardware self-check: the LZNT1 bucket sort and the Xpress chain links rely on gfx950 serving the returning
 * same-address LDS atomics of one wave instruction in lane order. Returns the number of lanes (over blocks x rounds x 64
 * lanes x {add, exchange}, keys drawn from nkeys <= 2048 values) that were served out of order: 0 on gfx950;
 * 0xFFFFFFFF if the check could not run. */
uint32_t     mscomp_amd_debug_lds_lane_order(mscomp_amd_ctx* ctx, uint32_t seed, uint32_t blocks, uint32_t rounds, uint32_t nkeys);
/* Hardware self-check: the LZNT1 match compares hand v_alignbyte_b32 a byte address as its shift and rely on the instruction reading bits
 * [1:0] of it alone. Returns the number of results (256 low bytes x 16 settings of the bits above them x 4 dword pairs x {vector, scalar}
 * operand, the dwords drawn from seed) that differ from {hi, lo} >> 8 (operand & 3): 0 on gfx950; 0xFFFFFFFF if the check could not run. */
uint32_t     mscomp_amd_debug_alignbyte(mscomp_amd_ctx* ctx, uint32_t seed);
/* A device that serves them in another order is not refused: the two kernels then issue that atomic one lane at a time (the same bytes, a
 * slower sort; csrc/kernels.h). Test hook: 1 = run that order-independent form on every device, 0 = back to the default. Process-wide. */
void         mscomp_amd_debug_set_serial_atomics(int on);
/* Version / build string of the library (includes the gfx target it was compiled for). */
const char*  mscomp_amd_version(void);

#ifdef __cplusplus
}
#endif
#endif
