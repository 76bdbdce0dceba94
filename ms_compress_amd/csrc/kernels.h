// kernels.h -- host-callable launchers of the gfx950 kernels (internal to libmscomp_amd.so).
#pragma once
#include "common.h"
#include <atomic>

namespace msc {

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is a PER-DEVICE setting: every launcher keeps one of these per kernel and sets
// the attribute the first time it launches on a device (bit = device ordinal; two host threads racing set it twice, which is
// harmless). A process-wide `static bool` left the second GPU of a process without the attribute.
struct PerDeviceOnce {
	std::atomic<uint64_t> seen[4] = {};                      // 256 device ordinals
	bool needed() const { int d = 0; (void)hipGetDevice(&d); return !((seen[(d >> 6) & 3].load(std::memory_order_acquire) >> (d & 63)) & 1u); }
	void done() { int d = 0; (void)hipGetDevice(&d); seen[(d >> 6) & 3].fetch_or(1ull << (d & 63), std::memory_order_release); }
};

// ---- lane order of same-address LDS atomics (util.hip) ----
// The LZNT1 bucket sort and the Xpress chain links hand out slots / links with ONE returning LDS atomic per 64 positions and need the
// same-address atomics of that instruction served in lane order -- what gfx950 does, checked once per device (ctx.hip lane_order_verdict). On
// a device that fails the check (or when the test hook says so) the same kernels issue the atomic one lane at a time, in a 64-step loop: DS
// operations of a wave execute in program order, which IS architectural. Same bytes, slower sort.
bool serial_atomics_on_current_device();
void set_serial_atomics(int device, int on);           // on: 1 = one lane at a time. device >= 0: that device's self-check verdict; device < 0: the process-wide test hook (its 0 does NOT clear a verdict)

// ---- LZNT1 (lznt1.hip) ----
#define LZNT1_SLOT 4352u     // scratch bytes per 4 KiB chunk image (2 B header + <=4096 B payload + emit slack)
#define LZNT1_REC  5632u     // scratch bytes of parse records per 4 KiB chunk (four-wave kernel: match tokens of 64 windows, two areas)
// dev (here and below): a compress plan with device-built tables -- bt.n_chunks is its bound, and the chunk-gridded kernels return past
// chunk_prefix[n_units] (their DEV instances; host plans run the original ones). prepare_*: the one-time LDS attributes of a launcher's kernels.
void launch_lznt1_chunks(hipStream_t st, const uint8_t* d_in, const BatchTables& bt, uint8_t* slots, uint32_t* slot_size, uint16_t* recs, bool dev = false);
void launch_lznt1_sa_chunks(hipStream_t st, const uint8_t* d_in, const BatchTables& bt, uint8_t* slots, uint32_t* slot_size, bool dev = false);   // lznt1_sa.hip: the suffix-array dictionary flavour
void prepare_lznt1_sa(bool dev);

// ---- Xpress / Xpress+Huffman match finder (xpress_match.hip) ----
// links: u16 per position (64 KiB "link chunks", chunk-major), lasthead: 32768 u16 per link chunk,
// mlen3/moff: per position len-3 (capped at 48-3) and offset (0 = no match).
void launch_xp_links(hipStream_t st, const uint8_t* d_in, const BatchTables& bt, uint16_t* links, uint16_t* lasthead, bool dev = false);
void launch_xp_find(hipStream_t st, const uint8_t* d_in, const BatchTables& bt, const uint16_t* links, const uint16_t* lasthead,
                    uint16_t* mlen3, uint16_t* moff, uint32_t max_off, int clip, bool dev = false);
void prepare_xp_match(bool dev);
// the same over chunks [chunk_base, chunk_base + chunk_count) only (the pipelined one-shot call: a range's kernels run while the next range is on its way up)
void launch_xp_links_range(hipStream_t st, const uint8_t* d_in, const BatchTables& bt, uint16_t* links, uint16_t* lasthead, uint32_t chunk_base, uint32_t chunk_count, bool dev = false);
void launch_xp_find_range(hipStream_t st, const uint8_t* d_in, const BatchTables& bt, const uint16_t* links, const uint16_t* lasthead,
                          uint16_t* mlen3, uint16_t* moff, uint32_t max_off, int clip, uint32_t chunk_base, uint32_t chunk_count, bool dev = false);
// the lazy finder (xpress_lazy.hip): Find only where a greedy parse can start a token -- Xpress, every unit at most 64 KiB. Fills the same
// arrays for a superset of the true token starts; the offsets of all other positions are 0.
void launch_xp_lazy2(hipStream_t st, const uint8_t* d_in, const BatchTables& bt, const uint16_t* links, uint16_t* mlen3, uint16_t* moff, bool dev = false);
void prepare_xp_lazy2(bool dev);


// ---- Xpress stream emission (xpress_emit.hip): one wavefront per unit ----
int xpress_emit_mode_for(uint32_t n_units, uint32_t n_chunks);
// per-window / per-super-block records of the Xpress parse (see xpress_emit.hip); the last 10 only for the block-per-super-block kernels
struct XpressWinBufs { u64* wtok; u64* wmat; uint32_t* wfar; uint32_t* wecur; uint32_t* weF; uint32_t* wsum; uint32_t* wnr; uint32_t* ws0; uint32_t* ws1;
                       uint32_t* sbtot; u64* sbpre; uint32_t* seam; u64* seampos; uint32_t* used; };
void launch_xpress_emit(hipStream_t st, const uint8_t* d_in, const BatchTables& bt, uint16_t* mlen3, const uint16_t* moff,
                        const XpressWinBufs& wb, uint8_t* d_out, u64* d_out_len, int32_t* d_status, bool dev = false);

// ---- Xpress+Huffman chunk pipeline (xhuff.hip) ----
void launch_xh_parse(hipStream_t st, const uint8_t* d_in, const BatchTables& bt, uint16_t* mlen3, const uint16_t* moff,
                     u64* tokbits, uint32_t* counts, uint32_t* extra, bool dev = false);
void launch_xh_huff(hipStream_t st, const BatchTables& bt, const uint32_t* counts, const uint32_t* extra, uint8_t* lens, uint16_t* codes,
                    uint32_t* chunk_size, uint32_t* fb_list, uint32_t* fb_count, uint32_t* fbflag, bool dev = false);   // dev: fb_count zeroed by a kernel
void launch_xh_huff_debug(hipStream_t st, const uint32_t* counts, uint8_t* lens, uint32_t n);
void launch_xh_huff_slow_debug(hipStream_t st, const uint32_t* counts, uint8_t* lens, uint32_t n);   // counts on symbols 0..0x100 only
void launch_xh_fallback(hipStream_t st, const uint8_t* d_in, const BatchTables& bt, const uint32_t* fb_list, const uint32_t* fb_count,
                        uint32_t blocks, u64* tokbits, uint8_t* lens, uint16_t* codes, uint32_t* chunk_size);
void prepare_xh_fallback();
void launch_xh_encode(hipStream_t st, const uint8_t* d_in, const BatchTables& bt, const uint16_t* mlen3, const uint16_t* moff,
                      const u64* tokbits, const uint8_t* lens, const uint16_t* codes, const uint32_t* fbflag, const u64* prefix, uint8_t* d_out, bool dev = false);

// ---- decompressors: LZNT1 (lznt1_decode.hip) ----
// The compressed input of a unit is cut into segments of LZD_SEG bytes (chunk_prefix[u] = first segment of unit u, n_chunks =
// segments of the batch). cin: header offsets, LZD_SLOTS per segment (u32); segL / segE / segcnt / segstop / segoff per speculated
// chain; selcnt / seloff per segment (the true chain); flat: u64 exclusive scan of selcnt (n_chunks + 1) = number of the first chunk of a segment; csize: decoded size or 0x8000 per
// chunk number (u16); stop / irregular (+1 global flag) per unit.
// (LZD_SEG: common.h, beside decode_chunks)
#define LZD_HEAD  12288u
#define LZD_SLOTS (LZD_SEG / 3u + 2u)
#define LZD_K     8u         // speculated chains kept per segment
struct LzdBufs { uint32_t* cin; uint16_t* csize; uint32_t* segL; uint32_t* segE; uint32_t* segcnt; uint32_t* segstop; uint32_t* segoff;   /* LZD_K per segment */
                 uint32_t* selcnt; uint32_t* seloff; uint32_t* stop; uint32_t* irregular; u64* flat; };
// dev: a plan with device-built tables (bt.n_chunks is its bound; the blocks past chunk_prefix[n_units] return at once)
void launch_lzd_segments(hipStream_t st, const uint8_t* d_in, const BatchTables& bt, const LzdBufs& b, bool dev = false);
void prepare_lzd_segments(bool dev);                      // its one-time LDS attribute (a dev plan sets it when it is created: its first execution may be captured)
uint32_t lzd_read_walked();
void launch_lzd_verify(hipStream_t st, const uint8_t* d_in, const BatchTables& bt, const LzdBufs& b);
// lzd_chunk_kernel: every chunk decoded | the irregular units' chunks decoded again to their places | every chunk only sized (the size query)
void launch_lzd_chunks(hipStream_t st, const uint8_t* d_in, const BatchTables& bt, const LzdBufs& b, uint8_t* d_out);
void launch_lzd_replace(hipStream_t st, const uint8_t* d_in, const BatchTables& bt, const LzdBufs& b, uint8_t* d_out);
void launch_lzd_sizes(hipStream_t st, const uint8_t* d_in, const BatchTables& bt, const LzdBufs& b);
void launch_lzd_finalize(hipStream_t st, const BatchTables& bt, const LzdBufs& b, u64* d_out_len, int32_t* d_status, u64* d_need = nullptr);

// ---- decompressors: Xpress (xpress_decode.hip) ----
// xpd_kernel: one wave walks and copies one stream
void launch_xpress_decompress(hipStream_t st, const uint8_t* d_in, const BatchTables& bt, uint8_t* d_out, u64* d_out_len, int32_t* d_status);
// large Xpress streams by segments (xps_*): plan tables + scratch
#define XPS_SEG    16384u                                 // input bytes per segment (12 whole files, segment / warm-up KiB: 32/32 15.5 ms, 16/16 14.1, 8/8 19.6, 32/8 21.2)
#define XPS_WARM   16384u                                 // a speculative walk starts this far before its segment
#define XPS_SEG_BYTES 64u
#define XPS_ROUNDS 8u                                     // rounds of "walk the segments again that do not hold"
struct XpsTables {
	const uint32_t* unit;          // n_big: the streams taken
	const u64* seg_prefix;         // n_big + 1: first segment of each
	void*     seg;                 // per segment: 64 bytes of state (XpsSeg)
	uint32_t* mode;                // per stream taken: 1 rounds running, 2 done by segments, 0 left to the one-wave walk
	uint32_t* done;                // per unit of the batch: XPS_DONE when the one-wave walk has nothing to do
	uint32_t  n_big, n_seg;
	uint32_t  seg_bytes, warm_bytes; // input bytes per segment; a speculative walk starts this far before its segment (<= seg_bytes)
	const uint32_t* cnt;           // null: a host plan, n_big / n_seg are the counts. A dev plan with large units: n_big / n_seg are its bounds (grids,
	                               // scratch layout) and cnt[0] / cnt[1] the counts of this execution, written by its path pass (the DEV kernel instances read them)
};
// The same through 32-bit tokens, the large streams by segments first (the DEV instances when x.cnt is set; no launch when x.n_big == 0).
// walk: x.done zeroed, xps_init_kernel, xps_walk_kernel<0>, the speculative walks. redo: xps_check_kernel<false>, xps_walk_kernel<1>, one round of
// "walk the segments again that do not hold". emit: xps_check_kernel<true>, the verdict, and xps_emit_kernel<true>; size: xps_emit_kernel<false>, no stores.
void launch_xps_walk(hipStream_t st, const uint8_t* d_in, const BatchTables& bt, const XpsTables& x);
void launch_xps_redo(hipStream_t st, const uint8_t* d_in, const BatchTables& bt, const XpsTables& x, u64* ntok, u64* d_out_len, int32_t* d_status);
void launch_xps_emit(hipStream_t st, const uint8_t* d_in, const BatchTables& bt, const XpsTables& x, const u64* tok_prefix, uint32_t* tok, u64* ntok, u64* d_out_len, int32_t* d_status);
void launch_xps_size(hipStream_t st, const uint8_t* d_in, const BatchTables& bt, const XpsTables& x, u64* ntok, u64* d_out_len, int32_t* d_status);
// xpt_parse_kernel<true>, a wave per stream x.done does not mark (x.n_big == 0: every stream); size: <false>, every test, no token written (ntok: n_units counts)
void launch_xpt_parse(hipStream_t st, const uint8_t* d_in, const BatchTables& bt, const u64* tok_prefix, uint32_t* tok, u64* ntok, u64* d_out_len, int32_t* d_status, const XpsTables& x);
void launch_xpt_size(hipStream_t st, const uint8_t* d_in, const BatchTables& bt, u64* ntok, u64* d_out_len, int32_t* d_status, const XpsTables& x);

// ---- decompressors: Xpress+Huffman (xhuff_decode.hip) ----
// tok_prefix[u] = first token slot of unit u, cand_prefix[u] = first candidate slot (n_slots in all); per candidate slot: offset, next offset,
// reach, state, bytes, tokens, token offset. (XHC_TILE_BYTES: common.h, beside decode_chunks)
enum { XHC_SERIAL = 1, XHC_SPEC = 2 };
struct XhcBufs { uint32_t* cand_cnt; uint32_t* mode; uint32_t* cand_pos; uint32_t* res_end; uint32_t* res_reach; uint32_t* res_state;
                 u64* res_prod; u64* res_ntok; u64* tok_off;
                 const u64* scr_prefix; uint32_t* scr_tok; };   // token scratch: first scratch slot of every unit (n_units + 1; equal = none), XHC_SCR tokens per candidate
#define XHC_SCR 65600u                                    // a candidate gives up to 65536 tokens before its 65536th byte
// In the order they run. mark: xb.cand_cnt zeroed, xhc_mark_kernel lists the candidate chunk starts (dev: as launch_lzd_segments). candidates:
// xhc_parse_kernel<1> walks every candidate as one chunk; size: <3>, which only measures (no tokens written, chunk 0 included). chain: xhc_chain_kernel,
// per buffer. tokens: xhc_gather_kernel when there is token scratch, xhc_parse_kernel<2> for the accepted chunks. xhd: xhd_parse_kernel<true>, the
// serial walk of the buffers the speculation could not do (mode: xb.mode); size: <false>, tokens only counted.
void launch_xhc_mark(hipStream_t st, const uint8_t* d_in, const BatchTables& bt, const u64* cand_prefix, const XhcBufs& xb, bool dev);
void launch_xhc_candidates(hipStream_t st, const uint8_t* d_in, const BatchTables& bt, const u64* tok_prefix, const u64* cand_prefix, uint32_t n_slots, const XhcBufs& xb, uint32_t* tok);
void launch_xhc_candidates_size(hipStream_t st, const uint8_t* d_in, const BatchTables& bt, const u64* cand_prefix, uint32_t n_slots, const XhcBufs& xb);
void launch_xhc_chain(hipStream_t st, const BatchTables& bt, const u64* cand_prefix, const XhcBufs& xb, u64* ntok, u64* d_out_len, int32_t* d_status);
void launch_xhc_tokens(hipStream_t st, const uint8_t* d_in, const BatchTables& bt, const u64* tok_prefix, const u64* cand_prefix, uint32_t n_slots, const XhcBufs& xb, uint32_t* tok);
void launch_xhd_parse(hipStream_t st, const uint8_t* d_in, const BatchTables& bt, const u64* tok_prefix, uint32_t* tok, u64* ntok, u64* d_out_len, int32_t* d_status, const uint32_t* mode);
void launch_xhd_size(hipStream_t st, const uint8_t* d_in, const BatchTables& bt, u64* ntok, u64* d_out_len, int32_t* d_status, const uint32_t* mode);

// ---- tokens -> bytes of both Xpress formats (lz_copy.hip): lz_copy_kernel, a wave per unit, and lz_copy_block_kernel, a block per larger one ----
// Units of lzg_min_cap output bytes and more are left to lzglobal.hip; with lzg_cnt (a dev plan with large units) the DEV instances, which leave the
// units of LZG_MIN_CAP and more when lzg_cnt[0] != 0
#define LZB_MIN_KB 32                                     // units with at least this much output take the block kernel (MSCOMP_AMD_LZB_MIN_KB overrides, for measurements): a wave per unit, lz_copy_kernel, takes 3.8 ms for a 64 KiB unit; the block 57 us: 3 239 units 4.0 -> 1.6 ms
void launch_lz_copy(hipStream_t st, const BatchTables& bt, const u64* tok_prefix, const uint32_t* tok, const u64* ntok, const u64* d_out_len, const int32_t* d_status, uint8_t* d_out, u64 lzg_min_cap, const uint32_t* lzg_cnt);
void launch_lz_copy_block(hipStream_t st, const BatchTables& bt, const u64* tok_prefix, const uint32_t* tok, const u64* ntok, const u64* d_out_len, const int32_t* d_status, uint8_t* d_out, u64 lzg_min_cap, const uint32_t* lzg_cnt);
void prepare_lz_copy_block();                             // the one-time LDS attribute of lz_copy_block_kernel

// ---- tokens -> bytes for large units by all CUs (lzglobal.hip) ----
#define LZG_PASSES 33u                                    // pointer passes launched (chains halve at least: 2^32 bytes); a pass returns at once when the one before left nothing open
// (LZG_TILE_SHIFT, LZG_MIN_CAP: common.h, beside lzg_takes; XPS_MIN_IN there too)
struct LzgTables {
	const uint32_t* unit;          // n_big: the units taken
	const u64* tb_prefix;          // n_big + 1: first token block (8192 tokens) of each
	const u64* tile_prefix;        // n_big + 1: first tile (8192 output bytes) of each
	const u64* word_prefix;        // n_big + 1: first word of each in `words`
	u64*      bsum;                // per token block: bytes its tokens give; then the bytes before it
	uint32_t* dir_tok;             // per tile: the first token that starts in the tile or behind it ...
	uint32_t* dir_pos;             // ... and where
	uint32_t* words;               // per output byte: LZG_VAL | byte, or the index of its source
	uint32_t* open;                // LZG_PASSES counters: words still pointing after each pass
	uint8_t*  tile_pass;           // per tile: the pointer pass that has to look at it next (0xFF: none)
	uint32_t  n_big, n_tb, n_tiles;
	const uint32_t* cnt;           // as XpsTables::cnt: cnt[0] units taken (0: the stage does not run in this execution), cnt[1] token blocks, cnt[2] tiles
};
void prepare_lz_copy_global(bool dev);                    // the one-time LDS attribute of lzg_expand_kernel (a dev plan sets it when it is created, as prepare_lzd_segments)
// directory: g.open zeroed, lzg_sums_kernel, lzg_scan_kernel, lzg_dir_kernel; expand: lzg_expand_kernel; jump: LZG_PASSES launches of lzg_jump_kernel.
// Each picks the DEV instances from g.cnt and launches nothing when g.n_big == 0.
void launch_lzg_directory(hipStream_t st, const LzgTables& g, const u64* tok_prefix, const uint32_t* tok, const u64* ntok, const u64* d_out_len, const int32_t* d_status);
void launch_lzg_expand(hipStream_t st, const LzgTables& g, const BatchTables& bt, const u64* tok_prefix, const uint32_t* tok, const u64* ntok, const u64* d_out_len, const int32_t* d_status, uint8_t* d_out);
#define LZG_HOPS 8u                                       // hops per pointer pass (MSCOMP_AMD_LZG_HOPS overrides, for measurements)
void launch_lzg_jump(hipStream_t st, const LzgTables& g, const BatchTables& bt, const u64* d_out_len, const int32_t* d_status, uint8_t* d_out);

// ---- plans with device-built tables (devplan.hip) ----
// One block walks the units in tiles of 1024: per unit, the checks of mscomp_amd_plan_execute_dev (in_len <= 0xFFFFF000, running totals of
// in_len / out_cap within the bounds), the unit's table row (in_off | in_len | out_off | out_cap; all zero for a rejected unit) in san
// (4 x n), reject[u], and the prefix arrays of the chunk counts (u32, n + 1 entries), the token slots and the candidate slots (u64, n + 1
// each, the candidate prefix right behind the token prefix) with the counts plan_create_impl uses on the host (common.h).
void launch_dev_tables(hipStream_t st, int format, uint32_t n, u64 in_total_max, u64 out_total_max, const u64* in_off, const u64* in_len,
                       const u64* out_off, const u64* out_cap, u64* san, uint32_t* chunk_prefix, u64* tok_prefix, uint32_t* reject);
// The path pass of a dev plan with large units (MSCOMP_AMD_DEV_LARGE_UNITS), one block behind the table pass: from the sanitised rows, the
// tables plan_create_impl builds on the host for the optional paths, with the same arithmetic (common.h). Each of the three parts is off
// when its first pointer is null.
struct DevPaths {
	uint32_t* xps_unit; u64* xps_seg_prefix; uint32_t* xps_cnt;       // Xpress streams walked by segments: units in unit order, first segment of each, {units, segments}
	uint32_t  xps_seg_bytes, xps_max, xps_seg_max;                    // (*_max: the entries the lists and the scratch were reserved for)
	uint32_t* lzg_unit; u64* lzg_tb_prefix; u64* lzg_tile_prefix; u64* lzg_word_prefix; uint32_t* lzg_cnt;   // the all-CU byte stage: {units, token blocks, tiles}, all 0 when the stage is off for the batch
	uint32_t  lzg_max; u64 lzg_tb_max, lzg_tile_max, lzg_word_max;
	u64*      scr_prefix;                                             // Xpress+Huffman: first token-scratch slot of every unit (n + 1)
};
void launch_dev_paths(hipStream_t st, int format, uint32_t n, const u64* san, const DevPaths& dp);
// size plans (mscomp_amd_plan_create_size_dev): the same pass with out_off = 0 and out_cap = limit for every unit (limit null: 2^64 - 1) and
// no bound on the limits' sum; the prefix arrays are those of a host size plan with these values
void launch_dev_stables(hipStream_t st, int format, uint32_t n, u64 in_total_max, const u64* in_off, const u64* in_len, const u64* limit,
                        u64* san, uint32_t* chunk_prefix, u64* tok_prefix, uint32_t* reject);
// the last launch of a size dev plan: units with reject[u] get MSCOMP_ARG_ERROR, length 0, need 0; copy_need: need = length for the others
void launch_dev_size_finish(hipStream_t st, const uint32_t* reject, uint32_t n, u64* d_out_len, u64* d_need, int32_t* d_status, bool copy_need);
// mscomp_amd_compact_dev: off[0..n] as launch_layout_dev(len, align), then the len[u] bytes at src + src_off[u] to packed + off[u], the
// padding between units zeroed, nothing at or behind packed + cap; `blocks` = the fixed grid of the copy, compact_dev_blocks() of the device
uint32_t compact_dev_blocks();
void launch_compact_dev(hipStream_t st, uint32_t n, const uint8_t* src, const u64* src_off, const u64* len, u64 align, uint8_t* packed, u64 cap,
                        u64* off, uint32_t blocks);
// the copy of mscomp_amd_compact_dev with a source address per unit (src_ptr[u], for len[u] bytes) and offsets that are already there
// (off[0..n], growing, off[n] = total): what a block container packs, its blocks lying in the staging area or in the caller's input
void launch_pack_ptrs(hipStream_t st, uint32_t n, const u64* src_ptr, const u64* len, const u64* off, uint8_t* packed, u64 cap, uint32_t blocks);
// p[0..n) = 0 as a kernel (a dev plan's launches hold no memset: they go into graphs the caller captures)
void launch_dev_zero(hipStream_t st, uint32_t* p, uint32_t n);
// units with reject[u]: status MSCOMP_ARG_ERROR, length 0 (after the decoders, which saw them as empty units with no room)
void launch_dev_reject(hipStream_t st, const uint32_t* reject, uint32_t n, u64* d_out_len, int32_t* d_status);
// off[0..n] = exclusive running sum of cap[i] rounded up to align (saturating at 2^64 - 1)
void launch_layout_dev(hipStream_t st, const u64* cap, uint32_t n, u64 align, u64* off);
// compress plans (mscomp_amd_plan_create_compress_dev): per unit the checks in_len <= in_unit_max and running total of in_len <= in_total_max,
// the sanitised row in san (as above), reject[u], and chunk_prefix (u32, n + 1) with compress_chunks(format, L): 4 KiB chunks for LZNT1,
// 64 KiB for the Xpress formats, none for an empty or a rejected unit
void launch_dev_ctables(hipStream_t st, int format, uint32_t n, u64 in_total_max, u64 in_unit_max, const u64* in_off, const u64* in_len,
                        const u64* out_off, const u64* out_cap, u64* san, uint32_t* chunk_prefix, uint32_t* reject);
// mscomp_amd_plan_layout_dev: cap[i] = the format's largest output for in_len[i] (cap may be null), off[0..n] as launch_layout_dev
void launch_clayout_dev(hipStream_t st, int format, const u64* in_len, uint32_t n, u64 align, u64* off, u64* cap);

// ---- block containers (blocks.hip; mscomp_amd_blocks_*) ----
// a fixed grid: the workgroups that `items` need at per_block each, `blocks` at most (a kernel on one walks its items with the grid's stride)
inline dim3 fixed_grid(u64 items, uint32_t per_block, uint32_t blocks)
{
	const u64 need = (items + per_block - 1u) / per_block;
	return dim3((uint32_t)(need < blocks ? need : blocks));
}
// the passes tiled over the rows of a table -- of splice by extents, of a transcoder, and the run passes of diff, match and repair (rowpass.h)
#define ROW_TILE DV_THREADS                            // rows per workgroup (MSCOMP_AMD_SPLICE_ROW_TILE)
inline uint32_t row_tiles(uint32_t rows) { return (rows + ROW_TILE - 1u) / ROW_TILE; }
// The container's own tables, in one buffer (blockobj.hip blocks_tab is the only place that knows the layout). n = resources, m = the bound of
// the blocks; the seven unit columns are what the inner dev plans read and write, with the container's blocks (compress) or the blocks in
// range (decompress) as units.
struct BlocksTab {
	u64* res_a;                                        // n: compress, where a resource's blocks are staged; decompress, the bytes its range stands for
	u64* res_b;                                        // n: decompress, first block of the clipped range
	u64* unit_first;                                   // n + 1: decompress, first unit of every resource
	u64 *in_off, *in_len, *out_off, *out_cap;          // m each: the inner plan's unit tables
	u64* ulen;                                         // m: the inner plan's d_out_len
	u64 *aux_a, *aux_b;                                // m each: compress, stored length | source address; decompress, raw block's offset in packed | in out
	int32_t* rstat;                                    // n: the resource's own status (bounds, block count, capacity)
	int32_t* ustat;                                    // m: the inner plan's d_status
	uint32_t* act;                                     // m: decompress, kind | data length << 2; crc, the block's resource
	uint32_t* ucrc;                                    // m: check, the CRC-32 of every block read; crc, x^(8 bytes of the resource behind the block)
};
// compress, in front of the inner plan: bounds check, block_first (n_res + 1) and the unit tables (two launches: one block over the resources,
// one thread per possible block)
void launch_blocks_ctables(hipStream_t st, uint32_t n_res, uint32_t nbmax, uint32_t shift, u64 in_max, const u64* res_off, const u64* res_len,
                           u64* block_first, const BlocksTab& t);
// compress, behind it: stored form per block (t.aux_a / t.aux_b for launch_pack_ptrs), block_off (nbmax + 1), d_status (one block)
void launch_blocks_select(hipStream_t st, uint32_t n_res, uint32_t nbmax, u64 cap, const uint8_t* d_in, const uint8_t* stage, const u64* block_first,
                          const BlocksTab& t, u64* block_off, int32_t* d_status);
// decompress, in front of the inner plan: the per-resource checks and the range, then unit tables and action words (two launches)
void launch_blocks_dtables(hipStream_t st, uint32_t n_res, uint32_t nbmax, uint32_t shift, u64 in_max, u64 packed_len, const u64* res_len,
                           const u64* block_first, const u64* block_off, const u64* range, const u64* d_out_off, const u64* d_out_cap, const uint32_t* only,
                           const BlocksTab& t);
// decompress, behind it: raw blocks to their places (`blocks` = compact_dev_blocks()), then status and length per resource
void launch_blocks_rawcopy(hipStream_t st, uint32_t nbmax, uint32_t shift, const uint8_t* packed, uint8_t* out, const BlocksTab& t, uint32_t blocks);
void launch_blocks_dfold(hipStream_t st, uint32_t n_res, const BlocksTab& t, u64* d_out_len, int32_t* d_status);
// salvage (mscomp_amd_blocks_salvage): launch_blocks_dtables with range null and `only` = the mask over the container's rows (may be null: the
// rows it marks SV_GOOD become empty units), the inner plan and launch_blocks_rawcopy as decompress runs them, then four passes of its own.
// The verdict of a row (MSCOMP_AMD_BLOCK_*):
#define SV_GOOD    0u
#define SV_TABLE   1u
#define SV_DECODE  2u
#define SV_CRC     3u
#define SV_SKIPPED 4u
// units: the CRC columns over the blocks in d_out that can be read (t.in_off = where every unit's block lies, t.in_len), t.out_off = the
// unit's row, verdict (nbmax) all SV_SKIPPED, count (4) cleared. t.ustat, t.ulen and t.act stay as the inner plan and the table pass left them
void launch_blocks_sunits(hipStream_t st, uint32_t n_res, uint32_t nbmax, uint32_t shift, const u64* block_first, const u64* d_out_off, const BlocksTab& t,
                          uint32_t* verdict, u64* count);
// behind the CRC kernels (block_crc null: behind the pass above): the judged rows' verdicts into verdict and, per unit, into t.ucrc
void launch_blocks_sverdict(hipStream_t st, uint32_t n_res, uint32_t nbmax, const uint32_t* block_crc, const BlocksTab& t, uint32_t* verdict);
// the judged bad rows zeroed in d_out (`blocks` = compact_dev_blocks()), then length, bad rows and status per resource and the counts
void launch_blocks_szero(hipStream_t st, uint32_t nbmax, uint32_t shift, uint8_t* out, const BlocksTab& t, uint32_t blocks);
void launch_blocks_sfold(hipStream_t st, uint32_t n_res, const BlocksTab& t, u64* d_out_len, uint32_t* d_bad, int32_t* d_status, u64* count);
// crc, behind launch_blocks_ctables: per block its resource (t.act) and the resource's bytes behind it (t.ulen), for launch_crc_units
void launch_blocks_crcgroups(hipStream_t st, uint32_t n_res, uint32_t nbmax, uint32_t shift, const u64* res_len, const u64* block_first, const BlocksTab& t);
// check, in front of the CRC kernels: checks 1 and 2 and the clipped range of the resources that are MSCOMP_OK in d_status (t.unit_first, t.res_b,
// t.rstat), then per unit where the block lies in the output (t.in_off, t.in_len) and its entry of d_block_crc (t.ulen); behind them: the verdicts
#define BK_LEAVE 1                                        // (t.rstat of a resource that was not MSCOMP_OK on entry to check: not a status)
void launch_blocks_ktables(hipStream_t st, uint32_t n_res, uint32_t nbmax, uint32_t shift, u64 in_max, const u64* res_len, const u64* block_first,
                           const u64* range, const u64* d_out_off, const int32_t* d_status, const BlocksTab& t);
// (an entry is `words` words, 1 or 4: `read` holds the units' entries as they were computed -- t.ucrc, or a digester's d.out --, `given` the caller's column)
void launch_blocks_kfold(hipStream_t st, uint32_t n_res, const uint32_t* read, const uint32_t* given, uint32_t words, const BlocksTab& t, u64* d_out_len, int32_t* d_status);
// the last pass of a write, a resize and a splice: every row of the new table (nbt) with a non-zero addr[row] to dst + new_off[row], runs of rows
// whose addr - new_off is constant as one copy; nothing at or behind dst + cap (`blocks` = compact_dev_blocks())
void launch_blocks_move(hipStream_t st, uint32_t nbt, u64 cap, const u64* new_off, const u64* addr, uint8_t* dst, uint32_t blocks);

// ---- block readers (reader.hip; mscomp_amd_reader_*) ----
// The reader's own tables, in one buffer (blockobj.hip access_tab is the only place that knows the layout). n = requests, m = blocks_max: the
// bound of the units, a unit being one (request, covering block) pair of an admitted request; nbt = the entries of the container's block table.
struct ReaderTab {
	u64 *q_off, *q_want, *q_j0, *q_len;                // n each: clipped offset, bytes wanted, container index of the first covering block, the resource's length
	u64* unit_first;                                   // n + 1: first unit of every request
	int32_t* q_stat;                                   // n: the request's own status (checks 1-5), then -- behind the fold -- its final one
	u64 *in_off, *in_len, *out_off, *out_cap, *ulen;   // m each: the inner plan's unit tables and d_out_len (only an owner that is decoded has a length)
	u64* src;                                          // m: an owner's block, as an address: its cache slot, or its place in d_packed when stored raw
	u64 *clen, *cum;                                   // m, m + 1: the bytes the CRC kernel reads of every unit (an owner that passed the table checks: e) and their running sum
	int32_t* ustat;                                    // m: the inner plan's d_status
	uint32_t *act, *owner, *uq, *ublk, *ucrc;          // m each: kind | data length << 2; the unit that owns this unit's block; its request; its block; the CRC-32 read
	uint32_t* own;                                     // nbt: per block of the container the bid of its owner (~unit, 0 = nobody)
	uint32_t* cnt;                                     // 2: distinct blocks of the last execution, and those that were decoded
};
// checks 1-5 per request, the clipped ranges and unit_first (one block). out_cap null: without check 4 (a block writer's admission)
void launch_reader_requests(hipStream_t st, uint32_t n_req, uint32_t n_res, uint32_t nbt, uint32_t m, uint32_t shift, const u64* res_len,
                            const u64* block_first, const u64* req, const u64* out_cap, const ReaderTab& t);
// behind it: t.own cleared, one owner per covering block, then the table checks and the inner plan's unit tables (three launches)
void launch_reader_units(hipStream_t st, uint32_t n_req, uint32_t nbt, uint32_t m, uint32_t shift, u64 packed_len, const uint8_t* packed,
                         const uint8_t* cache, const u64* block_off, const ReaderTab& t);
// behind the inner plan and the CRC kernels: status and length per request (block_crc may be null), then the slices of the MSCOMP_OK
// requests to d_out (`blocks` = compact_dev_blocks())
void launch_reader_fold(hipStream_t st, uint32_t n_req, const uint32_t* block_crc, const ReaderTab& t, u64* d_out_len, int32_t* d_status);
void launch_reader_gather(hipStream_t st, uint32_t n_req, uint32_t m, uint32_t shift, uint8_t* out, const u64* out_off, const ReaderTab& t, uint32_t blocks);

// ---- block searchers (search.hip; mscomp_amd_searcher_*, include/mscomp_amd_search.h) ----
// A searcher admits, shares, decodes and judges with the reader's passes on a ReaderTab of its own -- its admission counts the blocks of
// the look-ahead too --, and scans where the reader gathers. Its own columns (blockobj.hip search_tab knows the layout): an item is one
// (unit, tile) pair, tile = SR_TILE positions of the unit's block, item = (unit << (shift - SR_TILE_SHIFT)) + tile.
#define SR_PAT_MAX    64u                                 // MSCOMP_AMD_SEARCH_PAT_MAX: one bit of a mask word per pattern
#define SR_LEN_MAX    256u                                // MSCOMP_AMD_SEARCH_LEN_MAX
#define SR_TILE_SHIFT 12u                                 // the smallest block: a tile never spans two blocks
#define SR_TILE       (1u << SR_TILE_SHIFT)
struct SearchTab {
	u64* mask;                                         // 4 x 256: mask[k][b], bit p = pattern p has byte b at position k or is shorter than k + 1; a refused pattern has no bit
	u64* aux;                                          // 8: [a], a < 4: the patterns of length 1 .. a; [4]: those longer than 4 (the filter does not settle them)
	u64* poff;                                         // SR_PAT_MAX: d_pat_off[p]
	u64* first;                                        // items + 1: hits per item from the count pass, then their running sum (the item's first record)
	uint32_t* plen;                                    // SR_PAT_MAX: the pattern's length, 0 for a refused one and behind n_pat
};
// admission: launch_reader_requests without the capacity rule, the budget counting the blocks that cover `look` more bytes (one block)
void launch_search_requests(hipStream_t st, uint32_t n_req, uint32_t n_res, uint32_t nbt, uint32_t m, uint32_t shift, uint32_t look, const u64* res_len,
                            const u64* block_first, const u64* req, const ReaderTab& t);
// the patterns validated (pat_status), s.mask, s.aux, s.poff, s.plen (one block)
void launch_search_patterns(hipStream_t st, uint32_t n_pat, uint32_t len_max, const uint8_t* pat, const u64* pat_off, const SearchTab& s, int32_t* pat_status);
// behind the fold: the hits per item (a fixed grid of `blocks` dealt over the items, a wave per item), their running sum with req_hits
// and count (one block, then a thread per request), the records below hits_max (the fixed grid again)
void launch_search_count(hipStream_t st, uint32_t n_req, uint32_t m, uint32_t shift, uint32_t n_pat, uint32_t len_max, const uint8_t* pat, const SearchTab& s, const ReaderTab& t,
                         uint32_t blocks);
void launch_search_sum(hipStream_t st, uint32_t n_req, uint32_t shift, u64 hits_max, const SearchTab& s, const ReaderTab& t, u64* req_hits, u64* count);
void launch_search_emit(hipStream_t st, uint32_t n_req, uint32_t m, uint32_t shift, uint32_t n_pat, uint32_t len_max, u64 hits_max, const uint8_t* pat, const SearchTab& s,
                        const ReaderTab& t, u64* hits, uint32_t blocks);

// ---- block writers (writer.hip; mscomp_amd_writer_*) ----
// A writer admits, shares, decodes and judges with the reader's passes, on a ReaderTab of its own, and adds four columns to it
// (blockobj.hip access_tab knows the layout).
struct WriterTab {
	ReaderTab r;                                       // (r.cnt has four words here: [2] = dirty blocks, [3] = 1 when the table as a whole was refused)
	uint32_t* head;                                    // nbt: the last unit that joined a block's list, + 1 (0 = none)
	uint32_t* next;                                    // m: the unit that joined the list before this one, + 1
	uint32_t* dirty;                                   // m: 1 for an owner whose block an MSCOMP_OK request covers
	u64* addr;                                         // nbt: from the layout pass, where a new row's stored bytes lie (0 = nothing to move): launch_blocks_move
};
// behind launch_reader_units: t.head cleared, every unit linked to its block (two launches)
void launch_writer_link(hipStream_t st, uint32_t n_req, uint32_t nbt, uint32_t m, const WriterTab& t);
// behind the fold: raw owners loaded into the cache, the MSCOMP_OK requests applied in request order, t.dirty; then the unit tables of the inner
// compress plan (r.in_off .. r.out_cap) and of the CRC kernels (r.src, r.clen) over the dirty owners (two launches; `blocks` = compact_dev_blocks())
void launch_writer_patch(hipStream_t st, uint32_t n_req, uint32_t m, uint32_t shift, const uint8_t* src, const u64* src_off, uint8_t* cache,
                         const WriterTab& t, uint32_t blocks);
// behind the compress plan and the CRC kernels, one block: rule 0, new_off (nbt + 1), new_crc (nbt, may be null with block_crc), t.addr (clean
// blocks in packed, dirty ones in stage or cache), d_res_status, and -- for a refused table -- d_status and d_written
void launch_writer_layout(hipStream_t st, uint32_t n_req, uint32_t n_res, uint32_t nbt, uint32_t m, uint32_t shift, u64 packed_len, u64 cap, const uint8_t* packed,
                          const uint8_t* stage, const uint8_t* cache, const u64* block_first, const u64* block_off, const uint32_t* block_crc, const WriterTab& t,
                          u64* new_off, uint32_t* new_crc, u64* d_written, int32_t* d_status, int32_t* d_res_status);

// mscomp_amd_writer_resize, the writer's second call: the same tables, and two columns per resource behind them. A unit is a block whose
// data changes: the changed block of an admitted resource (its unit 0, when there is one), then its fresh blocks in order. Of the unit
// columns r.uq is the unit's resource, r.ublk its block within the resource, r.owner the data length e2 it will have, r.act kind | e << 2 of
// a changed block (RD_SKIP for a fresh one); r.cnt: [0] changed blocks, [2] blocks encoded, [3] = 1 for a refused table.
struct ResizeTab {
	WriterTab w;
	u64* ru_first;                                     // n_res + 1: first unit of every resource
	int32_t* rstat;                                    // n_res: the resource's status by rules 1 and 3, then -- behind the fold -- by rule 4 too
};
// rules 0-3 and ru_first (one block), then the units' rows: the changed blocks' table checks and the inner decompress plan's unit tables
void launch_resize_units(hipStream_t st, uint32_t n_res, uint32_t nbt, uint32_t m, uint32_t shift, u64 packed_len, const uint8_t* packed, const uint8_t* cache,
                         const u64* block_first, const u64* block_off, const u64* res_len, const u64* want, const ResizeTab& t);
// behind the decompress plan and the CRC kernels: rule 4 per resource (block_crc may be null)
void launch_resize_fold(hipStream_t st, uint32_t n_res, uint32_t m, uint32_t shift, const u64* block_first, const u64* res_len, const u64* want,
                        const uint32_t* block_crc, const ResizeTab& t);
// the new data of the accepted resources' units in their cache slots (kept bytes, then zeros), then the unit tables of the inner compress plan
// and of the CRC kernels over them (two launches; `blocks` = compact_dev_blocks())
void launch_resize_fill(hipStream_t st, uint32_t n_res, uint32_t m, uint32_t shift, uint8_t* cache, const ResizeTab& t, uint32_t blocks);
// behind the compress plan and the CRC kernels, one block: new_first (n_res + 1), rule 8, new_off (nbt + 1), new_crc (nbt, may be null with
// block_crc), t.w.addr per NEW row (clean ones at their old row in packed, dirty ones in stage or cache), new_len and res_status (n_res)
void launch_resize_layout(hipStream_t st, uint32_t n_res, uint32_t nbt, uint32_t shift, u64 packed_len, u64 cap, const uint8_t* packed, const uint8_t* stage,
                          const uint8_t* cache, const u64* block_first, const u64* block_off, const u64* res_len, const u64* want, const uint32_t* block_crc,
                          const ResizeTab& t, u64* new_first, u64* new_off, uint32_t* new_crc, u64* new_len, int32_t* res_status);

// ---- block splicers (splice.hip; mscomp_amd_splicer_*) ----
// One source container of a splice as the kernels take it (the fields of mscomp_amd_blocks_view), and the sources of a call: they travel by
// value in the kernel arguments, the unused ones zeroed.
struct SpliceView {
	const uint8_t* packed; u64 packed_len;
	const u64* first; const u64* off; const u64* res_len;  // n_res + 1, nbt + 1, n_res
	const uint32_t* crc;                               // nbt (read only when the new container gets checksums)
	u64 n_res, nbt;
};
struct SpliceSrc { SpliceView v[4]; };
// source s of the call (s < n_src <= 4), by selects over four arguments: an array indexed with a lane's s would be copied into scratch memory
#define SP_PICK(f) (s == 1u ? v1.f : s == 2u ? v2.f : s == 3u ? v3.f : v0.f)
__device__ __forceinline__ SpliceView sp_view(const SpliceView& v0, const SpliceView& v1, const SpliceView& v2, const SpliceView& v3, u64 s)
{
	return SpliceView{ SP_PICK(packed), SP_PICK(packed_len), SP_PICK(first), SP_PICK(off), SP_PICK(res_len), SP_PICK(crc), SP_PICK(n_res), SP_PICK(nbt) };
}
#undef SP_PICK
// The same for a kernel that takes the sources as ONE argument, a SpliceSrc by value: the compiler then reads a view's field where it lies,
// in the kernel-argument segment, at the lane's s -- no scratch copy, and not all four views held in scalar registers for the selects (64
// of 106: the kernels of dedup.hip and match.hip that did spilled up to 38 of them)
__device__ __forceinline__ const SpliceView& sp_view(const SpliceSrc& src, u64 s) { return src.v[s]; }
// Shared by dedup.hip and match.hip. Global resource g (< n0 + n1 + n2 + n3) as source and resource: the sources' resources are numbered
// back to back
__device__ __forceinline__ void dd_locate(const SpliceView& v0, const SpliceView& v1, const SpliceView& v2, u64 g, u64& s, u64& r)
{
	s = 0; r = g;
	if (r >= v0.n_res) { r -= v0.n_res; s = 1; if (r >= v1.n_res) { r -= v1.n_res; s = 2; if (r >= v2.n_res) { r -= v2.n_res; s = 3; } } }
}
__device__ __forceinline__ void dd_locate(const SpliceSrc& src, u64 g, u64& s, u64& r) { dd_locate(src.v[0], src.v[1], src.v[2], g, s, r); }
__device__ __forceinline__ u64 dd_mix(u64 x)                // (splitmix64's finaliser)
{
	x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 27; x *= 0x94D049BB133111EBull; x ^= x >> 31;
	return x;
}
// the first min(16, len) stored bytes of a row in w[0], w[1] and the last min(16, len) in w[2], w[3]: the part of a key tuple that is data
__device__ __forceinline__ void dd_edges(const uint8_t* __restrict__ p, u64 len, u64 (&w)[4])
{
	w[0] = w[1] = w[2] = w[3] = 0;
	if (len >= 16u) {
		const cpd_u16 a = *reinterpret_cast<const cpd_u16*>(p), b = *reinterpret_cast<const cpd_u16*>(p + len - 16u);
		w[0] = a.w[0] | (u64)a.w[1] << 32; w[1] = a.w[2] | (u64)a.w[3] << 32; w[2] = b.w[0] | (u64)b.w[1] << 32; w[3] = b.w[2] | (u64)b.w[3] << 32;
	} else {
		for (uint32_t i = 0; i < (uint32_t)len; ++i) { w[i >> 3] |= (u64)p[i] << ((i & 7u) * 8u); }
		w[2] = w[0]; w[3] = w[1];
	}
}
// the key of a row, mixed into the caller's seed h: its stored length, its CRC word (bit 32 set) when checksums take part, and the edges
// of its len stored bytes at p
__device__ __forceinline__ u64 row_key(u64 h, u64 len, uint32_t with_crc, uint32_t crc, const uint8_t* __restrict__ p)
{
	u64 w[4];
	dd_edges(p, len, w);
	h = dd_mix(h ^ len);
	if (with_crc) { h = dd_mix(h ^ ((u64)crc | (u64)1 << 32)); }
	h = dd_mix(h ^ w[0]); h = dd_mix(h ^ w[1]); h = dd_mix(h ^ w[2]); h = dd_mix(h ^ w[3]);
	return h;
}
// one block: rules 1-3 per pick (pick: 2 n_pick, source and resource), new_first (n_pick + 1), new_len and status (n_pick), then per NEW row
// new_off (nbt + 1), new_crc (nbt, may be null) and addr (nbt, for launch_blocks_move), then rule 7
void launch_splice_layout(hipStream_t st, const SpliceSrc& src, uint32_t n_src, uint32_t n_pick, uint32_t nbt, uint32_t shift, u64 cap, const u64* pick,
                          u64* new_first, u64* new_off, uint32_t* new_crc, u64* new_len, int32_t* status, u64* addr);

// mscomp_amd_splicer_splice_extents: a new resource is a list of extents (source, resource, first block, block count). The splicer's
// scratch for it (blockobj.hip splice_ext_tab knows the layout):
struct SpliceExtTab {
	u64* addr;                                         // nbt: where a new row's stored bytes lie (0 = nothing to move): launch_blocks_move
	u64* ext_row;                                      // n_ext + 1: the running counts of the extent pass, then every extent's first new row
	u64* tsum;                                         // row_tiles(nbt): the stored bytes of a tile of rows, then their running sum
	uint32_t* flag;                                    // 1: the extent table as a whole was refused (rule 0)
};
// the extent pass (one block): rules 0-6, new_first (n_res + 1), new_len and status (n_res), new_off[0], t.ext_row, t.flag
void launch_splice_extents(hipStream_t st, const SpliceSrc& src, uint32_t n_src, uint32_t n_res, uint32_t n_ext, uint32_t nbt, uint32_t shift, const u64* ext_first,
                           const u64* ext, u64* new_first, u64* new_off, u64* new_len, int32_t* status, const SpliceExtTab& t);
// behind it, the three-launch scan over the NEW table's rows in tiles of ROW_TILE (nbt > 0). tiles: per row its stored length (left in
// new_off[row + 1]), new_crc (nbt, may be null) and t.addr, per tile its sum; tilescan (one block): the running sum of the tile sums; rows:
// new_off (nbt + 1) and the capacity rule
void launch_splice_tiles(hipStream_t st, const SpliceSrc& src, uint32_t n_res, uint32_t nbt, const u64* ext_first, const u64* ext, const u64* new_first, u64* new_off,
                         uint32_t* new_crc, const SpliceExtTab& t);
void launch_splice_tilescan(hipStream_t st, uint32_t nbt, const SpliceExtTab& t);
void launch_splice_rows(hipStream_t st, uint32_t n_res, uint32_t nbt, u64 cap, const u64* ext_first, const u64* new_first, u64* new_off, uint32_t* new_crc, int32_t* status,
                        const SpliceExtTab& t);

// ---- the key table of dedup, match and sync ("The key table"; its device functions: rowpass.h kt_*) ----
// Open addressing over 64-bit keys, with the smallest item of every key. The carve functions of blockobj.hip size it: more slots than
// there can be keys, 2^32 at most -- a slot is named by a 32-bit word, and all-ones is no slot. (Only a syncer for more than 2^30 store
// blocks has 2^32 slots. A key whose walk ends on the last of them has no slot, in claim and find alike: its blocks are not found.)
#define KT_NONE 0xFFFFFFFFu                                // no slot (a walk that found none); in `min`: no item yet
struct KeyTable {
	u64* key;                                          // slots: the key a slot was claimed for (0 = empty)
	uint32_t* min;                                     // slots: the smallest item that came with the slot's key
	u64 slots;
};
// every slot empty (a fixed grid over the slots; `blocks` = crc_dev_blocks())
void launch_dedup_clear(hipStream_t st, const KeyTable& kt, uint32_t blocks);

// ---- block dedupers (dedup.hip; mscomp_amd_deduper_*) ----
// The deduper's own tables, in one buffer (blockobj.hip dedup_tab is the only place that knows the layout). n = n_res_total, the bound of
// the resources of all sources together; the key table has 2 n + 64 slots, its items are resources.
struct DedupTab {
	u64* ufirst;                                       // n + 1: first row of every resource, in a numbering of the rows of the resources that passed rules 1 and 2
	u64* key;                                          // n: the resource's 64-bit key
	KeyTable kt;
	uint32_t *slot_of, *cand, *flag;                   // n each: the resource's slot (KT_NONE: none); the smallest accepted resource with its key; 1 = not equal to that one
	uint32_t* rlist;                                   // n: the refuted resources, ascending
};
// The call in four stages, eight launches fixed by n_max and rows_max (the creation bounds; every grid is sized by them, none is launched
// with an empty one); n = the resources of this call (<= n_max), status = d_status, which the stages read back.
// judge: the key table cleared, rules 1 and 2 and the row numbering (one block), rule 3 (a fixed grid over the rows); `blocks` = crc_dev_blocks()
void launch_dedup_judge(hipStream_t st, const SpliceSrc& src, uint32_t n, uint32_t n_max, uint32_t rows_max, uint32_t shift, const DedupTab& t, int32_t* status, uint32_t blocks);
// the second of judge's row passes alone, as match and sync launch it over tables of their own: rule 3 over the rows of the numbering
// ufirst (n + 1)
void launch_dedup_rule3(hipStream_t st, const SpliceSrc& src, uint32_t n, uint32_t rows_max, const u64* ufirst, int32_t* status, uint32_t blocks);
// keys: the accepted resources' keys (the same grid over the rows), the keys into the table, the candidates (a thread per resource)
void launch_dedup_keys(hipStream_t st, const SpliceSrc& src, uint32_t n, uint32_t n_max, uint32_t rows_max, bool with_crc, const DedupTab& t, int32_t* status, uint32_t blocks);
// confirm: the byte compare, a fixed grid over (row, 16 KiB piece) items; `blocks` = compact_dev_blocks()
void launch_dedup_confirm(hipStream_t st, const SpliceSrc& src, uint32_t n, uint32_t n_max, uint32_t rows_max, uint32_t shift, bool with_crc, const DedupTab& t, uint32_t blocks);
// settle and emit (one block): rep, new_index (n each), pick (2 n_max, may be null when n is 0), count (4)
void launch_dedup_settle(hipStream_t st, const SpliceSrc& src, uint32_t n, uint32_t n_max, bool with_crc, const DedupTab& t, u64* rep, u64* new_index, u64* pick, u64* count);

// mscomp_amd_deduper_diff, the deduper's second call (diff.hip): which blocks of the new resources differ from the blocks at the same
// index of the base resources, answered as the delta and the patch extent lists. The scratch of a deduper made for it (blockobj.hip
// diff_tab knows the layout); n = n_pair, m = n_blocks_new:
struct DiffTab {
	u64* ufirst;                                       // n + 1: first new row of every pair, in a numbering of the new rows of the pairs that passed rules 1-3
	u64* pfirst;                                       // 3 n: the runs, changed runs and changed blocks in front of the pair's first row
	u64* tsum;                                         // 8 row_tiles(m): six sums and two maxima per tile of rows, then their running values
	uint32_t* verdict;                                 // m: 1 = a changed block, 3 = one the confirm pass found
};
// The call in five stages, seven launches fixed by the creation bounds (two -- seed and counts -- when n_pair or n_blocks_new is 0; the
// caller leaves the others out). seed (one block): rules 1-3, status (n_pair), t.ufirst
void launch_diff_seed(hipStream_t st, const SpliceView& base, const SpliceView& next, uint32_t n_pair, uint32_t nbn, uint32_t shift, const u64* pair, const DiffTab& t, int32_t* status);
// verdicts: the row checks of rule 2 and rule 5 without the bytes, a fixed grid over the new rows; `blocks` = crc_dev_blocks()
void launch_diff_verdicts(hipStream_t st, const SpliceView& base, const SpliceView& next, uint32_t n_pair, uint32_t nbn, uint32_t shift, bool with_crc, const u64* pair,
                          const DiffTab& t, int32_t* status, uint32_t blocks);
// confirm: the byte compare, a fixed grid over (row, 16 KiB piece) items; `blocks` = compact_dev_blocks()
void launch_diff_confirm(hipStream_t st, const SpliceView& base, const SpliceView& next, uint32_t n_pair, uint32_t nbn, uint32_t shift, const u64* pair, const DiffTab& t,
                         const int32_t* status, uint32_t blocks);
// runs (three launches: the tiles' sums, their running values in one block, the rows): delta_ext and patch_ext (4 n_blocks_new each), t.pfirst
void launch_diff_runs(hipStream_t st, const SpliceView& next, uint32_t n_pair, uint32_t nbn, const u64* pair, const DiffTab& t, const int32_t* status, u64* delta_ext, u64* patch_ext);
// the middle launch of the runs alone, rows_tilescan_kernel<6, 2> (rowpass.h), for a call that lays its tiles out as diff does (repair.hip):
// per tile eight words -- six sums, the last row that starts a run + 1, a count diff carries behind it (0: none) -- turned into their
// running values in place (one block)
void launch_diff_tilescan(hipStream_t st, uint32_t tiles, u64* tsum);
// counts: delta_first and patch_first (n_pair + 1, may be null when n_pair is 0), changed (n_pair), count (4)
void launch_diff_counts(hipStream_t st, uint32_t n_pair, uint32_t nbn, const DiffTab& t, u64* delta_first, u64* patch_first, u64* changed, u64* count, uint32_t blocks);

// mscomp_amd_deduper_repair, the deduper's fourth call (repair.hip): from the verdicts of a container and up to three copies
// (mscomp_amd_blocks_salvage), the extent list that takes every bad row from the first copy whose row is good. Its scratch is a DiffTab
// (n = n_res, m = n_blocks_new; verdict holds a row's choice: source | 4 when lost). Four stages, six launches fixed by the creation
// bounds (two -- seed and counts -- when n_res or n_blocks_new is 0; the caller leaves the others out).
// seed (one block): rules 1 and 2, status (n_res), t.ufirst; count[3] cleared
void launch_repair_seed(hipStream_t st, const SpliceView& primary, uint32_t n_res, uint32_t nbn, uint32_t shift, const DiffTab& t, int32_t* status, u64* count);
// choice: rule 3, a fixed grid over the rows; verdict[s] = the salvage verdicts of source s; `blocks` = crc_dev_blocks()
void launch_repair_choice(hipStream_t st, const SpliceSrc& src, const uint32_t* const (&verdict)[4], uint32_t n_src, uint32_t n_res, uint32_t nbn, uint32_t shift, bool with_crc,
                          const DiffTab& t, uint32_t blocks);
// runs (three launches: the tiles' sums, launch_diff_tilescan, the rows): ext (4 n_blocks_new), t.pfirst
void launch_repair_runs(hipStream_t st, const SpliceSrc& src, uint32_t n_res, uint32_t nbn, const DiffTab& t, u64* ext);
// counts: ext_first (n_res + 1, may be null when n_res is 0), fixed and lost (n_res), count (4), and MSCOMP_DATA_ERROR for a resource with a lost row
void launch_repair_counts(hipStream_t st, uint32_t n_res, uint32_t nbn, const DiffTab& t, u64* ext_first, u64* fixed, u64* lost, u64* count, int32_t* status, uint32_t blocks);

// mscomp_amd_deduper_match, the deduper's third call (match.hip): for every block of the resources of `next`, whether an equal block lies in
// one of up to three store containers (found), earlier in next (shared) or nowhere (fresh), answered as the delta and the patch extent
// lists. The views travel as a splicer's, the stores first and next at index n_src. The scratch of a deduper made for it (blockobj.hip
// match_tab knows the layout); n = n_res_total, m = n_blocks_total, mn = n_blocks_new:
struct MatchTab {
	u64* ufirst;                                       // n + 1: first row of every resource, in a numbering of the rows of the resources that passed rules 1, 2 and 4
	u64* pfirst;                                       // 5 n: per resource of next the patch runs, fresh runs, found, shared and fresh blocks in front of its first row
	u64* tsum;                                         // 8 row_tiles(mn): seven sums and one maximum per tile of next's rows, then their running values
	KeyTable kt;                                       // 2 m + 64 slots; its items are rows
	u64* nref;                                         // 1: the refuted rows of the execution
	uint32_t *slot_of, *flag, *rep, *rlist;            // m each: the row's slot (KT_NONE: none); 1 = not equal to its slot's smallest row; rep(u); the refuted rows, ascending
	uint32_t* flocal;                                  // mn: the fresh rows of its tile in front of a row of next
};
// The call in six stages, ten launches fixed by the creation bounds (three when n_blocks_total is 0, seven when n_blocks_new is 0; the
// caller leaves the others out, and launches launch_dedup_clear in front and launch_dedup_rule3 behind the seed).
// seed (one block): rules 1, 2 and 4, status (n), t.ufirst; n_store = the resources of the stores
void launch_match_seed(hipStream_t st, const SpliceSrc& src, uint32_t n, uint32_t n_store, uint32_t nbt, uint32_t nbn, uint32_t shift, const MatchTab& t, int32_t* status);
// keys: per row of an accepted resource its key into the table and itself into its slot's minimum; t.slot_of, t.flag; `blocks` = crc_dev_blocks()
void launch_match_keys(hipStream_t st, const SpliceSrc& src, uint32_t n, uint32_t nbt, uint32_t shift, bool with_crc, const MatchTab& t, const int32_t* status, uint32_t blocks);
// confirm: a row against its slot's smallest row, a fixed grid over (row, 16 KiB piece) items; t.flag, and t.rep as the tables give it; `blocks` = compact_dev_blocks()
void launch_match_confirm(hipStream_t st, const SpliceSrc& src, uint32_t n, uint32_t nbt, uint32_t shift, bool with_crc, const MatchTab& t, uint32_t blocks);
// settle (one block): the flagged rows listed and answered exactly in t.rep, t.nref
void launch_match_settle(hipStream_t st, const SpliceSrc& src, uint32_t n, uint32_t shift, bool with_crc, const MatchTab& t);
// runs (three launches over next's rows: the tiles' sums, their running values in one block, the rows): delta_ext and patch_ext (4 mn each), t.pfirst
void launch_match_runs(hipStream_t st, const SpliceSrc& src, uint32_t n_src, uint32_t n, uint32_t n_store, uint32_t nbn, uint32_t shift, const MatchTab& t, const int32_t* status,
                       u64* delta_ext, u64* patch_ext);
// counts: delta_first and patch_first (next's n_res + 1, may be null when n is 0), cls (3 per resource of next), count (6); `settled`: t.nref was written
void launch_match_counts(hipStream_t st, uint32_t n, uint32_t n_store, uint32_t nbn, bool settled, const MatchTab& t, u64* delta_first, u64* patch_first, u64* cls, u64* count,
                         uint32_t blocks);

// mscomp_amd_deduper_match_digest (match_digest.hip; include/mscomp_amd_match_digest.h): match with equality decided by a row's data length
// and its 16 bytes of a digest column, no stored byte read. The views' columns, 4 nbt words each and 16-byte aligned, travel by value
// beside the SpliceSrc, column s belonging to view s; the scratch is a MatchTab. Keys, confirm and settle are its own -- fixed grids with
// a lane per row, `blocks` = crc_dev_blocks(), and one block --; the other seven launches are match's, in match's order.
struct DigestCols { const uint32_t* c[4]; };
void launch_match_digest_keys(hipStream_t st, const SpliceSrc& src, const DigestCols& cols, uint32_t n, uint32_t nbt, uint32_t shift, const MatchTab& t,
                              const int32_t* status, uint32_t blocks);
void launch_match_digest_confirm(hipStream_t st, const SpliceSrc& src, const DigestCols& cols, uint32_t n, uint32_t nbt, uint32_t shift, const MatchTab& t, uint32_t blocks);
void launch_match_digest_settle(hipStream_t st, const SpliceSrc& src, const DigestCols& cols, uint32_t n, uint32_t shift, const MatchTab& t);

// ---- block transcoders (transcode.hip; mscomp_amd_transcoder_*) ----
// What a transcoder is made for, by value in every kernel's arguments. A group is an aligned span of G = 1 << sg bytes of a resource
// (sg = max(s1, s2)): md = G / B1 source blocks and me = G / B2 new blocks at most. mode: what may be carried.
#define TC_GENERIC 0u                                     // every source block decoded, every new block encoded
#define TC_JOIN    1u                                     // LZNT1 to LZNT1, B2 > B1: a new block whose members all shrank is carried
#define TC_SPLIT   2u                                     // LZNT1 to LZNT1, B2 < B1: a new block whose chunk images shrink it is carried
struct TcDims {
	uint32_t n_res, nbt, nbn, ngmax, gmax;             // resources; entries of the old and of the new block table; the bound of the groups; groups_max
	uint32_t s1, s2, sg, mode;
};
// The transcoder's own tables, in one buffer (blockobj.hip transcode_tab is the only place that knows the layout). Rows of the new table
// are numbered twice: p-rows over the resources that passed rules 1 and 2 (what the class pass fills), final rows over the accepted ones.
struct TranscodeTab {
	u64 *gfirst, *pfirst;                              // n_res + 1 each: first group, first p-row of every resource that passed rules 1 and 2
	int32_t* rstat;                                    // n_res: the resource's status, rule by rule
	uint32_t *gres, *gwork, *gcum;                     // ngmax each: the group's resource; 1 = worked; worked groups up to and including it
	uint32_t* slot_group;                              // gmax: the group in a slot of cache and staging, + 1 (0 = free)
	u64 *plen, *paddr, *pjf, *pdl;                     // nbn each, per p-row: a carried row's stored length and address; first member row of a carried join (~0: none) and its data length
	uint32_t *pkind, *pcrc;                            // nbn each: TC_ROW_*; the folded CRC-32 of a carried join
	u64 *addr, *tsum;                                  // nbn, tiles: per final row where its stored bytes lie (launch_blocks_move); the row tiles' sums
	u64 *d_in_off, *d_in_len, *d_out_off, *d_out_cap, *d_ulen;   // gmax md each: the inner decompress plan's unit tables and lengths
	u64 *d_src, *d_clen, *d_cum, *d_row, *d_raw;       // ... what the CRC kernels read of a decoded member (d_cum: + 1), its row of the old table, a raw member's address
	int32_t* d_ustat; uint32_t *d_act, *d_crc;         // ... the inner plan's status; kind | data length << 2 (copied raw into the cache, or decoded); the CRC-32 read
	u64 *e_in_off, *e_in_len, *e_out_off, *e_out_cap, *e_ulen;   // gmax me each: the inner compress plan's unit tables and lengths
	u64 *e_src, *e_clen, *e_cum;                       // ... the new block's data as an address, the bytes the CRC kernels read of it (e_cum: + 1)
	int32_t* e_ustat; uint32_t* e_crc;
	uint32_t* cnt;                                     // 4: new blocks carried, source blocks decoded, new blocks encoded; 1 = the table as a whole was refused
};
// rules 0-2 (one block): t.rstat, t.gfirst, t.pfirst; t.slot_group and t.cnt cleared
void launch_tc_resources(hipStream_t st, const TcDims& d, const u64* block_first, const u64* res_len, const TranscodeTab& t);
// rule 3, one thread per group: the members' table checks, the class of the group (the chunk header walk on a split) and its p-rows
void launch_tc_classes(hipStream_t st, const TcDims& d, const uint8_t* packed, u64 packed_len, const u64* block_first, const u64* block_off, const u64* res_len,
                       bool with_crc, const TranscodeTab& t);
// rule 4 (one block): the worked groups' slots, then the unit tables of both inner plans and of the CRC kernels (two launches)
void launch_tc_units(hipStream_t st, const TcDims& d, const uint8_t* packed, const uint8_t* cache, const u64* block_first, const u64* block_off, const u64* res_len,
                     bool with_crc, const TranscodeTab& t);
// behind the inner decompress plan: the raw members of the joined groups into the cache (`blocks` = compact_dev_blocks()); behind the CRC
// kernels: a member that did not decode to its length, or not to its checksum, fails its resource (block_crc may be null)
void launch_tc_gather(hipStream_t st, const TcDims& d, uint8_t* cache, const TranscodeTab& t, uint32_t blocks);
void launch_tc_judge(hipStream_t st, const TcDims& d, const uint32_t* block_crc, const TranscodeTab& t);
// rule 5 (one block): new_first (n_res + 1), status (n_res), new_off[0]; then the three row passes tiled over the new table as splice by
// extents tiles them -- tiles, launch_splice_tilescan, rows: new_off (nbn + 1), new_crc (nbn, may be null), t.addr, rule 6
void launch_tc_first(hipStream_t st, const TcDims& d, const u64* res_len, const TranscodeTab& t, u64* new_first, u64* new_off, int32_t* status);
void launch_tc_tiles(hipStream_t st, const TcDims& d, const uint8_t* stage, const u64* res_len, bool with_crc, const TranscodeTab& t, const u64* new_first, u64* new_off,
                     uint32_t* new_crc);
void launch_tc_rows(hipStream_t st, const TcDims& d, u64 cap, const TranscodeTab& t, const u64* new_first, u64* new_off, uint32_t* new_crc, int32_t* status);

// ---- block syncers (sync.hip; mscomp_amd_syncer_*) ----
// A rolling scan of raw units against the block checksums of ONE store. A PIECE is SYNC_RUN bytes of a unit -- what a lane of the scan
// walks --, a TILE SYNC_TILE bytes, 64 pieces -- what a wave walks. A unit of L >= B bytes has L / SYNC_RUN + 1 piece boundaries and
// L / SYNC_TILE + 1 tiles; a shorter one has none. A position of the scan is named by its TILE COORDINATE, tile * SYNC_TILE + offset in
// the tile: it grows with (unit, position).
#define SYNC_TILE      4096u                               // positions a wave of the scan owns (MSCOMP_AMD_SYNC_TILE); no more than the smallest block size
#define SYNC_RUN       64u                                 // ... and a lane of it
#ifndef SYNC_BITS_LOG
#define SYNC_BITS_LOG  18u                                 // the prefilter bitmap: 2^18 bits, 32 KiB of LDS (a build may state another size to measure it)
#endif
#define SYNC_BIT_WORDS (1u << (SYNC_BITS_LOG - 5u))
#define SYNC_CONSTS    (5u * 256u + 4u)                    // per block size: tb[256], mb[4][256], the seed word (and three words of padding)
// The syncer's own tables, in one buffer (blockobj.hip sync_tab is the only place that knows the layout). n = n_res, nu = n_units, nc =
// n_cand_max; tiles_max = in_total_max / SYNC_TILE + nu, pieces_max = in_total_max / SYNC_RUN + nu.
struct SyncTab {
	u64* ufirst;                                       // n + 1: first row of every store resource, in a numbering of the rows of the resources that passed rules 1 and 2
	KeyTable kt;                                       // a power of two of slots, 2^(32 - slot_shift); a key is (CRC word ^ seed) | 1 << 32, its items are the eligible rows
	uint32_t* bits;                                   // SYNC_BIT_WORDS: the bits at the word's low and at its high SYNC_BITS_LOG bits are set for every word in the table
	uint32_t* consts;                                  // SYNC_CONSTS, written once at creation (sync_host_consts)
	u64 *cum, *uoff, *ulen;                            // nu + 1, nu, nu: running sum of the accepted lengths; offset and length of a unit (0, 0 when refused)
	u64 *pfirst, *tfirst;                              // nu + 1 each: first piece boundary, first tile of every unit
	uint32_t* pabs;                                    // pieces_max: raw(unit[: piece boundary])
	uint32_t* traw;                                    // tiles_max: raw(tile), then raw(unit[: tile])
	u64* tword;                                        // 8 tiles_max: what the tile pass leaves per tile and the tile scan adds (sync.hip SW_*)
	u64* cpos; uint32_t *cunit, *crow, *flag;          // nc each: a kept candidate's position, unit and row; 1 = its bytes differ from the decoded row's
	u64 *req, *qlen; int32_t* qstat;                   // 3 nc, nc, nc: the reader core's requests, lengths and statuses
	u64* count;                                        // 8: d_count of the last execution
	uint32_t slot_shift;                               // where a word's walk begins: (word * 0x9E3779B1) >> slot_shift
	uint32_t tiles_max;
};
// the per-block-size constants of the scan, on the host (SYNC_CONSTS words): tb[b] = raw(b) x^(8B) -- the byte that leaves a window --,
// mb[k][b] = (b in byte k of a register) x^(8B), crc_seed(B)
void sync_host_consts(uint32_t shift, uint32_t* out);
// The call in five stages, every grid fixed by the creation bounds. store (three launches and launch_dedup_rule3 between the first two):
// the key table and the bitmap cleared; the seed, one workgroup -- rules 1 and 2, status (n_res), t.ufirst --; the eligible rows' words into table and bitmap
void launch_sync_clear(hipStream_t st, const SyncTab& t, uint32_t blocks);
void launch_sync_seed(hipStream_t st, const SpliceView& v, uint32_t n, uint32_t shift, const SyncTab& t, int32_t* status);
void launch_sync_keys(hipStream_t st, const SpliceView& v, uint32_t n, uint32_t nbt, uint32_t shift, const SyncTab& t, const int32_t* status, uint32_t blocks);
// units (one workgroup): the bounds rule, status (n_units), t.cum .. t.tfirst
void launch_sync_units(hipStream_t st, uint32_t n_units, uint32_t shift, u64 in_total_max, const u64* in_off, const u64* in_len, const SyncTab& t, int32_t* status);
// boundaries (three launches): raw() of every piece and tile; the tiles' running values per unit (one workgroup); t.pabs
void launch_sync_bounds(hipStream_t st, uint32_t n_units, const uint8_t* in, const SyncTab& t, uint32_t blocks);
// scan (three launches): the tile pass, the tile scan (one workgroup: t.count[0 .. 2]), the runs pass, which writes the kept candidates
void launch_sync_scan(hipStream_t st, uint32_t n_units, uint32_t n_cand, uint32_t shift, const uint8_t* in, const SyncTab& t, uint32_t blocks);
// confirm, around the reader core's passes: in front of them the requests (t.req, t.flag cleared); behind them the compare in pieces of 16 KiB
void launch_sync_requests(hipStream_t st, uint32_t n, uint32_t n_cand, uint32_t shift, const SyncTab& t);
void launch_sync_confirm(hipStream_t st, uint32_t n_cand, uint32_t shift, const uint8_t* in, const SyncTab& t, const ReaderTab& r, uint32_t blocks);
// select and emit (one workgroup): the greedy walk per unit, the hits, the literal runs, the counts (distinct: the reader core's count of owners, may be null)
void launch_sync_select(hipStream_t st, uint32_t n_units, uint32_t shift, const SyncTab& t, const int32_t* status, const uint32_t* distinct, u64* hit_first, u64* req, u64* req_off,
                        u64* lit_first, u64* lit, u64* count);

// the digest syncer's pass 5 around the digest kernels (digest.hip): behind launch_sync_requests, the unit table -- off / len (n_cand
// each) = the B-byte window of every kept candidate in the new data, (0, 0) behind the kept ones -- and t.qstat (MSCOMP_OK, or
// MSCOMP_DATA_ERROR for a row outside the numbering); behind the root pass, the window's digest in wdig (4 per candidate) against the
// four words at the candidate's table row in block_digest: a mismatch sets t.flag. No stored byte is read.
void launch_sync_digest_units(hipStream_t st, uint32_t n, uint32_t n_cand, uint32_t shift, const SyncTab& t, u64* off, u64* len);
void launch_sync_digest_compare(hipStream_t st, const SpliceView& v, uint32_t n, uint32_t n_cand, const uint32_t* block_digest, const SyncTab& t, const uint32_t* wdig);

// ---- BLAKE2s block digests (digest.hip; mscomp_amd_digester_*, mscomp_amd_syncer_sync_digest) ----
// digest(D) of a unit of 1 <= e <= B bytes: BLAKE2s in tree mode, leaves of DG_LEAF bytes, two levels, unlimited fan-out, 16 bytes inner
// and final, no key. The passes work on a device unit table: unit u = len[u] bytes at base + off[u] for u < min(*count, n_max), and its
// leaf k has the slot (u << (shift - 10)) + k of `leaf`, whatever the other units' lengths: no numbering pass, and 16 B / 1024 bytes of
// scratch per possible unit.
#define DG_LEAF       1024u
#define DG_LEAF_SHIFT 10u
struct DigestTab {
	const u64* off; const u64* len;                    // n_max each
	const u64* count;                                  // 1: the units of this execution
	uint32_t* leaf;                                    // 4 (n_max << (shift - 10)): the leaves' inner digests
	uint32_t* out;                                     // 4 n_max: a scratch column for the units' digests (check, sync); blocks writes the caller's
	uint32_t n_max, shift;
};
// the leaf pass: a fixed grid dealt over the leaf slots, a lane per leaf of up to 16 compressions; `blocks` = crc_dev_blocks()
void launch_digest_leaves(hipStream_t st, const uint8_t* base, const DigestTab& d, uint32_t blocks);
// the root pass, a lane per unit over its 16 n bytes of leaf digests: out[4 u ..] (n_max entries; four zero words at and behind *count
// and for an empty unit). rstat (n_res, may be null): copied to d_status by the same launch
void launch_digest_roots(hipStream_t st, const DigestTab& d, uint32_t* out, uint32_t n_res, const int32_t* rstat, int32_t* d_status);
// (check, behind the root pass: launch_blocks_kfold over d.out and the caller's block_digest, four words per entry)

// ---- Reed-Solomon parity rows (parity.hip, gfmath.h; mscomp_amd_parity_*) ----
// m parity rows per group of k table rows, over the STORED bytes: P_p = XOR_i alpha^(p i) D_i in GF(2^8). Row j of the nb rows the
// container has is member j / G of group j % G, G = ceil(nb / k): nb is a device value, so every pass works G out for itself and is
// gridded by gmax = ceil(nbt / k). Parity row q = g m + p. The scratch of a parity object (blockobj.hip parity_tab knows the layout),
// Q = m gmax:
struct ParityTab {
	u64 *plen, *clen, *cum;                            // Q, Q, Q + 1: a parity row's length by the row lengths; the bytes the CRC kernels read of it; their running sum
	u64* fixlen;                                       // nbt: rebuild, the stored length of a row it rebuilds, else 0
	u64* count;                                        // 8: rebuild, d_count[0..5], then the listed groups
	uint32_t* pcrc;                                    // Q: the CRC-32 read of every parity row
	uint32_t* rflag;                                   // nbt: rebuild, 1 = the row is rebuilt
	uint32_t* grec;                                    // 6 gmax: rebuild, a record per listed (damaged, recoverable) group: e | parities, members, three rows of the inverse, g
	uint32_t nbt, gmax, k, m, shift;
};
#define PA_TILE_SHIFT 12u                              // a workgroup item of the parity and solve passes: 4096 bytes of a group's column
// build (nine launches with the three of the CRC pass between units and head; the caller runs that one). rows: rule 1, row_len (nbt);
// groups: t.plen; scan: the running sum of t.plen is par_off (one workgroup; out: n + 1 entries); units: t.clen by rule 4; parity: the bytes, a fixed grid
// dealt over (group, column tile); head: par_crc from t.pcrc, par_head and the status. `mis`: the view's table is not of nbt rows (rule 0)
void launch_parity_rows(hipStream_t st, const SpliceView& v, const ParityTab& t, bool mis, uint32_t* row_len, uint32_t blocks);
void launch_parity_groups(hipStream_t st, const SpliceView& v, const ParityTab& t, bool mis, const uint32_t* row_len, const u64* head, uint32_t blocks);
void launch_parity_scan(hipStream_t st, u64 n, const u64* len, u64* out);
void launch_parity_units(hipStream_t st, const ParityTab& t, const u64* par_off, u64 par_cap, uint32_t blocks);
void launch_parity_build(hipStream_t st, const SpliceView& v, const ParityTab& t, bool mis, const uint32_t* row_len, uint8_t* par, u64 par_cap, const u64* par_off, uint32_t blocks);
void launch_parity_head(hipStream_t st, const SpliceView& v, const ParityTab& t, bool mis, const u64* par_off, u64 par_cap, uint32_t* par_crc, u64* par_head, int32_t* status,
                        uint32_t blocks);
// rebuild: launch_parity_groups with the caller's header (rule 0), then -- check: t.clen by rule 2's table half, t.fixlen, t.rflag and
// t.count cleared; the CRC pass into t.pcrc; damage: a lane per group, rules 1-3, the records and counts; launch_parity_scan over t.fixlen
// gives fix_off; solve: a fixed grid dealt over (listed group, column tile); tail: the verdicts, the counts and the status
void launch_parity_check(hipStream_t st, const ParityTab& t, const u64* par_off, u64 par_len, uint32_t blocks);
void launch_parity_damage(hipStream_t st, const SpliceView& v, const ParityTab& t, bool mis, const uint32_t* verdict, const u64* par_off, u64 par_len, const uint32_t* par_crc,
                          const uint32_t* row_len, const u64* head, uint32_t blocks);
void launch_parity_solve(hipStream_t st, const SpliceView& v, const ParityTab& t, bool mis, const uint8_t* par, const u64* par_off, const uint32_t* row_len, const u64* head,
                         uint8_t* fix, u64 fix_cap, const u64* fix_off, uint32_t blocks);
void launch_parity_tail(hipStream_t st, const SpliceView& v, const ParityTab& t, bool mis, const u64* head, u64 fix_cap, const u64* fix_off, uint32_t* fix_verdict, u64* count,
                        int32_t* status, uint32_t blocks);

// ---- CRC-32 of units in HBM (crc32.hip; mscomp_amd_plan_*_crc_dev, mscomp_amd_blocks_crc / _check) ----
// the table pass, one block: cum[0..n] = running sum of the accepted in_len (a unit whose running total exceeds in_total_max: length 0, status
// MSCOMP_ARG_ERROR), off[i] = its offset. in_off / off and status may be null.
void launch_crc_tables(hipStream_t st, uint32_t n, u64 in_total_max, const u64* in_off, const u64* in_len, u64* off, u64* cum, int32_t* status);
// behind it, one thread per unit: crc[i] = the terms of the CRC of cum[i + 1] - cum[i] bytes that do not depend on the data; fac[i] =
// x^(8 after[i]). Either pair may be null.
void launch_crc_seeds(hipStream_t st, uint32_t n, const u64* cum, uint32_t* crc, const u64* after, uint32_t* fac);
// the bytes: crc[u] ^= the data terms of the cum[u + 1] - cum[u] bytes at base + off[u]; with gcrc, also gcrc[grp[u]] ^= the same terms times
// fac[u]. `blocks` = the fixed grid, crc_dev_blocks() of the device
uint32_t crc_dev_blocks();
void launch_crc_units(hipStream_t st, uint32_t n, const uint8_t* base, const u64* off, const u64* cum, uint32_t* crc,
                      const uint32_t* grp, const uint32_t* fac, uint32_t* gcrc, uint32_t blocks);

// mscomp_amd_res_crc_dev: res_crc[r] = the CRC-32 of resource r from its blocks' CRC-32s alone. A seed kernel (one thread per resource:
// status, res_crc = 0), then a fixed grid over the table's blocks: each finds its resource and folds block_crc[j] x^(8 bytes of the
// resource behind block j) into the resource's word with an atomic XOR. `blocks` = crc_dev_blocks()
void launch_res_crc(hipStream_t st, uint32_t n_res, uint32_t nbt, uint32_t shift, const u64* block_first, const u64* res_len, const uint32_t* block_crc,
                    uint32_t* res_crc, int32_t* status, uint32_t blocks);

// The same fold along runs of any table (a transcoder's carried joins): out[i] = the CRC-32 of the len[i] bytes whose pieces of
// 1 << shift bytes (the last one shorter) have the CRC-32s crc_in[first[i] ..], for the rows i < min(n, *n_live) with first[i] != ~0; the
// other rows are left alone. One thread per row, no data read.
void launch_crc_fold_runs(hipStream_t st, uint32_t n, const u64* n_live, uint32_t shift, const u64* first, const u64* len, const uint32_t* crc_in, uint32_t* out);

// ---- utilities (util.hip) ----
// prefix[0..n] = exclusive scan of sizes[0..n) as u64 (prefix[n] = total). block_sums: scratch of ceil(n/1024)+1 u64.
void launch_scan_sizes(hipStream_t st, const uint32_t* sizes, u64* prefix, uint32_t n, u64* block_sums);
// Concatenate the chunk images of every unit into the caller's output (skips units that do not fit): a fixed grid over tiles of 64 chunks,
// place_blocks() of the device and instance, capped by the tiles of the batch and by the test hook (host.h Switches: place_cap, 0 = no cap)
void launch_concat_slots(hipStream_t st, const uint8_t* slots, uint32_t slot_stride, const uint32_t* slot_size,
                         const u64* prefix, const BatchTables& bt, uint8_t* d_out, bool dev = false);
uint32_t place_blocks(bool dev);
// Per unit: out_len, status (OK / BUF_ERROR); LZNT1 also appends the uncounted 00 00 End_of_buffer when room.
// outputs of a batch packed back to back: packed_off[0..n] (device), bytes of unit u at d_packed + packed_off[u]
void launch_compact(hipStream_t st, const uint8_t* d_out, const u64* d_out_off, const uint32_t* d_tile_prefix, uint32_t n_units, uint32_t n_tiles,
                    const u64* d_out_len, u64* d_packed_off, uint8_t* d_packed);
uint32_t run_lds_lane_order_check(hipStream_t st, uint32_t seed, uint32_t blocks, uint32_t rounds, uint32_t nkeys, uint32_t* d_bad);
// v_alignbyte_b32 with operands that have bits above [1:0] set (util.hip): the number of results, of ALIGNBYTE_CHECK_WORDS written to d_out,
// that differ from {hi, lo} >> 8 (operand & 3); 0xFFFFFFFF = the check could not run
#define ALIGNBYTE_CHECK_WORDS (256u * 128u)
uint32_t run_alignbyte_check(hipStream_t st, uint32_t seed, uint32_t* d_out);
void launch_finalize_units(hipStream_t st, const u64* prefix, const BatchTables& bt, uint8_t* d_out,
                           u64* d_out_len, int32_t* d_status, int lznt1_eob);

} // namespace msc
