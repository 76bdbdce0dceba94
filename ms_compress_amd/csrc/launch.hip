// launch.hip -- the launch sequences of a plan, one per direction and one for the size query, for host-table and device-table plans alike
// (plan.hip and plan_dev.hip run them through plan_run), and the views of the context scratch they launch over. Host code only.
#include "host.h"

using namespace msc;

static const uint32_t XH_FB_BLOCKS = 256;              // persistent blocks of the fallback kernel (one per CU: its package pool fills the LDS)

static LzgTables lzg_tables(const mscomp_amd_plan* p, mscomp_amd_ctx* c)
{
	LzgTables g = {};
	const DevPaths& d = p->paths;
	g.n_big = p->lzg_big; g.n_tb = p->lzg_tb; g.n_tiles = p->lzg_tiles; g.cnt = d.lzg_cnt;
	if (!g.n_big) { return g; }
	g.unit = d.lzg_unit; g.tb_prefix = d.lzg_tb_prefix; g.tile_prefix = d.lzg_tile_prefix; g.word_prefix = d.lzg_word_prefix;
	g.bsum = static_cast<u64*>(c->lzg_bsum.p);
	lzg_dir_layout(g, c->lzg_dir.p, p->lzg_tiles); lzg_words_layout(g, c->lzg_words.p, p->lzg_words, p->lzg_tiles);
	return g;
}
// the last stage of Xpress / Xpress+Huffman decompression: tokens -> bytes (a wave per small unit, a block per middle one, all CUs for the large ones)
static void run_lz_copy_global(mscomp_amd_ctx* c, const mscomp_amd_plan* p, hipStream_t st, const u64* tp, const uint32_t* tok, const u64* ntok,
                               const u64* d_out_len, const int32_t* d_status, uint8_t* d_out)
{
	if (!p->lzg_big) { return; }
	const LzgTables g = lzg_tables(p, c);
	{ KernelTimer t(c, "lzg_dir_kernels"); launch_lzg_directory(st, g, tp, tok, ntok, d_out_len, d_status); }
	{ KernelTimer t(c, "lzg_expand_kernel"); launch_lzg_expand(st, g, p->bt, tp, tok, ntok, d_out_len, d_status, d_out); }
	{ KernelTimer t(c, "lzg_jump_kernel"); launch_lzg_jump(st, g, p->bt, d_out_len, d_status, d_out); }
}

static XpressWinBufs xpress_win_bufs(mscomp_amd_ctx* c, uint32_t n_chunks)
{
	XpressWinBufs b = {};
	b.wtok = static_cast<u64*>(c->wtok.p); b.wmat = static_cast<u64*>(c->wmat.p); b.wfar = static_cast<uint32_t*>(c->wfar.p);
	if (c->wrec.p && c->sbrec.p) { wrec_layout(b, c->wrec.p, (size_t)n_chunks * 1024u + 64); sbrec_layout(b, c->sbrec.p, (size_t)n_chunks + 1); }
	return b;
}

// the scratch of the LZNT1 header chain, laid out for the plan's chunk (segment) count
static LzdBufs lzd_bufs(mscomp_amd_ctx* c, const mscomp_amd_plan* p)
{
	LzdBufs b;
	b.cin = static_cast<uint32_t*>(c->dz_cin.p); b.csize = static_cast<uint16_t*>(c->dz_csize.p); b.flat = static_cast<u64*>(c->prefix.p);
	dz_unit_layout(b, c->dz_unit.p, p->n_units, p->n_chunks);
	return b;
}
// the candidate records of Xpress+Huffman decompression, laid out for the plan's candidate slots (the token scratch, if any, is set by the caller)
static XhcBufs xhc_bufs(mscomp_amd_ctx* c, const mscomp_amd_plan* p) { XhcBufs xb = {}; dz_xhc_layout(xb, c->dz_xhc.p, p->n_units, p->xhc_slots); return xb; }

// the segment tables and scratch of the large Xpress streams of p (xps_*): none when the plan does not take that path
static XpsTables xps_tables(const mscomp_amd_plan* p, mscomp_amd_ctx* c)
{
	XpsTables x = {};
	if (!p->xps_big) { return x; }
	const DevPaths& d = p->paths;
	x.unit = d.xps_unit; x.seg_prefix = d.xps_seg_prefix; x.n_big = p->xps_big; x.n_seg = p->xps_seg; x.seg_bytes = p->xps_seg_bytes; x.warm_bytes = p->xps_warm_bytes; x.cnt = d.xps_cnt;
	xps_buf_layout(x, c->xps_buf.p, p->xps_seg, p->xps_big, p->n_units);
	return x;
}

// the per-unit path verdicts an execution of p leaves in the ctx scratch: Xpress+Huffman, XHC_SPEC / XHC_SERIAL for every unit (xhc_chain_kernel);
// Xpress, the segment walk's mode for every unit with XPS_MIN_IN input bytes or more (2 = done by segments, 0 = the one-wave walk), none when
// the plan does not take that path
void msc::note_modes(mscomp_amd_plan* p)
{
	mscomp_amd_ctx* c = p->ctx;
	c->dbg_mode = nullptr; c->dbg_mode_n = 0; c->dbg_mode_cnt = nullptr;
	c->dbg_lzg_open = p->large && p->lzg_big ? lzg_tables(p, c).open : nullptr;
	if (p->format == MSCOMP_XPRESS_HUFF && p->n_units) { c->dbg_mode = xhc_bufs(c, p).mode; c->dbg_mode_n = p->n_units; }
	if (p->format == MSCOMP_XPRESS && p->xps_big && (p->sizing || p->large || g_sw.xpd.load(std::memory_order_relaxed) == 0)) { c->dbg_mode = xps_tables(p, c).mode; c->dbg_mode_n = p->xps_big; c->dbg_mode_cnt = p->paths.xps_cnt; }
}

// ---- the launch sequences: one per direction, for host-table and device-table plans alike ----
// A dev plan runs the DEV instances of the chunk-gridded kernels (p->dev: bt.n_chunks is its bound, the blocks past chunk_prefix[n_units] return at
// once); its table pass goes in front of these launches and its reject pass behind them, at the call site (mscomp_amd_plan_execute_dev /
// _execute_size_dev). The optional paths -- xps_* segments, the lzglobal.hip stage, Xpress+Huffman token scratch -- are off for a plain dev plan
// by their zero counts; a dev plan with large units (p->large) has their bounds in the same fields, a path pass behind its table pass that
// builds their tables, and runs the DEV instances of their kernels, which read the counts of the execution from device memory.

// The first stages that decode_launch and size_launch share. LZNT1, the header chain: which chunk headers hold, and where each chunk's
// bytes go (a dev plan: segments past the real count add nothing to the scan -- zeroed by a kernel, no memset: the launches may go into a
// caller's graph)
static void lzd_headers(mscomp_amd_plan* p, const uint8_t* d_in, const LzdBufs& b)
{
	mscomp_amd_ctx* c = p->ctx;
	hipStream_t st = c->stream;
	if (p->dev) { launch_dev_zero(st, b.selcnt, p->n_chunks); }
	{ KernelTimer t(c, "lzd_seg_kernel"); launch_lzd_segments(st, d_in, p->bt, b, p->dev); }
	{ KernelTimer t(c, "lzd_verify_kernel"); launch_lzd_verify(st, d_in, p->bt, b); }
	{ KernelTimer t(c, "scan_sizes"); launch_scan_sizes(st, b.selcnt, b.flat, p->n_chunks, static_cast<u64*>(c->tile_sums.p)); }
}
// Xpress, the segment walk of the large streams: every segment walked speculatively, then `rounds` of "walk the segments again that do not hold"
static void xps_walk(mscomp_amd_plan* p, const uint8_t* d_in, const XpsTables& x, uint32_t rounds, u64* ntok, uint64_t* d_out_len, int32_t* d_status)
{
	mscomp_amd_ctx* c = p->ctx;
	{ KernelTimer t2(c, "xps_walk_kernel"); launch_xps_walk(c->stream, d_in, p->bt, x); }
	for (uint32_t r = 0; r < rounds; ++r) { KernelTimer t2(c, "xps_redo_kernels"); launch_xps_redo(c->stream, d_in, p->bt, x, ntok, d_out_len, d_status); }
}
// Xpress+Huffman, the mark stage: the candidate chunk starts of every unit
static void xhc_mark(mscomp_amd_plan* p, const uint8_t* d_in, const XhcBufs& xb)
{
	KernelTimer t(p->ctx, "xhc_mark_kernel"); launch_xhc_mark(p->ctx->stream, d_in, p->bt, p->cand_prefix, xb, p->dev);
}

void msc::decode_launch(mscomp_amd_plan* p, const uint8_t* d_in, uint8_t* d_out, uint64_t* d_out_len, int32_t* d_status)
{
	mscomp_amd_ctx* c = p->ctx;
	hipStream_t st = c->stream;
	const u64* tp = p->tok_prefix; uint32_t* tok = static_cast<uint32_t*>(c->dz_tok.p); u64* ntok = static_cast<u64*>(c->dz_ntok.p);
	const u64 gmin = p->lzg_big ? (u64)LZG_MIN_CAP : ~(u64)0;           // (host plans; p->large: the byte kernels read lzg_cnt instead)
	const uint32_t* gcnt = p->large && p->lzg_big ? p->paths.lzg_cnt : nullptr;
	switch (p->format) {
	case MSCOMP_LZNT1: {
		const LzdBufs b = lzd_bufs(c, p);
		lzd_headers(p, d_in, b);
		{ KernelTimer t(c, "lzd_chunk_kernel"); launch_lzd_chunks(st, d_in, p->bt, b, d_out); }
		{ KernelTimer t(c, "lzd_finalize_kernel"); launch_lzd_finalize(st, p->bt, b, d_out_len, d_status); }
		{ KernelTimer t(c, "lzd_replace_kernel"); launch_lzd_replace(st, d_in, p->bt, b, d_out); }
		return;
	}
	case MSCOMP_XPRESS: {                                          // tokens a flag word at a time, then the copy kernels; large streams of host plans by segments first
		const int mode = p->dev ? (p->large ? 0 : 2) : g_sw.xpd.load(std::memory_order_relaxed);   // (the test hook switches host plans only; a dev plan walks by segments when it was created for large units)
		if (mode == 1) { KernelTimer t(c, "xpd_kernel"); launch_xpress_decompress(st, d_in, p->bt, d_out, d_out_len, d_status); return; }
		const XpsTables x = mode != 2 ? xps_tables(p, c) : XpsTables{};
		if (x.n_big) {
			xps_walk(p, d_in, x, env_xps_rounds(), ntok, d_out_len, d_status);
			{ KernelTimer t2(c, "xps_emit_kernel"); launch_xps_emit(st, d_in, p->bt, x, tp, tok, ntok, d_out_len, d_status); }
		}
		{ KernelTimer t(c, "xpt_parse_kernel"); launch_xpt_parse(st, d_in, p->bt, tp, tok, ntok, d_out_len, d_status, x); }
		{ KernelTimer t(c, "lz_copy_kernel"); launch_lz_copy(st, p->bt, tp, tok, ntok, d_out_len, d_status, d_out, gmin, gcnt); }
		{ KernelTimer t(c, "lz_copy_block_kernel"); launch_lz_copy_block(st, p->bt, tp, tok, ntok, d_out_len, d_status, d_out, gmin, gcnt); }
		break;
	}
	default: {                                                     // MSCOMP_XPRESS_HUFF (without token scratch the accepted chunks are walked twice)
		XhcBufs xb = xhc_bufs(c, p);
		if (p->xhc_scr) { xb.scr_prefix = p->scr_prefix; xb.scr_tok = static_cast<uint32_t*>(c->dz_scr.p); }
		xhc_mark(p, d_in, xb);
		{ KernelTimer t(c, "xhc_parse_kernel"); launch_xhc_candidates(st, d_in, p->bt, tp, p->cand_prefix, p->xhc_slots, xb, tok); }
		{ KernelTimer t(c, "xhc_chain_kernel"); launch_xhc_chain(st, p->bt, p->cand_prefix, xb, ntok, d_out_len, d_status); }
		{ KernelTimer t(c, "xhc_parse2_kernel"); launch_xhc_tokens(st, d_in, p->bt, tp, p->cand_prefix, p->xhc_slots, xb, tok); }
		{ KernelTimer t(c, "xhd_parse_kernel"); launch_xhd_parse(st, d_in, p->bt, tp, tok, ntok, d_out_len, d_status, xb.mode); }
		{ KernelTimer t(c, "lz_copy_kernel"); launch_lz_copy(st, p->bt, tp, tok, ntok, d_out_len, d_status, d_out, gmin, gcnt); launch_lz_copy_block(st, p->bt, tp, tok, ntok, d_out_len, d_status, d_out, gmin, gcnt); }   // (both under one name)
		break;
	}
	}
	run_lz_copy_global(c, p, st, tp, tok, ntok, d_out_len, d_status, d_out);
}

void msc::compress_launch(mscomp_amd_plan* p, const uint8_t* d_in, uint8_t* d_out, uint64_t* d_out_len, int32_t* d_status)
{
	mscomp_amd_ctx* c = p->ctx;
	hipStream_t st = c->stream;
	const bool dev = p->dev;
	uint32_t* slot_size = static_cast<uint32_t*>(c->slot_size.p);
	u64* prefix = static_cast<u64*>(c->prefix.p);
	u64* tile_sums = static_cast<u64*>(c->tile_sums.p);
	uint16_t* links = static_cast<uint16_t*>(c->links.p); uint16_t* lasthead = static_cast<uint16_t*>(c->lasthead.p);
	uint16_t* mlen3 = static_cast<uint16_t*>(c->mlen3.p); uint16_t* moff = mlen3 + 1;   /* one word per position: length - 3 | offset << 16 (common.h S16) */
	const bool find = !p->matches_ready;                           // (Xpress formats: the pipelined one-shot call has run links + find itself, for this execution only)
	p->matches_ready = false;
	switch (p->format) {
	case MSCOMP_LZNT1: {                                           // (dev: the chunk kernels write a size of 0 for the chunks past the real count)
		uint8_t* slots = static_cast<uint8_t*>(c->slots.p);
		if (p->lznt1_sa) { KernelTimer t(c, "lznt1_sa_chunk_kernel"); launch_lznt1_sa_chunks(st, d_in, p->bt, slots, slot_size, dev); }
		else { KernelTimer t(c, "lznt1_chunk_kernel"); launch_lznt1_chunks(st, d_in, p->bt, slots, slot_size, static_cast<uint16_t*>(c->lzrec.p), dev); }
		{ KernelTimer t(c, "scan_sizes"); launch_scan_sizes(st, slot_size, prefix, p->n_chunks, tile_sums); }
		{ KernelTimer t(c, "concat_slots_kernel"); launch_concat_slots(st, slots, LZNT1_SLOT, slot_size, prefix, p->bt, d_out, dev); }
		{ KernelTimer t(c, "finalize_units_kernel"); launch_finalize_units(st, prefix, p->bt, d_out, d_out_len, d_status, 1); }
		break;
	}
	case MSCOMP_XPRESS: {
		if (find) {
			{ KernelTimer t(c, "xp_links_kernel"); launch_xp_links(st, d_in, p->bt, links, lasthead, dev); }
			// units of one link chunk: Find only where a greedy parse can start a token, window and links in LDS; longer streams: every position
			if (g_sw.finder.load(std::memory_order_relaxed) != 2 && p->max_unit <= 65536u) { KernelTimer t(c, "xp_lazy2_kernel"); launch_xp_lazy2(st, d_in, p->bt, links, mlen3, moff, dev); }
			else { KernelTimer t(c, "xp_find_kernel"); launch_xp_find(st, d_in, p->bt, links, lasthead, mlen3, moff, 0x2000u, 0, dev); }
		}
		{ KernelTimer t(c, "xpress_emit_kernel"); launch_xpress_emit(st, d_in, p->bt, mlen3, moff, xpress_win_bufs(c, p->n_chunks), d_out, d_out_len, d_status, dev); }
		break;
	}
	default: {                                                     // MSCOMP_XPRESS_HUFF (dev: xh_huff_kernel<true> writes a size of 0 for the chunks past the real count)
		u64* tokbits = static_cast<u64*>(c->tokbits.p); uint32_t* counts = static_cast<uint32_t*>(c->counts.p);
		uint32_t* extra = static_cast<uint32_t*>(c->extra.p); uint8_t* lens = static_cast<uint8_t*>(c->lens.p);
		uint16_t* codes = static_cast<uint16_t*>(c->codes.p); uint32_t* fbflag = static_cast<uint32_t*>(c->fbflag.p);
		uint32_t* fb_count; uint32_t* fb_list;
		fb_list_layout(fb_count, fb_list, c->fb_list.p, p->n_chunks);
		if (find) {
			{ KernelTimer t(c, "xp_links_kernel"); launch_xp_links(st, d_in, p->bt, links, lasthead, dev); }
			{ KernelTimer t(c, "xp_find_kernel"); launch_xp_find(st, d_in, p->bt, links, lasthead, mlen3, moff, 0xFFFFu, 1, dev); }
		}
		{ KernelTimer t(c, "xh_parse_kernel"); launch_xh_parse(st, d_in, p->bt, mlen3, moff, tokbits, counts, extra, dev); }
		{ KernelTimer t(c, "xh_huff_kernel"); launch_xh_huff(st, p->bt, counts, extra, lens, codes, slot_size, fb_list, fb_count, fbflag, dev); }
		{ KernelTimer t(c, "xh_fallback_kernel"); launch_xh_fallback(st, d_in, p->bt, fb_list, fb_count, XH_FB_BLOCKS, tokbits, lens, codes, slot_size); }
		{ KernelTimer t(c, "scan_sizes"); launch_scan_sizes(st, slot_size, prefix, p->n_chunks, tile_sums); }
		{ KernelTimer t(c, "xh_encode_kernel"); launch_xh_encode(st, d_in, p->bt, mlen3, moff, tokbits, lens, codes, fbflag, prefix, d_out, dev); }
		{ KernelTimer t(c, "finalize_units_kernel"); launch_finalize_units(st, prefix, p->bt, d_out, d_out_len, d_status, 0); }
		break;
	}
	}
}

// ---- decompressed-size query: the decoders' walks without the byte stage and without token stores ----
void msc::size_launch(mscomp_amd_plan* p, const uint8_t* d_in, uint64_t* d_out_len, uint64_t* d_need, int32_t* d_status)
{
	mscomp_amd_ctx* c = p->ctx;
	hipStream_t st = c->stream;
	u64* ntok = static_cast<u64*>(c->dz_ntok.p);
	switch (p->format) {
	case MSCOMP_LZNT1: {                                   // the header chain as in decode_launch, then every chunk sized, then the verdict at the limit (which writes need)
		const LzdBufs b = lzd_bufs(c, p);
		lzd_headers(p, d_in, b);
		{ KernelTimer t(c, "lzd_size_kernel"); launch_lzd_sizes(st, d_in, p->bt, b); }
		{ KernelTimer t(c, "lzd_finalize_kernel"); launch_lzd_finalize(st, p->bt, b, d_out_len, d_status, d_need); }
		break;
	}
	case MSCOMP_XPRESS: {                                  // large streams of host plans by segments, the others (a dev plan: every stream) by the one-wave walk
		const XpsTables x = xps_tables(p, c);
		if (x.n_big) {
			xps_walk(p, d_in, x, XPS_ROUNDS, ntok, d_out_len, d_status);   // (the constant: MSCOMP_AMD_XPS_ROUNDS applies to decompress plans only)
			{ KernelTimer t2(c, "xps_size_kernel"); launch_xps_size(st, d_in, p->bt, x, ntok, d_out_len, d_status); }
		}
		{ KernelTimer t(c, "xpt_size_kernel"); launch_xpt_size(st, d_in, p->bt, ntok, d_out_len, d_status, x); }
		break;
	}
	default: {                                             // MSCOMP_XPRESS_HUFF
		const XhcBufs xb = xhc_bufs(c, p);
		xhc_mark(p, d_in, xb);
		{ KernelTimer t(c, "xhc_size_kernel"); launch_xhc_candidates_size(st, d_in, p->bt, p->cand_prefix, p->xhc_slots, xb); }
		{ KernelTimer t(c, "xhc_chain_kernel"); launch_xhc_chain(st, p->bt, p->cand_prefix, xb, ntok, d_out_len, d_status); }
		{ KernelTimer t(c, "xhd_size_kernel"); launch_xhd_size(st, d_in, p->bt, ntok, d_out_len, d_status, xb.mode); }
		break;
	}
	}
}
