// plan.hip -- plans with host tables (include/mscomp_amd.h): what a plan reserves, its creation and destruction, execute / execute_size, the
// one-call batch entries, capacity layout and compaction. Host code only: the launches are launch.hip's.
#include "host.h"

using namespace msc;

// `tables` of the plan, reserved for its kind and counts (tables_layout), and what the launch code reads of it: bt, the prefixes and reject
// of a dev plan (the launch functions do not know where a creator put them)
bool msc::reserve_tables(mscomp_amd_plan* p)
{
	PlanCols t;
	const bool scr = p->large && p->format == MSCOMP_XPRESS_HUFF && !p->sizing;
	if (!p->tables.reserve(tables_layout(t, nullptr, p->n_units, p->dev, p->decompress, scr) + 8)) { return false; }
	tables_layout(t, p->tables.p, p->n_units, p->dev, p->decompress, scr);
	p->bt = { t.in_off, t.in_len, t.out_off, t.out_cap, t.chunk_prefix, p->n_units, p->n_chunks };
	p->tok_prefix = t.tok_prefix; p->cand_prefix = t.cand_prefix; p->scr_prefix = t.scr_prefix; p->reject = t.reject;
	return true;
}
// a table to a plan-owned buffer, waited for (the table is the caller's local)
static bool upload(mscomp_amd_ctx* c, const DevBuf& b, const std::vector<uint64_t>& tab)
{
	return hipMemcpyAsync(b.p, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, c->stream) == hipSuccess && hipStreamSynchronize(c->stream) == hipSuccess;
}

// ---- the ctx scratch of a plan, reserved when the plan is created so that execute() never allocates ----
// Host plans call these with their exact counts, dev plans with their bounds.
static bool reserve_scan(mscomp_amd_ctx* c, size_t n_chunks)   // launch_scan_sizes over the chunks
{
	return c->prefix.reserve((n_chunks + 2) * sizeof(uint64_t)) && c->tile_sums.reserve((n_chunks / 1024 + 4) * sizeof(uint64_t));
}
bool msc::reserve_compress_scratch(mscomp_amd_ctx* c, MSCompFormat format, size_t n_units, size_t n_chunks, bool lznt1_sa)
{
	bool ok = c->slot_size.reserve((n_chunks + 1) * sizeof(uint32_t)) && reserve_scan(c, n_chunks);
	if (ok && format == MSCOMP_LZNT1) { ok = c->slots.reserve(n_chunks * LZNT1_SLOT + 64) && (lznt1_sa || c->lzrec.reserve(n_chunks * LZNT1_REC + 64)); }
	if (ok && format != MSCOMP_LZNT1) {
		const size_t per = n_chunks * 65536u * sizeof(uint16_t) + 64;
		// (mlen3: 4 bytes per position, both halves of the match word)
		ok = c->links.reserve(per) && c->mlen3.reserve(2 * per) && c->lasthead.reserve(per / 2 + 64);
	}
	if (ok && format == MSCOMP_XPRESS) {
		const size_t nw = n_chunks * 1024u + 64, ns = n_chunks + 1;
		ok = c->wtok.reserve(nw * 8) && c->wmat.reserve(nw * 8) && c->wfar.reserve(nw * 4);
		if (ok && xpress_emit_mode_for((uint32_t)n_units, (uint32_t)n_chunks) == 4) {    // the block-per-super-block kernels (launch_xpress_emit chooses from the same two numbers)
			XpressWinBufs wb;
			ok = c->wrec.reserve(wrec_layout(wb, nullptr, nw)) && c->sbrec.reserve(sbrec_layout(wb, nullptr, ns));
		}
	}
	if (ok && format == MSCOMP_XPRESS_HUFF) {
		const size_t nc = n_chunks + 1;
		uint32_t* fb_count; uint32_t* fb_list;
		ok = c->tokbits.reserve(nc * 1024 * 8) && c->counts.reserve(nc * 512 * 4) && c->extra.reserve(nc * 4) &&
		     c->lens.reserve(nc * 512) && c->codes.reserve(nc * 1024) && c->fb_list.reserve(fb_list_layout(fb_count, fb_list, nullptr, n_chunks)) && c->fbflag.reserve(nc * 4);
	}
	return ok;
}
// decompress and size plans. LZNT1: the header chain (lzd_bufs) and its scan; Xpress formats: token counts, `slots` 32-bit tokens unless a size
// plan asks (store), and for Xpress+Huffman the records of `cands` candidates (xhc_bufs)
bool msc::reserve_decode_scratch(mscomp_amd_ctx* c, MSCompFormat format, size_t n_units, size_t n_chunks, uint64_t slots, uint64_t cands, bool store)
{
	LzdBufs b; XhcBufs xb;
	if (format == MSCOMP_LZNT1) {
		return reserve_scan(c, n_chunks) && c->dz_cin.reserve(n_chunks * LZD_SLOTS * 4 + 64) && c->dz_csize.reserve(n_chunks * LZD_SLOTS * 2 + 64) &&
		       c->dz_unit.reserve(dz_unit_layout(b, nullptr, n_units, n_chunks) + 24);
	}
	return (!store || c->dz_tok.reserve(slots * 4 + 256)) && c->dz_ntok.reserve((n_units + 1) * 8) &&
	       (format != MSCOMP_XPRESS_HUFF || c->dz_xhc.reserve(dz_xhc_layout(xb, nullptr, n_units, cands) + 64));
}

// The table and the scratch of a plan's segment walk, for nb streams of sg segments in all, and of its all-CU stage, for nb units of tb token
// blocks, tl tiles and wd words: the counts of a host plan, the bounds of a dev plan with large units (whose tables end with the counts of
// an execution). false: not to be had, the plan's path stays off.
bool msc::reserve_xps(mscomp_amd_plan* p, size_t nb, uint64_t sg)
{
	DevPaths d; XpsTables x;
	if (!p->xps_tab.reserve(xps_tab_layout(d, nullptr, nb, p->large)) || !p->ctx->xps_buf.reserve(xps_buf_layout(x, nullptr, sg, nb, p->n_units) + 64)) { return false; }
	xps_tab_layout(p->paths, p->xps_tab.p, nb, p->large);
	p->paths.xps_max = p->xps_big = (uint32_t)nb; p->paths.xps_seg_max = p->xps_seg = (uint32_t)sg; p->paths.xps_seg_bytes = p->xps_seg_bytes = env_xps_seg(); p->xps_warm_bytes = env_xps_warm();
	return true;
}
bool msc::reserve_lzg(mscomp_amd_plan* p, size_t nb, uint64_t tb, uint64_t tl, uint64_t wd)
{
	DevPaths d; LzgTables g;
	mscomp_amd_ctx* c = p->ctx;
	if (!p->lzg_tab.reserve(lzg_tab_layout(d, nullptr, nb, p->large)) || !c->lzg_bsum.reserve(tb * 8 + 64) || !c->lzg_dir.reserve(lzg_dir_layout(g, nullptr, tl) + 64) ||
	    !c->lzg_words.reserve(lzg_words_layout(g, nullptr, wd, tl) + 64)) { p->lzg_tab.release(); (void)hipGetLastError(); return false; }
	lzg_tab_layout(p->paths, p->lzg_tab.p, nb, p->large);
	p->paths.lzg_max = p->lzg_big = (uint32_t)nb; p->paths.lzg_tb_max = p->lzg_tb = (uint32_t)tb; p->paths.lzg_tile_max = p->lzg_tiles = (uint32_t)tl; p->paths.lzg_word_max = p->lzg_words = wd;
	return true;
}

// ---- the steps of plan_create_impl ----
// Staging of the unit tables of a compress plan: the context's pinned memory, grown as needed, so that the copy goes up stream-ordered and
// the creation does not wait for the stream. null: not to be had (the caller stages in a vector and waits, as every decompress plan does:
// those upload more tables)
static uint64_t* pinned_staging(mscomp_amd_ctx* c, size_t bytes)
{
	if (c->h_tab_busy) { (void)hipEventSynchronize(c->h_tab_ev); c->h_tab_busy = false; }   // (the previous plan's copy: long done)
	if (c->h_tab_cap < bytes) {
		if (c->h_tab) { (void)hipHostFree(c->h_tab); c->h_tab = nullptr; c->h_tab_cap = 0; }
		const size_t want = bytes + bytes / 8 + 4096;
		if (hipHostMalloc(&c->h_tab, want, hipHostMallocDefault) == hipSuccess) { c->h_tab_cap = want; } else { c->h_tab = nullptr; (void)hipGetLastError(); }
	}
	if (c->h_tab && !c->h_tab_ev && hipEventCreateWithFlags(&c->h_tab_ev, hipEventDisableTiming) != hipSuccess) { c->h_tab_ev = nullptr; (void)hipGetLastError(); }
	return c->h_tab && c->h_tab_ev ? static_cast<uint64_t*>(c->h_tab) : nullptr;
}
// The table pool of a context. A new plan takes the smallest pooled buffer that is large enough (else reserve_tables makes a new one) ...
static void pool_pick(mscomp_amd_plan* p, size_t bytes)
{
	std::vector<DevBuf>& pool = p->ctx->table_pool;
	size_t best = pool.size();
	for (size_t i = 0; i < pool.size(); ++i) { if (pool[i].cap >= bytes && (best == pool.size() || pool[i].cap < pool[best].cap)) { best = i; } }
	if (best < pool.size()) { p->tables = pool[best]; p->tables.asked = 0; pool.erase(pool.begin() + (long)best); }   // (asked: this plan's own, from its reserve)
}
// ... and a destroyed plan's goes back. The pool keeps the 8 LARGEST buffers it has seen: a full pool gives up its smallest one for a larger
// one (a pool full of small buffers made every larger plan hipFree on destroy -- a device-wide wait)
static void pool_return(mscomp_amd_plan* p)
{
	std::vector<DevBuf>& pool = p->ctx->table_pool;
	if (!p->tables.p) { return; }
	if (pool.size() < 8) { pool.push_back(p->tables); p->tables.p = nullptr; p->tables.cap = 0; return; }
	size_t least = 0;
	for (size_t i = 1; i < pool.size(); ++i) { if (pool[i].cap < pool[least].cap) { least = i; } }
	if (pool[least].cap < p->tables.cap) { DevBuf t = pool[least]; pool[least] = p->tables; p->tables = t; }   // (the smaller one is released with the plan)
}
static MSCompStatus decode_prefixes(mscomp_amd_plan* p, const uint64_t* in_len, const uint64_t* out_cap, bool& okd);
static MSCompStatus choose_lzg(mscomp_amd_plan* p, const uint64_t* in_len, const uint64_t* out_cap);
static MSCompStatus choose_xps(mscomp_amd_plan* p, const uint64_t* in_len, bool& okd);

MSCompStatus msc::plan_create_impl(mscomp_amd_ctx* c, MSCompFormat format, bool decompress, size_t n_units, const uint64_t* in_off, const uint64_t* in_len,
                                   const uint64_t* out_off, const uint64_t* out_cap, mscomp_amd_plan** out, bool sizing)
{
	if (!creator_args(c, n_units, known_format(format), out) || (n_units && (!in_off || !in_len || !out_off || !out_cap))) { return MSCOMP_ARG_ERROR; }
	DeviceGuard g(c->device);
	if (!g.ok) { return MSCOMP_ERRNO; }
	std::unique_ptr<mscomp_amd_plan> p(new (std::nothrow) mscomp_amd_plan());   // (every return below that is not the last one gives up the plan and what it holds)
	if (!p) { return MSCOMP_MEM_ERROR; }
	p->ctx = c; p->format = format; p->decompress = decompress; p->sizing = sizing; p->n_units = (uint32_t)n_units; p->run.never = n_units == 0;
	p->lznt1_sa = !decompress && format == MSCOMP_LZNT1 && lznt1_sa_for(c);

	PlanCols hc;                                         // the columns in the staging memory, filled below
	const size_t bytes = tables_layout(hc, nullptr, n_units, false, false, false) + 8;
	std::vector<uint64_t> host;
	uint64_t* h = decompress ? nullptr : pinned_staging(c, bytes);
	const bool pinned = h != nullptr;
	if (!pinned) { host.resize(bytes / 8); h = host.data(); }
	tables_layout(hc, h, n_units, false, false, false);
	uint64_t chunks = 0, total = 0;
	for (size_t i = 0; i < n_units; ++i) {
		hc.in_off[i] = in_off[i]; hc.in_len[i] = in_len[i]; hc.out_off[i] = out_off[i]; hc.out_cap[i] = out_cap[i];
		hc.chunk_prefix[i] = (uint32_t)chunks;
		if (decompress && in_len[i] > 0xFFFFF000u) { return MSCOMP_ARG_ERROR; }   // offsets inside a unit are 32-bit (4 GiB - 4096 at most)
		chunks += decompress ? decode_chunks(format, in_len[i]) : compress_chunks(format, in_len[i]);
		total += in_len[i];
		if (in_len[i] > p->max_unit) { p->max_unit = in_len[i]; }
		if (chunks > 0x7FFFFFF0u) { return MSCOMP_ARG_ERROR; }
	}
	hc.chunk_prefix[n_units] = (uint32_t)chunks;
	p->n_chunks = (uint32_t)chunks;
	p->total_in = total;
	pool_pick(p.get(), bytes);
	if (!reserve_tables(p.get())) { return MSCOMP_MEM_ERROR; }
	if (hipMemcpyAsync(p->tables.p, h, bytes, hipMemcpyHostToDevice, c->stream) != hipSuccess) { return MSCOMP_ERRNO; }
	if (pinned) { if (hipEventRecord(c->h_tab_ev, c->stream) != hipSuccess) { return MSCOMP_ERRNO; } c->h_tab_busy = true; }
	else if (hipStreamSynchronize(c->stream) != hipSuccess) { return MSCOMP_ERRNO; }

	if (!decompress) {
		if (!reserve_compress_scratch(c, format, n_units, p->n_chunks, p->lznt1_sa)) { return MSCOMP_MEM_ERROR; }
		*out = p.release();
		return MSCOMP_OK;
	}
	bool okd = reserve_scan(c, p->n_chunks) && (format != MSCOMP_LZNT1 || reserve_decode_scratch(c, format, n_units, p->n_chunks, 0, 0, false));
	MSCompStatus s = MSCOMP_OK;                          // (of a step: not MSCOMP_OK ends the creation; okd = false, out of memory, ends it behind the steps)
	if (okd && format != MSCOMP_LZNT1) { s = decode_prefixes(p.get(), in_len, out_cap, okd); }
	if (s == MSCOMP_OK && okd && !sizing && format != MSCOMP_LZNT1) { s = choose_lzg(p.get(), in_len, out_cap); }
	if (s == MSCOMP_OK && okd && format == MSCOMP_XPRESS) { s = choose_xps(p.get(), in_len, okd); }
	if (s != MSCOMP_OK) { return s; }
	if (!okd) { return MSCOMP_MEM_ERROR; }
	*out = p.release();
	return MSCOMP_OK;
}

// The token / candidate / scratch prefixes of a decompress or size plan of the Xpress formats, and the scratch they count. tokpre: first
// token slot | Xpress+Huffman: first candidate slot | first token-scratch slot of every unit. A size plan writes no tokens (its token prefix
// stays zero; an Xpress size plan has no table at all)
static MSCompStatus decode_prefixes(mscomp_amd_plan* p, const uint64_t* in_len, const uint64_t* out_cap, bool& okd)
{
	mscomp_amd_ctx* c = p->ctx;
	const MSCompFormat format = p->format; const size_t n_units = p->n_units; const bool sizing = p->sizing;
	const bool xh = format == MSCOMP_XPRESS_HUFF;
	const int rows = xh ? 3 : sizing ? 0 : 1;
	PlanCols tc;                                       // its rows in `tp`, filled here, then in the plan's buffer
	const size_t tp_bytes = tokpre_layout(tc, nullptr, n_units, rows);
	std::vector<uint64_t> tp(tp_bytes / 8);
	tokpre_layout(tc, tp.data(), n_units, rows);
	uint64_t slots = 0, cands = 0, scr = 0;
	for (size_t i = 0; i <= n_units; ++i) {
		if (!sizing) { tc.tok_prefix[i] = slots; }
		if (xh) { tc.cand_prefix[i] = cands; tc.scr_prefix[i] = scr; }
		if (i == n_units) { break; }
		if (!sizing) { slots += token_slots(format, in_len[i], out_cap[i]); }
		if (xh) { cands += candidate_slots(in_len[i], out_cap[i]); }
		if (xh && !sizing) { scr += scratch_slots(in_len[i], out_cap[i]); }   // a buffer of several chunks: its candidates keep their tokens (no second walk)
	}
	if (cands > 0x7FFFFFF0u) { return MSCOMP_ARG_ERROR; }
	p->xhc_slots = (uint32_t)cands;
	okd = p->tokpre.reserve(tp_bytes) && reserve_decode_scratch(c, format, n_units, p->n_chunks, slots, cands, !sizing);
	if (xh) {
		// ... if that scratch is affordable: at most MSCOMP_AMD_XHC_SCR_MAX_MB (default 32 GiB; 0 = always walk twice) and at most half of
		// what the device has free right now; a reservation that fails anyway switches the path off (the second walk needs no scratch)
		const uint64_t need = scr * XHC_SCR * 4 + 64, scr_budget = optional_scratch_budget(env_xhc_scr_budget(), c->dz_scr.cap);
		if (scr && (need > scr_budget || !okd || !c->dz_scr.reserve(need))) { for (size_t i = 0; i <= n_units; ++i) { tc.scr_prefix[i] = 0; } scr = 0; }
		p->xhc_scr = scr;
	}
	if (okd && !tp.empty() && !upload(c, p->tokpre, tp)) { return MSCOMP_ERRNO; }
	tokpre_layout(tc, p->tokpre.p, n_units, rows);
	p->tok_prefix = tc.tok_prefix; p->cand_prefix = tc.cand_prefix; p->scr_prefix = tc.scr_prefix;
	return MSCOMP_OK;
}
// The all-CU byte stage (lzglobal.hip) of a decompress plan of the Xpress formats: whether the plan takes it, and its table. Units with room
// for LZG_MIN_CAP bytes or more get their bytes from all CUs: 4 bytes of scratch per byte of capacity; when that is more than the budget
// (MSCOMP_AMD_LZG_MAX_MB, default 64 GiB of the 288; 0 switches the path off) the block-per-unit kernel takes them
static MSCompStatus choose_lzg(mscomp_amd_plan* p, const uint64_t* in_len, const uint64_t* out_cap)
{
	mscomp_amd_ctx* c = p->ctx;
	const MSCompFormat format = p->format; const size_t n_units = p->n_units;
	const uint64_t budget = optional_scratch_budget(env_lzg_budget(), c->lzg_words.cap);   // ... and never more than half of the free HBM: the block kernel needs none of it
	std::vector<uint32_t> big;
	uint64_t words = 0;
	bool too_large = false;                                       // (32-bit word indices: a unit with room for 4 GiB keeps the whole plan on the block kernel, which every such unit then takes)
	for (size_t i = 0; i < n_units; ++i) { if (lzg_too_large(out_cap[i])) { too_large = true; } else if (lzg_takes(out_cap[i])) { big.push_back((uint32_t)i); words += lzg_words(out_cap[i]); } }
	if (too_large) { big.clear(); }
	// ... and when it pays (common.h lzg_pays)
	uint64_t tot = 0, mx = 0;
	for (uint32_t i : big) { tot += out_cap[i]; mx = out_cap[i] > mx ? out_cap[i] : mx; }
	const bool pays = lzg_pays(tot, mx);
	if (!big.empty() && pays && words * 4 <= budget) {
		const size_t nb = big.size();
		DevPaths h;                                                   // the table's columns in `tab`
		std::vector<uint64_t> tab(lzg_tab_layout(h, nullptr, nb, false) / 8);
		lzg_tab_layout(h, tab.data(), nb, false);
		memcpy(h.lzg_unit, big.data(), nb * 4);
		uint64_t tb = 0, tl = 0, wd = 0;
		for (size_t k = 0; k <= nb; ++k) {
			h.lzg_tb_prefix[k] = tb; h.lzg_tile_prefix[k] = tl; h.lzg_word_prefix[k] = wd;
			if (k == nb) { break; }
			const size_t i = big[k];
			tb += lzg_token_blocks(format, in_len[i], out_cap[i]); tl += lzg_tiles(out_cap[i]); wd += lzg_words(out_cap[i]);
		}
		if (tb < 0x7FFFFFF0ull && tl < 0x7FFFFFF0ull && reserve_lzg(p, nb, tb, tl, wd) && !upload(c, p->lzg_tab, tab)) { return MSCOMP_ERRNO; }
	}
	return MSCOMP_OK;
}
// The segment walk of the large streams of an Xpress decompress or size plan: which units take it, and its table (okd = false: out of memory)
static MSCompStatus choose_xps(mscomp_amd_plan* p, const uint64_t* in_len, bool& okd)
{
	mscomp_amd_ctx* c = p->ctx;
	const size_t n_units = p->n_units;
	std::vector<uint32_t> big;
	for (size_t i = 0; i < n_units; ++i) { if (xps_takes(in_len[i])) { big.push_back((uint32_t)i); } }
	if (!big.empty()) {
		const size_t nb = big.size();
		DevPaths h;
		std::vector<uint64_t> tab(xps_tab_layout(h, nullptr, nb, false) / 8);
		xps_tab_layout(h, tab.data(), nb, false);
		memcpy(h.xps_unit, big.data(), nb * 4);
		const uint32_t seg_b = env_xps_seg();
		uint64_t sg = 0;
		for (size_t k = 0; k <= nb; ++k) { h.xps_seg_prefix[k] = sg; if (k < nb) { sg += xps_segments(in_len[big[k]], seg_b); } }
		okd = sg >= 0x7FFFFFF0ull || reserve_xps(p, nb, sg);
		if (okd && p->xps_big && !upload(c, p->xps_tab, tab)) { return MSCOMP_ERRNO; }
	}
	return MSCOMP_OK;
}

// the body of the three one-call batch entries: the plan just created (s: or the status that refused it) executed, waited for and destroyed
template <class Exec> static MSCompStatus run_once(mscomp_amd_ctx* c, MSCompStatus s, mscomp_amd_plan* p, const Exec& exec)
{
	if (s != MSCOMP_OK) { return s; }
	s = exec();
	DeviceGuard g(c->device);
	if (hipStreamSynchronize(c->stream) != hipSuccess && s == MSCOMP_OK) { s = MSCOMP_ERRNO; }
	mscomp_amd_plan_destroy(p);
	return s;
}

extern "C" {

MSCompStatus mscomp_amd_plan_create(mscomp_amd_ctx* c, MSCompFormat format, size_t n_units, const uint64_t* in_off, const uint64_t* in_len,
                                    const uint64_t* out_off, const uint64_t* out_cap, mscomp_amd_plan** out)
{
	return plan_create_impl(c, format, false, n_units, in_off, in_len, out_off, out_cap, out);
}
MSCompStatus mscomp_amd_plan_create_decompress(mscomp_amd_ctx* c, MSCompFormat format, size_t n_units, const uint64_t* in_off, const uint64_t* in_len,
                                               const uint64_t* out_off, const uint64_t* out_cap, mscomp_amd_plan** out)
{
	return plan_create_impl(c, format, true, n_units, in_off, in_len, out_off, out_cap, out);
}

void mscomp_amd_plan_destroy(mscomp_amd_plan* p)
{
	if (!p) { return; }
	DeviceGuard g(p->ctx->device);
	(void)hipStreamSynchronize(p->ctx->stream);
	pool_return(p);
	delete p;
}

MSCompStatus mscomp_amd_plan_execute(mscomp_amd_plan* p, const uint8_t* d_in, uint8_t* d_out, uint64_t* d_out_len, int32_t* d_status)
{
	if (!p || p->sizing || p->dev || (p->n_units && (!d_out_len || !d_status)) || (p->total_in && !d_in)) { return MSCOMP_ARG_ERROR; }
	DeviceGuard g(p->ctx->device);
	if (!g.ok) { return MSCOMP_ERRNO; }
	if (p->decompress) { note_modes(p); }
	const void* args[8] = { d_in, d_out, d_out_len, d_status };
	return plan_run(p->run, p->ctx, args, [&] { (p->decompress ? decode_launch : compress_launch)(p, d_in, d_out, d_out_len, d_status); });
}

MSCompStatus mscomp_amd_compress_batch(mscomp_amd_ctx* c, MSCompFormat format, size_t n_units,
                                       const uint8_t* d_in, const uint64_t* in_off, const uint64_t* in_len,
                                       uint8_t* d_out, const uint64_t* out_off, const uint64_t* out_cap,
                                       uint64_t* d_out_len, int32_t* d_status)
{
	mscomp_amd_plan* p = nullptr;
	const MSCompStatus s = mscomp_amd_plan_create(c, format, n_units, in_off, in_len, out_off, out_cap, &p);
	return run_once(c, s, p, [&] { return mscomp_amd_plan_execute(p, d_in, d_out, d_out_len, d_status); });
}

MSCompStatus mscomp_amd_decompress_batch(mscomp_amd_ctx* c, MSCompFormat format, size_t n_units,
                                       const uint8_t* d_in, const uint64_t* in_off, const uint64_t* in_len,
                                       uint8_t* d_out, const uint64_t* out_off, const uint64_t* out_cap,
                                       uint64_t* d_out_len, int32_t* d_status)
{
	mscomp_amd_plan* p = nullptr;
	const MSCompStatus s = mscomp_amd_plan_create_decompress(c, format, n_units, in_off, in_len, out_off, out_cap, &p);
	return run_once(c, s, p, [&] { return mscomp_amd_plan_execute(p, d_in, d_out, d_out_len, d_status); });
}

// ---- decompressed-size query (include/mscomp_amd.h): the decoders' walks without the byte stage and without token stores ----
// A size plan is a decompress plan whose out_cap table holds the limits and whose out_off table is zero: the kernels test against out_cap as
// the decoders do, and none of them writes output. Scratch follows the input: no token slots, no lzglobal words, no candidate token scratch.
MSCompStatus mscomp_amd_plan_create_size(mscomp_amd_ctx* c, MSCompFormat format, size_t n_units, const uint64_t* in_off, const uint64_t* in_len,
                                         const uint64_t* limit, mscomp_amd_plan** out)
{
	if (!creator_args(c, n_units, known_format(format), out) || (n_units && (!in_off || !in_len))) { return MSCOMP_ARG_ERROR; }
	std::vector<uint64_t> zero(n_units, 0), lim;
	if (!limit) { lim.assign(n_units, ~(uint64_t)0); limit = lim.data(); }
	return plan_create_impl(c, format, true, n_units, in_off, in_len, zero.data(), limit, out, true);
}

MSCompStatus mscomp_amd_plan_execute_size(mscomp_amd_plan* p, const uint8_t* d_in, uint64_t* d_out_len, uint64_t* d_need, int32_t* d_status)
{
	if (!p || !p->sizing || p->dev || (p->n_units && (!d_out_len || !d_need || !d_status)) || (p->total_in && !d_in)) { return MSCOMP_ARG_ERROR; }
	mscomp_amd_ctx* c = p->ctx;
	DeviceGuard g(c->device);
	if (!g.ok) { return MSCOMP_ERRNO; }
	if (p->n_units) {
		note_modes(p);
		size_launch(p, d_in, d_out_len, d_need, d_status);
		// Xpress / Xpress+Huffman: the smallest capacity that decodes is the length itself (every length test is "does it fit"), and d_out_len is 0
		// for a unit that is not MSCOMP_OK
		if (p->format != MSCOMP_LZNT1) { (void)hipMemcpyAsync(d_need, d_out_len, (size_t)p->n_units * sizeof(uint64_t), hipMemcpyDeviceToDevice, c->stream); }
	}
	return hipGetLastError() == hipSuccess ? MSCOMP_OK : MSCOMP_ERRNO;
}

MSCompStatus mscomp_amd_decompressed_size_batch(mscomp_amd_ctx* c, MSCompFormat format, size_t n_units, const uint8_t* d_in,
                                                const uint64_t* in_off, const uint64_t* in_len, const uint64_t* limit,
                                                uint64_t* d_out_len, uint64_t* d_need, int32_t* d_status)
{
	mscomp_amd_plan* p = nullptr;
	const MSCompStatus s = mscomp_amd_plan_create_size(c, format, n_units, in_off, in_len, limit, &p);
	return run_once(c, s, p, [&] { return mscomp_amd_plan_execute_size(p, d_in, d_out_len, d_need, d_status); });
}

// ---- batch helpers: capacity planning and device-side compaction ----
uint64_t mscomp_amd_plan_layout(MSCompFormat format, size_t n_units, const uint64_t* in_len, uint64_t align, uint64_t* out_off, uint64_t* out_cap)
{
	if (!align) { align = 1; }
	uint64_t pos = 0;
	if (n_units && format != MSCOMP_NONE && !known_format(format)) { return (uint64_t)-1; }
	for (size_t i = 0; i < n_units; ++i) {
		const uint64_t cap = layout_cap((int)format, in_len[i]);     // (common.h: the format's largest output; MSCOMP_NONE, the length)
		if (out_off) { out_off[i] = pos; }
		if (out_cap) { out_cap[i] = cap; }
		pos += (cap + align - 1) / align * align;
	}
	return pos;
}

MSCompStatus mscomp_amd_compact_batch(mscomp_amd_ctx* c, size_t n_units, const uint8_t* d_out, const uint64_t* out_off, const uint64_t* out_cap,
                                      const uint64_t* d_out_len, uint8_t* d_packed, uint64_t* d_packed_off)
{
	if (!c || !d_packed_off || (n_units && (!d_out || !out_off || !out_cap || !d_out_len || !d_packed)) || n_units > 0x7FFFFFF0u) { return MSCOMP_ARG_ERROR; }
	DeviceGuard g(c->device);
	if (!g.ok) { return MSCOMP_ERRNO; }
	if (n_units == 0) { return hipMemsetAsync(d_packed_off, 0, 8, c->stream) == hipSuccess ? MSCOMP_OK : MSCOMP_ERRNO; }
	u64* off; uint32_t* tp;                                // the table's columns in `host`, then in cp_tab
	const size_t bytes = cp_tab_layout(off, tp, nullptr, n_units) + 8;
	std::vector<uint64_t> host(bytes / 8);
	cp_tab_layout(off, tp, host.data(), n_units);
	uint64_t tiles = 0;
	for (size_t i = 0; i < n_units; ++i) {
		off[i] = out_off[i]; tp[i] = (uint32_t)tiles;
		tiles += (out_cap[i] + 65535u) / 65536u;
		if (tiles > 0x7FFFFFF0u) { return MSCOMP_ARG_ERROR; }
	}
	tp[n_units] = (uint32_t)tiles;
	if (!c->cp_tab.reserve(bytes)) { return MSCOMP_MEM_ERROR; }
	if (hipMemcpyAsync(c->cp_tab.p, host.data(), bytes, hipMemcpyHostToDevice, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) { return MSCOMP_ERRNO; }
	cp_tab_layout(off, tp, c->cp_tab.p, n_units);
	launch_compact(c->stream, d_out, off, tp, (uint32_t)n_units, (uint32_t)tiles, d_out_len, d_packed_off, d_packed);
	return hipGetLastError() == hipSuccess ? MSCOMP_OK : MSCOMP_ERRNO;
}

} // extern "C"
