// api.hip -- C-ABI of libmscomp_amd.so (include/mscomp_amd.h): context, plan, batch execution and the
// drop-in one-shot entry points. Host orchestration only; every output byte comes from the HIP kernels.
//
// Reference boundary mirrored here: ms_compress / ms_max_compressed_size (/root/reference/src/mscomp.cpp:96-117),
// lznt1_compress (/root/reference/src/lznt1_compress.cpp:233), xpress_compress (/root/reference/src/xpress_compress.cpp:240),
// xpress_huff_compress (/root/reference/src/xpress_huff_compress.cpp:247).
#include "host.h"
#include <mutex>
#include <thread>
#include <condition_variable>
#include <string>

using namespace msc;

// A captured hipGraph of a plan holds raw scratch pointers and a kernel choice. Two counters say when it is stale:
// the context's own epoch (bumped whenever one of ITS device buffers moves; a context is used by one host thread at a
// time, so a plain counter) and a process-wide one for the test hooks that switch kernels (atomic: any thread may call them
// while other threads execute plans; host.h declares it for the other host files).
std::atomic<uint64_t> msc::g_mode_epoch{1};
// The mscomp_amd_debug_set_* hooks pick between bit-identical kernels for the tests. They are process-wide, so the product ignores them unless the
// process asked for them BEFORE the library was loaded (MSCOMP_AMD_TEST_HOOKS=1: tests/conftest.py and the tools do): a deployment cannot have its
// kernels switched under it by a stray call.
bool msc::test_hooks_on() { static const bool on = [] { const char* e = getenv("MSCOMP_AMD_TEST_HOOKS"); return e && *e == '1'; }(); return on; }

namespace {

static std::atomic<int> g_finder_mode{1};              // 1 = default (Xpress units up to 64 KiB: the lazy finder, xpress_lazy.hip), 2 = Find for every position everywhere
static int lznt1_sa_env() { const char* e = getenv("MSCOMP_AMD_LZNT1_SA_DICT"); return (e && *e && *e != '0') ? 1 : 0; }
static std::atomic<int> g_lznt1_sa{lznt1_sa_env()};    // 1 = LZNT1 compresses with the suffix-array dictionary flavour (lznt1_sa.hip; the reference's MSCOMP_WITH_LZNT1_SA_DICT build)
static std::atomic<int> g_one_zero_copy{[] { const char* e = getenv("MSCOMP_AMD_ONE_ZEROCOPY"); return (e && *e == '0') ? 0 : 1; }()};   // large host-pointer LZNT1 calls: 1 = caller buffers mapped, one launch (default), 0 = slices on three streams
static std::atomic<int> g_xpd_mode{0};                 // Xpress decompression: 0 = tokens a flag word at a time + copy kernels (default; large streams by segments), 1 = xpd_kernel (a token at a time, bytes in the same wave), 2 = as 0 without the segments
const uint32_t XH_FB_BLOCKS = 256;                     // persistent blocks of the fallback kernel (one per CU: its package pool fills the LDS)
// the flavour a plan created in `c` right now would get
bool lznt1_sa_for(const mscomp_amd_ctx* c) { return (c->lznt1_sa >= 0 ? c->lznt1_sa : g_lznt1_sa.load(std::memory_order_relaxed)) != 0; }

// Bytes an OPTIONAL fast-path scratch buffer may take: the environment's cap, and never more than half of what the device has free
// right now (what the buffer already holds counts as free: reserve() reuses it). The fast paths have fallbacks that need no scratch,
// so a plan never fails for them (the constants above assume a 288 GB device that is otherwise empty; a caller may hold most of it).
uint64_t optional_scratch_budget(uint64_t env_cap, size_t already_held)
{
	size_t free_b = 0, total_b = 0;
	if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); return env_cap; }
	const uint64_t half = ((uint64_t)free_b + already_held) / 2;
	return env_cap < half ? env_cap : half;
}

} // namespace

extern "C" {

const char* mscomp_amd_version(void) { return "mscomp_amd 0.6 (gfx950, HIP; LZNT1 / Xpress / Xpress+Huffman compressors and decompressors, LZNT1 streaming, host batches over several GPUs)"; }

size_t lznt1_max_compressed_size(size_t n)       { return lznt1_max_out(n); }
size_t xpress_max_compressed_size(size_t n)      { return xpress_max_out(n); }
size_t xpress_huff_max_compressed_size(size_t n) { return xpress_huff_max_out(n); }
#ifndef MSCOMP_AMD_NO_FACADE   /* define when src/mscomp.cpp of the reference is linked too */
size_t ms_max_compressed_size(MSCompFormat f, size_t n)
{
	switch ((int)f) {
	case MSCOMP_NONE:        return n;
	case MSCOMP_LZNT1:       return lznt1_max_compressed_size(n);
	case MSCOMP_XPRESS:      return xpress_max_compressed_size(n);
	case MSCOMP_XPRESS_HUFF: return xpress_huff_max_compressed_size(n);
	default:                 return (size_t)-1;                          // mscomp.cpp:98
	}
}
#endif

// The LZNT1 bucket sort and the Xpress chain links are only bit-exact when the returning same-address LDS atomics of one
// wave instruction are served in lane order (util.hip: lds_lane_order_kernel). That is how gfx950 behaves, but it is not an
// architectural promise, so the library checks the device it is about to use, once per device and process. A device that serves them in
// another order gets the order-independent form of the two kernels (one lane at a time: kernels.h set_serial_atomics -- the same bytes,
// a slower sort); a device on which the check cannot RUN is refused (MSCOMP_ERRNO): wrong bytes must never leave silently.
static int lane_order_verdict(int device, hipStream_t st)
{
	static std::mutex mu;
	static int verdict[64];                            // 0 = unknown, 1 = in order, -1 = out of order / check failed
	if (device >= 64) { device = 63; }
	std::lock_guard<std::mutex> lk(mu);
	if (verdict[device] == 0) {
		uint32_t* d_bad = nullptr;
		uint32_t bad = 0xFFFFFFFFu;
		if (hipMalloc(reinterpret_cast<void**>(&d_bad), 64) == hipSuccess) {
			bad = run_lds_lane_order_check(st, 0x5EEDu + (uint32_t)device, 64, 64, 97, d_bad);     // 64 blocks x 64 rounds x 64 lanes x {add, exchange}
			if (bad == 0) { bad = run_lds_lane_order_check(st, 0xC0FFEEu, 64, 64, 2048, d_bad); }
			(void)hipFree(d_bad);
		}
		verdict[device] = bad == 0 ? 1 : (bad == 0xFFFFFFFFu ? -1 : 2);             // 2 = runs, out of order: the serial form
		if (verdict[device] == 2) { set_serial_atomics(device, 1); }
	}
	return verdict[device];
}

MSCompStatus mscomp_amd_ctx_create(int device, void* hip_stream, mscomp_amd_ctx** out)
{
	if (!out) { return MSCOMP_ARG_ERROR; }
	*out = nullptr;
	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) { return MSCOMP_ERRNO; }
	DeviceGuard g(device);
	if (!g.ok) { return MSCOMP_ERRNO; }
	if (lane_order_verdict(device, (hipStream_t)hip_stream) < 1) { return MSCOMP_ERRNO; }
	mscomp_amd_ctx* c = new (std::nothrow) mscomp_amd_ctx();
	if (!c) { return MSCOMP_MEM_ERROR; }
	c->device = device; c->stream = (hipStream_t)hip_stream;
	c->cpd_blocks = compact_dev_blocks();
	c->crc_blocks = crc_dev_blocks();
	(void)place_blocks(false); (void)place_blocks(true);           // (the grid of the LZNT1 placement, kept per device in util.hip: asked here, not inside a capture)
	*out = c;
	return MSCOMP_OK;
}

void mscomp_amd_ctx_destroy(mscomp_amd_ctx* c)
{
	if (!c) { return; }
	DeviceGuard g(c->device);
	(void)hipStreamSynchronize(c->stream);
	for (auto& r : c->recs) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
	for (auto e : c->free_events) { (void)hipEventDestroy(e); }
	for (DevBuf* b : c->bufs()) { b->release(); }
	for (DevBuf& b : c->table_pool) { b.release(); }
	if (c->h_tab) { (void)hipHostFree(c->h_tab); }
	if (c->h_tab_ev) { (void)hipEventDestroy(c->h_tab_ev); }
	delete c;
}

void mscomp_amd_profile_enable(mscomp_amd_ctx* c, int on) { if (c) { c->profiling = on != 0; } }

int mscomp_amd_profile_read(mscomp_amd_ctx* c, const char** names, double* ms, uint64_t* launches, int cap)
{
	if (!c) { return 0; }
	DeviceGuard g(c->device);
	(void)hipStreamSynchronize(c->stream);
	int n = 0;
	for (auto& r : c->recs) {
		float t = 0.f; (void)hipEventElapsedTime(&t, r.a, r.b);
		int k = 0;
		for (; k < n; ++k) { if (names[k] == r.name) { break; } }
		if (k == n) { if (n >= cap) { continue; } names[n] = r.name; ms[n] = 0; launches[n] = 0; ++n; }
		ms[k] += t; launches[k] += 1;
		c->free_events.push_back(r.a); c->free_events.push_back(r.b);
	}
	c->recs.clear();
	return n;
}

// `tables` of the plan, reserved for its kind and counts (tables_layout), and what the launch code reads of it: bt, the prefixes and reject
// of a dev plan (the launch functions do not know where a creator put them)
static bool reserve_tables(mscomp_amd_plan* p)
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
static bool reserve_compress_scratch(mscomp_amd_ctx* c, MSCompFormat format, size_t n_units, size_t n_chunks, bool lznt1_sa)
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
static bool reserve_decode_scratch(mscomp_amd_ctx* c, MSCompFormat format, size_t n_units, size_t n_chunks, uint64_t slots, uint64_t cands, bool store)
{
	LzdBufs b; XhcBufs xb;
	if (format == MSCOMP_LZNT1) {
		return reserve_scan(c, n_chunks) && c->dz_cin.reserve(n_chunks * LZD_SLOTS * 4 + 64) && c->dz_csize.reserve(n_chunks * LZD_SLOTS * 2 + 64) &&
		       c->dz_unit.reserve(dz_unit_layout(b, nullptr, n_units, n_chunks) + 24);
	}
	return (!store || c->dz_tok.reserve(slots * 4 + 256)) && c->dz_ntok.reserve((n_units + 1) * 8) &&
	       (format != MSCOMP_XPRESS_HUFF || c->dz_xhc.reserve(dz_xhc_layout(xb, nullptr, n_units, cands) + 64));
}

// ---- the optional paths: their environment settings (read once), for host plans and for the bounds of dev plans with large units ----
// segment size / warm-up of the segment walk (MSCOMP_AMD_XPS_SEG_KB / _WARM_KB override the defaults, for measurements)
static uint32_t xps_seg_env() { static const uint32_t b = [] { const char* e = getenv("MSCOMP_AMD_XPS_SEG_KB"); const long v = e ? atol(e) : 0; return (uint32_t)(v >= 4 && v <= 65536 ? v << 10 : XPS_SEG); }(); return b; }
static uint32_t xps_warm_env() { static const uint32_t b = [] { const char* e = getenv("MSCOMP_AMD_XPS_WARM_KB"); const long v = e ? atol(e) : 0; const uint32_t w = (uint32_t)(v >= 1 && v <= 65536 ? v << 10 : XPS_WARM); return w < xps_seg_env() ? w : xps_seg_env(); }(); return b; }
// the all-CU byte stage: MSCOMP_AMD_LZG_MAX_MB, default 64 GiB of the 288; 0 switches the path off
static uint64_t lzg_budget_env() { static const uint64_t b = [] { const char* e = getenv("MSCOMP_AMD_LZG_MAX_MB"); const long long v = e ? atoll(e) : 65536; return (uint64_t)(v < 0 ? 0 : v) << 20; }(); return b; }
// the candidate token scratch: MSCOMP_AMD_XHC_SCR_MAX_MB, default 32 GiB; 0 = always walk twice
static uint64_t xhc_scr_env() { static const uint64_t b = [] { const char* e = getenv("MSCOMP_AMD_XHC_SCR_MAX_MB"); const long long v = e ? atoll(e) : 32768; return (uint64_t)(v < 0 ? 0 : v) << 20; }(); return b; }
// The table and the scratch of a plan's segment walk, for nb streams of sg segments in all, and of its all-CU stage, for nb units of tb token
// blocks, tl tiles and wd words: the counts of a host plan, the bounds of a dev plan with large units (whose tables end with the counts of
// an execution). false: not to be had, the plan's path stays off.
static bool reserve_xps(mscomp_amd_plan* p, size_t nb, uint64_t sg)
{
	DevPaths d; XpsTables x;
	if (!p->xps_tab.reserve(xps_tab_layout(d, nullptr, nb, p->large)) || !p->ctx->xps_buf.reserve(xps_buf_layout(x, nullptr, sg, nb, p->n_units) + 64)) { return false; }
	xps_tab_layout(p->paths, p->xps_tab.p, nb, p->large);
	p->paths.xps_max = p->xps_big = (uint32_t)nb; p->paths.xps_seg_max = p->xps_seg = (uint32_t)sg; p->paths.xps_seg_bytes = p->xps_seg_bytes = xps_seg_env(); p->xps_warm_bytes = xps_warm_env();
	return true;
}
static bool reserve_lzg(mscomp_amd_plan* p, size_t nb, uint64_t tb, uint64_t tl, uint64_t wd)
{
	DevPaths d; LzgTables g;
	mscomp_amd_ctx* c = p->ctx;
	if (!p->lzg_tab.reserve(lzg_tab_layout(d, nullptr, nb, p->large)) || !c->lzg_bsum.reserve(tb * 8 + 64) || !c->lzg_dir.reserve(lzg_dir_layout(g, nullptr, tl) + 64) ||
	    !c->lzg_words.reserve(lzg_words_layout(g, nullptr, wd, tl) + 64)) { p->lzg_tab.release(); (void)hipGetLastError(); return false; }
	lzg_tab_layout(p->paths, p->lzg_tab.p, nb, p->large);
	p->paths.lzg_max = p->lzg_big = (uint32_t)nb; p->paths.lzg_tb_max = p->lzg_tb = (uint32_t)tb; p->paths.lzg_tile_max = p->lzg_tiles = (uint32_t)tl; p->paths.lzg_word_max = p->lzg_words = wd;
	return true;
}

static MSCompStatus plan_create_impl(mscomp_amd_ctx* c, MSCompFormat format, bool decompress, size_t n_units,
                                     const uint64_t* in_off, const uint64_t* in_len,
                                     const uint64_t* out_off, const uint64_t* out_cap, mscomp_amd_plan** out, bool sizing = false)
{
	if (!out) { return MSCOMP_ARG_ERROR; }
	*out = nullptr;
	if (!c || (n_units && (!in_off || !in_len || !out_off || !out_cap)) || n_units > 0x7FFFFFF0u) { return MSCOMP_ARG_ERROR; }
	if (!known_format(format)) { return MSCOMP_ARG_ERROR; }
	DeviceGuard g(c->device);
	if (!g.ok) { return MSCOMP_ERRNO; }
	std::unique_ptr<mscomp_amd_plan> p(new (std::nothrow) mscomp_amd_plan());   // (every return below that is not the last one gives up the plan and what it holds)
	if (!p) { return MSCOMP_MEM_ERROR; }
	p->ctx = c; p->format = format; p->decompress = decompress; p->sizing = sizing; p->n_units = (uint32_t)n_units; p->run.never = n_units == 0;
	p->lznt1_sa = !decompress && format == MSCOMP_LZNT1 && lznt1_sa_for(c);

	PlanCols hc;                                         // the columns in the staging memory, filled below
	const size_t bytes = tables_layout(hc, nullptr, n_units, false, false, false) + 8;
	std::vector<uint64_t> host;
	uint64_t* h = nullptr;
	if (!decompress) {                                   // compress plans: pinned staging, no stream wait (the decompress plans below upload more tables and wait as before)
		if (c->h_tab_busy) { (void)hipEventSynchronize(c->h_tab_ev); c->h_tab_busy = false; }   // (the previous plan's copy: long done)
		if (c->h_tab_cap < bytes) {
			if (c->h_tab) { (void)hipHostFree(c->h_tab); c->h_tab = nullptr; c->h_tab_cap = 0; }
			const size_t want = bytes + bytes / 8 + 4096;
			if (hipHostMalloc(&c->h_tab, want, hipHostMallocDefault) == hipSuccess) { c->h_tab_cap = want; } else { c->h_tab = nullptr; (void)hipGetLastError(); }
		}
		if (c->h_tab && !c->h_tab_ev && hipEventCreateWithFlags(&c->h_tab_ev, hipEventDisableTiming) != hipSuccess) { c->h_tab_ev = nullptr; (void)hipGetLastError(); }
		if (c->h_tab && c->h_tab_ev) { h = static_cast<uint64_t*>(c->h_tab); }
	}
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
	{	// the smallest pooled buffer that is large enough, else a new one
		size_t best = c->table_pool.size();
		for (size_t i = 0; i < c->table_pool.size(); ++i) { if (c->table_pool[i].cap >= bytes && (best == c->table_pool.size() || c->table_pool[i].cap < c->table_pool[best].cap)) { best = i; } }
		if (best < c->table_pool.size()) { p->tables = c->table_pool[best]; p->tables.asked = 0; c->table_pool.erase(c->table_pool.begin() + (long)best); }   // (asked: this plan's own, from the reserve below)
	}
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
	if (okd && format != MSCOMP_LZNT1) {
		// tokpre: first token slot | Xpress+Huffman: first candidate slot | first token-scratch slot of every unit. A size plan writes no
		// tokens (its token prefix stays zero; an Xpress size plan has no table at all)
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
			const uint64_t need = scr * XHC_SCR * 4 + 64, scr_budget = optional_scratch_budget(xhc_scr_env(), c->dz_scr.cap);
			if (scr && (need > scr_budget || !okd || !c->dz_scr.reserve(need))) { for (size_t i = 0; i <= n_units; ++i) { tc.scr_prefix[i] = 0; } scr = 0; }
			p->xhc_scr = scr;
		}
		if (okd && !tp.empty() && !upload(c, p->tokpre, tp)) { return MSCOMP_ERRNO; }
		tokpre_layout(tc, p->tokpre.p, n_units, rows);
		p->tok_prefix = tc.tok_prefix; p->cand_prefix = tc.cand_prefix; p->scr_prefix = tc.scr_prefix;
	}
	if (okd && !sizing && (format == MSCOMP_XPRESS || format == MSCOMP_XPRESS_HUFF)) {
		// units with room for LZG_MIN_CAP bytes or more get their bytes from all CUs (lzglobal.hip): 4 bytes of scratch per byte of capacity;
		// when that is more than the budget (MSCOMP_AMD_LZG_MAX_MB, default 64 GiB of the 288; 0 switches the path off) the block-per-unit kernel takes them
		const uint64_t budget = optional_scratch_budget(lzg_budget_env(), c->lzg_words.cap);   // ... and never more than half of the free HBM: the block kernel needs none of it
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
			if (tb < 0x7FFFFFF0ull && tl < 0x7FFFFFF0ull && reserve_lzg(p.get(), nb, tb, tl, wd) && !upload(c, p->lzg_tab, tab)) { return MSCOMP_ERRNO; }
		}
	}
	if (okd && format == MSCOMP_XPRESS) {
		std::vector<uint32_t> big;
		for (size_t i = 0; i < n_units; ++i) { if (xps_takes(in_len[i])) { big.push_back((uint32_t)i); } }
		if (!big.empty()) {
			const size_t nb = big.size();
			DevPaths h;
			std::vector<uint64_t> tab(xps_tab_layout(h, nullptr, nb, false) / 8);
			xps_tab_layout(h, tab.data(), nb, false);
			memcpy(h.xps_unit, big.data(), nb * 4);
			const uint32_t seg_b = xps_seg_env();
			uint64_t sg = 0;
			for (size_t k = 0; k <= nb; ++k) { h.xps_seg_prefix[k] = sg; if (k < nb) { sg += xps_segments(in_len[big[k]], seg_b); } }
			okd = sg >= 0x7FFFFFF0ull || reserve_xps(p.get(), nb, sg);
			if (okd && p->xps_big && !upload(c, p->xps_tab, tab)) { return MSCOMP_ERRNO; }
		}
	}
	if (!okd) { return MSCOMP_MEM_ERROR; }
	*out = p.release();
	return MSCOMP_OK;
}

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
	if (p->tables.p) {
		// the pool keeps the 8 LARGEST buffers it has seen: a full pool gives up its smallest one for a larger one (a pool full of
		// small buffers made every larger plan hipFree on destroy -- a device-wide wait)
		std::vector<DevBuf>& pool = p->ctx->table_pool;
		if (pool.size() < 8) { pool.push_back(p->tables); p->tables.p = nullptr; p->tables.cap = 0; }
		else {
			size_t least = 0;
			for (size_t i = 1; i < pool.size(); ++i) { if (pool[i].cap < pool[least].cap) { least = i; } }
			if (pool[least].cap < p->tables.cap) { DevBuf t = pool[least]; pool[least] = p->tables; p->tables = t; }   // (the smaller one is released with the plan)
		}
	}
	delete p;
}

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
extern "C++" void msc::note_modes(mscomp_amd_plan* p)
{
	mscomp_amd_ctx* c = p->ctx;
	c->dbg_mode = nullptr; c->dbg_mode_n = 0; c->dbg_mode_cnt = nullptr;
	c->dbg_lzg_open = p->large && p->lzg_big ? lzg_tables(p, c).open : nullptr;
	if (p->format == MSCOMP_XPRESS_HUFF && p->n_units) { c->dbg_mode = xhc_bufs(c, p).mode; c->dbg_mode_n = p->n_units; }
	if (p->format == MSCOMP_XPRESS && p->xps_big && (p->sizing || p->large || g_xpd_mode.load(std::memory_order_relaxed) == 0)) { c->dbg_mode = xps_tables(p, c).mode; c->dbg_mode_n = p->xps_big; c->dbg_mode_cnt = p->paths.xps_cnt; }
}

// ---- the launch sequences: one per direction, for host-table and device-table plans alike ----
// A dev plan runs the DEV instances of the chunk-gridded kernels (p->dev: bt.n_chunks is its bound, the blocks past chunk_prefix[n_units] return at
// once); its table pass goes in front of these launches and its reject pass behind them, at the call site (mscomp_amd_plan_execute_dev /
// _execute_size_dev). The optional paths -- xps_* segments, the lzglobal.hip stage, Xpress+Huffman token scratch -- are off for a plain dev plan
// by their zero counts; a dev plan with large units (p->large) has their bounds in the same fields, a path pass behind its table pass that
// builds their tables, and runs the DEV instances of their kernels, which read the counts of the execution from device memory.
static void decode_launch(mscomp_amd_plan* p, const uint8_t* d_in, uint8_t* d_out, uint64_t* d_out_len, int32_t* d_status)
{
	mscomp_amd_ctx* c = p->ctx;
	hipStream_t st = c->stream;
	const u64* tp = p->tok_prefix; uint32_t* tok = static_cast<uint32_t*>(c->dz_tok.p); u64* ntok = static_cast<u64*>(c->dz_ntok.p);
	const u64 gmin = p->lzg_big ? (u64)LZG_MIN_CAP : ~(u64)0;           // (host plans; p->large: the byte kernels read lzg_cnt instead)
	const uint32_t* gcnt = p->large && p->lzg_big ? p->paths.lzg_cnt : nullptr;
	switch (p->format) {
	case MSCOMP_LZNT1: {
		const LzdBufs b = lzd_bufs(c, p);
		if (p->dev) { launch_dev_zero(st, b.selcnt, p->n_chunks); }       // segments past the real count add nothing to the scan (a kernel, no memset: the launches may go into a caller's graph)
		{ KernelTimer t(c, "lzd_seg_kernel"); launch_lzd_segments(st, d_in, p->bt, b, p->dev); }
		{ KernelTimer t(c, "lzd_verify_kernel"); launch_lzd_verify(st, d_in, p->bt, b); }
		{ KernelTimer t(c, "scan_sizes"); launch_scan_sizes(st, b.selcnt, b.flat, p->n_chunks, static_cast<u64*>(c->tile_sums.p)); }
		{ KernelTimer t(c, "lzd_chunk_kernel"); launch_lzd_chunks(st, d_in, p->bt, b, d_out); }
		{ KernelTimer t(c, "lzd_finalize_kernel"); launch_lzd_finalize(st, p->bt, b, d_out_len, d_status); }
		{ KernelTimer t(c, "lzd_replace_kernel"); launch_lzd_replace(st, d_in, p->bt, b, d_out); }
		return;
	}
	case MSCOMP_XPRESS: {                                          // tokens a flag word at a time, then the copy kernels; large streams of host plans by segments first
		const int mode = p->dev ? (p->large ? 0 : 2) : g_xpd_mode.load(std::memory_order_relaxed);   // (the test hook switches host plans only; a dev plan walks by segments when it was created for large units)
		if (mode == 1) { KernelTimer t(c, "xpd_kernel"); launch_xpress_decompress(st, d_in, p->bt, d_out, d_out_len, d_status); return; }
		const XpsTables x = mode != 2 ? xps_tables(p, c) : XpsTables{};
		if (x.n_big) {
			{ KernelTimer t2(c, "xps_walk_kernel"); launch_xps_walk(st, d_in, p->bt, x); }
			static const uint32_t rounds = [] { const char* e = getenv("MSCOMP_AMD_XPS_ROUNDS"); const long v = e ? atol(e) : 0; return (uint32_t)(v >= 1 && v <= 256 ? v : XPS_ROUNDS); }();
			for (uint32_t r = 0; r < rounds; ++r) { KernelTimer t2(c, "xps_redo_kernels"); launch_xps_redo(st, d_in, p->bt, x, ntok, d_out_len, d_status); }
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
		{ KernelTimer t(c, "xhc_mark_kernel"); launch_xhc_mark(st, d_in, p->bt, p->cand_prefix, xb, p->dev); }
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

static void compress_launch(mscomp_amd_plan* p, const uint8_t* d_in, uint8_t* d_out, uint64_t* d_out_len, int32_t* d_status)
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
			if (g_finder_mode.load(std::memory_order_relaxed) != 2 && p->max_unit <= 65536u) { KernelTimer t(c, "xp_lazy2_kernel"); launch_xp_lazy2(st, d_in, p->bt, links, mlen3, moff, dev); }
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
	MSCompStatus s = mscomp_amd_plan_create(c, format, n_units, in_off, in_len, out_off, out_cap, &p);
	if (s != MSCOMP_OK) { return s; }
	s = mscomp_amd_plan_execute(p, d_in, d_out, d_out_len, d_status);
	DeviceGuard g(c->device);
	if (hipStreamSynchronize(c->stream) != hipSuccess && s == MSCOMP_OK) { s = MSCOMP_ERRNO; }
	mscomp_amd_plan_destroy(p);
	return s;
}

MSCompStatus mscomp_amd_decompress_batch(mscomp_amd_ctx* c, MSCompFormat format, size_t n_units,
                                       const uint8_t* d_in, const uint64_t* in_off, const uint64_t* in_len,
                                       uint8_t* d_out, const uint64_t* out_off, const uint64_t* out_cap,
                                       uint64_t* d_out_len, int32_t* d_status)
{
	mscomp_amd_plan* p = nullptr;
	MSCompStatus s = mscomp_amd_plan_create_decompress(c, format, n_units, in_off, in_len, out_off, out_cap, &p);
	if (s != MSCOMP_OK) { return s; }
	s = mscomp_amd_plan_execute(p, d_in, d_out, d_out_len, d_status);
	DeviceGuard g(c->device);
	if (hipStreamSynchronize(c->stream) != hipSuccess && s == MSCOMP_OK) { s = MSCOMP_ERRNO; }
	mscomp_amd_plan_destroy(p);
	return s;
}

// ---- decompressed-size query (include/mscomp_amd.h): the decoders' walks without the byte stage and without token stores ----
// A size plan is a decompress plan whose out_cap table holds the limits and whose out_off table is zero: the kernels test against out_cap as
// the decoders do, and none of them writes output. Scratch follows the input: no token slots, no lzglobal words, no candidate token scratch.
MSCompStatus mscomp_amd_plan_create_size(mscomp_amd_ctx* c, MSCompFormat format, size_t n_units, const uint64_t* in_off, const uint64_t* in_len,
                                         const uint64_t* limit, mscomp_amd_plan** out)
{
	if (!out) { return MSCOMP_ARG_ERROR; }
	*out = nullptr;
	if (!c || (n_units && (!in_off || !in_len)) || n_units > 0x7FFFFFF0u) { return MSCOMP_ARG_ERROR; }
	if (!known_format(format)) { return MSCOMP_ARG_ERROR; }
	std::vector<uint64_t> zero(n_units, 0), lim;
	if (!limit) { lim.assign(n_units, ~(uint64_t)0); limit = lim.data(); }
	return plan_create_impl(c, format, true, n_units, in_off, in_len, zero.data(), limit, out, true);
}

static void size_launch(mscomp_amd_plan* p, const uint8_t* d_in, uint64_t* d_out_len, uint64_t* d_need, int32_t* d_status)
{
	mscomp_amd_ctx* c = p->ctx;
	hipStream_t st = c->stream;
	u64* ntok = static_cast<u64*>(c->dz_ntok.p);
	switch (p->format) {
	case MSCOMP_LZNT1: {                                   // the header chain as in decode_launch, then every chunk sized, then the verdict at the limit (which writes need)
		const LzdBufs b = lzd_bufs(c, p);
		if (p->dev) { launch_dev_zero(st, b.selcnt, p->n_chunks); }   // (as in decode_launch)
		{ KernelTimer t(c, "lzd_seg_kernel"); launch_lzd_segments(st, d_in, p->bt, b, p->dev); }
		{ KernelTimer t(c, "lzd_verify_kernel"); launch_lzd_verify(st, d_in, p->bt, b); }
		{ KernelTimer t(c, "scan_sizes"); launch_scan_sizes(st, b.selcnt, b.flat, p->n_chunks, static_cast<u64*>(c->tile_sums.p)); }
		{ KernelTimer t(c, "lzd_size_kernel"); launch_lzd_sizes(st, d_in, p->bt, b); }
		{ KernelTimer t(c, "lzd_finalize_kernel"); launch_lzd_finalize(st, p->bt, b, d_out_len, d_status, d_need); }
		break;
	}
	case MSCOMP_XPRESS: {                                  // large streams of host plans by segments, the others (a dev plan: every stream) by the one-wave walk
		const XpsTables x = xps_tables(p, c);
		if (x.n_big) {
			{ KernelTimer t2(c, "xps_walk_kernel"); launch_xps_walk(st, d_in, p->bt, x); }
			for (uint32_t r = 0; r < XPS_ROUNDS; ++r) { KernelTimer t2(c, "xps_redo_kernels"); launch_xps_redo(st, d_in, p->bt, x, ntok, d_out_len, d_status); }
			{ KernelTimer t2(c, "xps_size_kernel"); launch_xps_size(st, d_in, p->bt, x, ntok, d_out_len, d_status); }
		}
		{ KernelTimer t(c, "xpt_size_kernel"); launch_xpt_size(st, d_in, p->bt, ntok, d_out_len, d_status, x); }
		break;
	}
	default: {                                             // MSCOMP_XPRESS_HUFF
		const XhcBufs xb = xhc_bufs(c, p);
		{ KernelTimer t(c, "xhc_mark_kernel"); launch_xhc_mark(st, d_in, p->bt, p->cand_prefix, xb, p->dev); }
		{ KernelTimer t(c, "xhc_size_kernel"); launch_xhc_candidates_size(st, d_in, p->bt, p->cand_prefix, p->xhc_slots, xb); }
		{ KernelTimer t(c, "xhc_chain_kernel"); launch_xhc_chain(st, p->bt, p->cand_prefix, xb, ntok, d_out_len, d_status); }
		{ KernelTimer t(c, "xhd_size_kernel"); launch_xhd_size(st, d_in, p->bt, ntok, d_out_len, d_status, xb.mode); }
		break;
	}
	}
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
	MSCompStatus s = mscomp_amd_plan_create_size(c, format, n_units, in_off, in_len, limit, &p);
	if (s != MSCOMP_OK) { return s; }
	s = mscomp_amd_plan_execute_size(p, d_in, d_out_len, d_need, d_status);
	DeviceGuard g(c->device);
	if (hipStreamSynchronize(c->stream) != hipSuccess && s == MSCOMP_OK) { s = MSCOMP_ERRNO; }
	mscomp_amd_plan_destroy(p);
	return s;
}

// ---- plans with device tables (include/mscomp_amd.h): created from bounds, tables built on the device by every execution ----
// The plan holds its bounds and scratch sized for them; p->tables holds what the table pass (devplan.hip) writes each time (tables_layout).

// The optional paths of a dev plan with large units (Xpress formats): tables and scratch for the most that a batch within the plan's bounds
// can put on each path, by the thresholds of common.h. N units, I input bytes, O bytes of capacity, toks token slots at most (create_decode_dev):
//   segment walk    a stream taken has XPS_MIN_IN bytes or more: min(N, I / XPS_MIN_IN) streams, I / segment + that many segments
//   all-CU stage    a unit taken has room for LZG_MIN_CAP bytes or more: B = min(N, O / LZG_MIN_CAP) units, O + 64 B words, O / 8192 + B tiles,
//                   toks / 8192 + B token blocks
//   token scratch   a unit taken has room for more than 65536 bytes: S = min(N, O / 65537) units, whose candidate slots are bounded as the
//                   plan's are, with S for N
// The all-CU stage and the token scratch are optional as in a host plan: over the budget (of the bounds, here) or not to be had, the path is
// off for the life of the plan (its bound stays 0) and the block-per-unit kernel / the second walk take the units. false: out of memory.
static bool reserve_dev_paths(mscomp_amd_plan* p, uint64_t N, uint64_t I, uint64_t O, uint64_t toks)
{
	mscomp_amd_ctx* c = p->ctx;
	if (p->format == MSCOMP_XPRESS) {
		const uint64_t nb = N < I / XPS_MIN_IN ? N : I / XPS_MIN_IN, sg = I / xps_seg_env() + nb;
		if (nb && sg < 0x7FFFFFF0ull && !reserve_xps(p, nb, sg)) { return false; }
	}
	if (p->sizing) { return true; }
	const uint64_t B = N < O / LZG_MIN_CAP ? N : O / LZG_MIN_CAP;
	if (B && O < (1ull << 60)) {
		const uint64_t wd = O + 64 * B, tl = (O >> LZG_TILE_SHIFT) + B, tb = toks / 8192 + B;
		const uint64_t budget = optional_scratch_budget(lzg_budget_env(), c->lzg_words.cap);
		if (wd <= budget / 4 && tb < 0x7FFFFFF0ull && tl < 0x7FFFFFF0ull) { (void)reserve_lzg(p, B, tb, tl, wd); }
	}
	if (p->format == MSCOMP_XPRESS_HUFF) {
		const uint64_t S = N < O / 65537u ? N : O / 65537u;
		const uint64_t by_out = O / 65536u + 2 * S, by_len = I / 260u + S, most = by_out < by_len ? by_out : by_len, scr = most + most / 4 + 2 * S;
		const uint64_t budget = optional_scratch_budget(xhc_scr_env(), c->dz_scr.cap);
		if (S && scr <= budget / (XHC_SCR * 4ull) && scr * XHC_SCR * 4 + 64 <= budget) {
			if (c->dz_scr.reserve(scr * XHC_SCR * 4 + 64)) { p->xhc_scr = scr; p->paths.scr_prefix = p->scr_prefix; } else { (void)hipGetLastError(); }
		}
	}
	return true;
}
static void run_dev_paths(mscomp_amd_plan* p)
{
	if (!p->large || !(p->xps_big || p->lzg_big || p->xhc_scr)) { return; }
	KernelTimer t(p->ctx, "dv_paths_kernel");
	launch_dev_paths(p->ctx->stream, (int)p->format, p->n_units, static_cast<const u64*>(p->tables.p), p->paths);
}

// The bounds of a decompress dev plan's per-unit counts summed over the batch: every accepted unit has in_len <= 0xFFFFF000 and the accepted
// ones sum to at most in_total_max / out_total_max; a rejected unit counts as an empty one (one chunk, 64 token slots, 3 candidates).
// false: more than the tables can address (MSCOMP_MEM_ERROR). Needs no device: a creator calls it before the context is used.
extern "C++" bool msc::decode_dev_counts(MSCompFormat format, uint64_t N, uint64_t in_total_max, uint64_t O, bool sizing, uint64_t& I, uint64_t& chunks, uint64_t& toks, uint64_t& cands)
{
	I = in_total_max < N * 0xFFFFF000ull ? in_total_max : N * 0xFFFFF000ull;
	chunks = N; toks = 0; cands = 0;
	if (format == MSCOMP_LZNT1) { chunks = N + I / LZD_SEG; }
	if (format == MSCOMP_XPRESS_HUFF) { chunks = N + I / XHC_TILE_BYTES; }
	if (chunks > 0x7FFFFFF0ull) { return false; }
	if (format != MSCOMP_LZNT1 && !sizing) {
		const uint64_t by_in = (format == MSCOMP_XPRESS ? 1 : 8) * I + O / 32766u + N;   // (I < 2^45 here for Xpress+Huffman: its chunk bound held)
		toks = (O < by_in ? O : by_in) + 64 * N;
		if (toks > (1ull << 46)) { return false; }
	}
	if (format == MSCOMP_XPRESS_HUFF) {
		const uint64_t by_out = O / 65536u + 2 * N, by_len = I / 260u + N, most = by_out < by_len ? by_out : by_len;
		cands = most + most / 4 + 2 * N;
		if (cands > 0x7FFFFFF0ull) { return false; }
	}
	return true;
}

// Decompress plans, and size plans: a decompress dev plan whose table pass takes the limits for the capacities (devplan.hip
// dv_tables_kernel<true>), with no bound on their sum (out_total_max = 2^64 - 1 here: a unit's candidate slots are then bounded by its input,
// whatever its limit) and whose scratch follows the input alone (the token prefix is written and not used: a size plan stores no tokens).
static MSCompStatus create_decode_dev(mscomp_amd_ctx* c, MSCompFormat format, size_t n_units, uint64_t in_total_max, uint64_t out_total_max, bool sizing,
                                      uint32_t flags, mscomp_amd_plan** out)
{
	if (!out) { return MSCOMP_ARG_ERROR; }
	*out = nullptr;
	if (!c || n_units > 0x7FFFFFF0u || (flags & ~MSCOMP_AMD_DEV_LARGE_UNITS)) { return MSCOMP_ARG_ERROR; }
	if (!known_format(format)) { return MSCOMP_ARG_ERROR; }
	const uint64_t N = n_units;
	uint64_t I = 0, chunks = 0, toks = 0, cands = 0;
	if (!decode_dev_counts(format, N, in_total_max, out_total_max, sizing, I, chunks, toks, cands)) { return MSCOMP_MEM_ERROR; }   // (checked before the context is used)
	const uint64_t O = out_total_max;
	DeviceGuard g(c->device);
	if (!g.ok) { return MSCOMP_ERRNO; }
	std::unique_ptr<mscomp_amd_plan> p(new (std::nothrow) mscomp_amd_plan());
	if (!p) { return MSCOMP_MEM_ERROR; }
	p->ctx = c; p->format = format; p->decompress = true; p->sizing = sizing; p->dev = true; p->n_units = (uint32_t)N; p->run.never = N == 0; p->n_chunks = (uint32_t)chunks;
	p->in_total_max = in_total_max; p->out_total_max = sizing ? 0 : out_total_max; p->total_in = in_total_max; p->xhc_slots = (uint32_t)cands;
	p->large = (flags & MSCOMP_AMD_DEV_LARGE_UNITS) && format != MSCOMP_LZNT1;   // (LZNT1 has no optional paths: its dev plans run the host plan's kernels already)
	bool ok = reserve_tables(p.get()) && reserve_decode_scratch(c, format, N, chunks, toks, cands, !sizing);
	if (ok && p->large) { ok = reserve_dev_paths(p.get(), N, I, O, toks); }
	if (!ok) { (void)hipGetLastError(); return MSCOMP_MEM_ERROR; }
	// the one-time kernel attributes of the instances this plan launches: set now, so that no first launch happens inside a caller's capture
	if (format == MSCOMP_LZNT1) { prepare_lzd_segments(true); } else if (!sizing) { prepare_lz_copy_block(); }
	if (p->lzg_big) { prepare_lz_copy_global(true); }
	*out = p.release();
	return MSCOMP_OK;
}
MSCompStatus mscomp_amd_plan_create_decompress_dev(mscomp_amd_ctx* c, MSCompFormat format, size_t n_units, uint64_t in_total_max, uint64_t out_total_max,
                                                   mscomp_amd_plan** out)
{
	return create_decode_dev(c, format, n_units, in_total_max, out_total_max, false, 0, out);
}
MSCompStatus mscomp_amd_plan_create_decompress_dev_ex(mscomp_amd_ctx* c, MSCompFormat format, size_t n_units, uint64_t in_total_max, uint64_t out_total_max,
                                                      uint32_t flags, mscomp_amd_plan** out)
{
	return create_decode_dev(c, format, n_units, in_total_max, out_total_max, false, flags, out);
}
MSCompStatus mscomp_amd_plan_create_size_dev_ex(mscomp_amd_ctx* c, MSCompFormat format, size_t n_units, uint64_t in_total_max, uint32_t flags, mscomp_amd_plan** out)
{
	return create_decode_dev(c, format, n_units, in_total_max, ~(uint64_t)0, true, flags, out);
}
MSCompStatus mscomp_amd_plan_create_size_dev(mscomp_amd_ctx* c, MSCompFormat format, size_t n_units, uint64_t in_total_max, mscomp_amd_plan** out)
{
	return create_decode_dev(c, format, n_units, in_total_max, ~(uint64_t)0, true, 0, out);
}

// Compress plans: the compressing half of the same pipeline (tables by dv_ctables_kernel).
MSCompStatus mscomp_amd_plan_create_compress_dev(mscomp_amd_ctx* c, MSCompFormat format, size_t n_units, uint64_t in_total_max, uint64_t in_unit_max,
                                                 mscomp_amd_plan** out)
{
	if (!out) { return MSCOMP_ARG_ERROR; }
	*out = nullptr;
	if (!c || n_units > 0x7FFFFFF0u || in_unit_max == 0 || in_unit_max > 0xFFFFF000ull) { return MSCOMP_ARG_ERROR; }
	if (!known_format(format)) { return MSCOMP_ARG_ERROR; }
	DeviceGuard g(c->device);
	if (!g.ok) { return MSCOMP_ERRNO; }
	// chunks of the accepted units: each has at most ceil(U / k), and as sum ceil(L / k) <= N + floor(sum L / k), at most N + floor(I / k) in all
	// (the first term keeps a batch of 64 KiB units at one link chunk -- 448 KiB of Xpress match scratch -- per unit)
	const uint64_t N = n_units, U = in_unit_max, I = in_total_max < N * U ? in_total_max : N * U;
	const uint64_t by_unit = N * compress_chunks(format, U), by_total = N + I / compress_chunk_bytes(format), chunks = by_unit < by_total ? by_unit : by_total;
	if (chunks > 0x7FFFFFF0ull) { return MSCOMP_MEM_ERROR; }
	std::unique_ptr<mscomp_amd_plan> p(new (std::nothrow) mscomp_amd_plan());
	if (!p) { return MSCOMP_MEM_ERROR; }
	p->ctx = c; p->format = format; p->decompress = false; p->dev = true; p->n_units = (uint32_t)N; p->run.never = N == 0; p->n_chunks = (uint32_t)chunks;
	p->in_total_max = in_total_max; p->total_in = in_total_max; p->max_unit = U;   // (max_unit: the bound dv_ctables_kernel checks, and the Xpress finder as compress_launch chooses it)
	p->lznt1_sa = format == MSCOMP_LZNT1 && lznt1_sa_for(c);
	if (!reserve_tables(p.get()) || !reserve_compress_scratch(c, format, N, chunks, p->lznt1_sa)) { (void)hipGetLastError(); return MSCOMP_MEM_ERROR; }
	// the one-time kernel attributes of the instances this plan launches: set now, so that no first launch happens inside a caller's capture
	if (format == MSCOMP_LZNT1 && p->lznt1_sa) { prepare_lznt1_sa(true); }
	if (format != MSCOMP_LZNT1) { prepare_xp_match(true); }
	if (format == MSCOMP_XPRESS) { prepare_xp_lazy2(true); }
	if (format == MSCOMP_XPRESS_HUFF) { prepare_xh_fallback(); }
	*out = p.release();
	return MSCOMP_OK;
}

// The launches of one execution of a compress or decompress dev plan: mscomp_amd_plan_execute_dev runs them through plan_run, a block
// container inside its own sequence (it is that call's plan_run, or the caller's capture, that may turn them into a graph).
extern "C++" void msc::dev_launch(mscomp_amd_plan* p, const uint8_t* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len,
                                   uint8_t* d_out, const uint64_t* d_out_off, const uint64_t* d_out_cap, uint64_t* d_out_len, int32_t* d_status)
{
	mscomp_amd_ctx* c = p->ctx;
	u64* san = static_cast<u64*>(p->tables.p); uint32_t* chunk_prefix = const_cast<uint32_t*>(p->bt.chunk_prefix);
	const int f = (int)p->format; const uint32_t n = p->n_units;
	if (p->decompress) {
		{ KernelTimer t(c, "dv_tables_kernel"); launch_dev_tables(c->stream, f, n, p->in_total_max, p->out_total_max, d_in_off, d_in_len, d_out_off, d_out_cap, san, chunk_prefix, p->tok_prefix, p->reject); }
		run_dev_paths(p);
		decode_launch(p, d_in, d_out, d_out_len, d_status);
	} else {
		{ KernelTimer t(c, "dv_ctables_kernel"); launch_dev_ctables(c->stream, f, n, p->in_total_max, p->max_unit, d_in_off, d_in_len, d_out_off, d_out_cap, san, chunk_prefix, p->reject); }
		compress_launch(p, d_in, d_out, d_out_len, d_status);
	}
	// the units the table pass rejected (the kernels saw them as empty units without room)
	{ KernelTimer t(c, "dv_reject_kernel"); launch_dev_reject(c->stream, p->reject, n, d_out_len, d_status); }
}

MSCompStatus mscomp_amd_plan_execute_dev(mscomp_amd_plan* p, const uint8_t* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len,
                                         uint8_t* d_out, const uint64_t* d_out_off, const uint64_t* d_out_cap, uint64_t* d_out_len, int32_t* d_status)
{
	if (!p || !p->dev || p->sizing || p->crc) { return MSCOMP_ARG_ERROR; }
	if (p->n_units && (!d_in_off || !d_in_len || !d_out_off || !d_out_cap || !d_out_len || !d_status)) { return MSCOMP_ARG_ERROR; }
	if ((p->in_total_max && !d_in) || (p->out_total_max && !d_out)) { return MSCOMP_ARG_ERROR; }
	if (!p->decompress && p->n_units && !d_out) { return MSCOMP_ARG_ERROR; }   // (a compress plan has no output bound: an empty unit may get LZNT1's 00 00)
	if (p->n_units == 0) { return MSCOMP_OK; }
	mscomp_amd_ctx* c = p->ctx;
	DeviceGuard g(c->device);
	if (!g.ok) { return MSCOMP_ERRNO; }
	if (p->decompress) { note_modes(p); }
	p->ran = true;
	const void* args[8] = { d_in, d_in_off, d_in_len, d_out, d_out_off, d_out_cap, d_out_len, d_status };
	return plan_run(p->run, p->ctx, args, [&] { dev_launch(p, d_in, d_in_off, d_in_len, d_out, d_out_off, d_out_cap, d_out_len, d_status); });
}

MSCompStatus mscomp_amd_plan_execute_size_dev(mscomp_amd_plan* p, const uint8_t* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len,
                                              const uint64_t* d_limit, uint64_t* d_out_len, uint64_t* d_need, int32_t* d_status)
{
	if (!p || !p->dev || !p->sizing) { return MSCOMP_ARG_ERROR; }
	if (p->n_units && (!d_in_off || !d_in_len || !d_out_len || !d_need || !d_status)) { return MSCOMP_ARG_ERROR; }
	if (p->in_total_max && !d_in) { return MSCOMP_ARG_ERROR; }
	if (p->n_units == 0) { return MSCOMP_OK; }
	mscomp_amd_ctx* c = p->ctx;
	DeviceGuard g(c->device);
	if (!g.ok) { return MSCOMP_ERRNO; }
	note_modes(p);
	p->ran = true;
	const void* args[8] = { d_in, d_in_off, d_in_len, d_limit, d_out_len, d_need, d_status };
	return plan_run(p->run, p->ctx, args, [&] {
		{ KernelTimer t(c, "dv_tables_kernel"); launch_dev_stables(c->stream, (int)p->format, p->n_units, p->in_total_max, d_in_off, d_in_len, d_limit, static_cast<u64*>(p->tables.p),
		                                                          const_cast<uint32_t*>(p->bt.chunk_prefix), p->tok_prefix, p->reject); }
		run_dev_paths(p);
		size_launch(p, d_in, d_out_len, d_need, d_status);
		// rejected units; and need = length where the kernels above did not write it (LZNT1's finalize did) -- a kernel, where a host size plan
		// ends with a copy: no memcpy node in a caller's graph
		{ KernelTimer t(c, "dv_size_finish_kernel"); launch_dev_size_finish(c->stream, p->reject, p->n_units, d_out_len, d_need, d_status, p->format != MSCOMP_LZNT1); }
	});
}

// ---- CRC-32 of a batch in HBM (include/mscomp_amd.h; kernels: crc32.hip) ----
MSCompStatus mscomp_amd_plan_create_crc_dev(mscomp_amd_ctx* c, size_t n_units, uint64_t in_total_max, mscomp_amd_plan** out)
{
	if (!out) { return MSCOMP_ARG_ERROR; }
	*out = nullptr;
	if (!c || n_units > 0x7FFFFFF0u || in_total_max >= (1ull << 50)) { return MSCOMP_ARG_ERROR; }   // (distances to a unit's end stay below 2^50: crc32.hip crc_xpow)
	DeviceGuard g(c->device);
	if (!g.ok) { return MSCOMP_ERRNO; }
	std::unique_ptr<mscomp_amd_plan> p(new (std::nothrow) mscomp_amd_plan());
	if (!p) { return MSCOMP_MEM_ERROR; }
	p->ctx = c; p->dev = true; p->crc = true; p->n_units = (uint32_t)n_units; p->run.never = n_units == 0; p->in_total_max = in_total_max; p->total_in = in_total_max;
	u64* cum; u64* off;
	if (!p->tables.reserve(crc_tables_layout(cum, off, nullptr, n_units))) { (void)hipGetLastError(); return MSCOMP_MEM_ERROR; }
	*out = p.release();
	return MSCOMP_OK;
}

MSCompStatus mscomp_amd_plan_execute_crc_dev(mscomp_amd_plan* p, const uint8_t* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len,
                                             uint32_t* d_crc, int32_t* d_status)
{
	if (!p || !p->crc) { return MSCOMP_ARG_ERROR; }
	if (p->n_units && (!d_in_off || !d_in_len || !d_crc || !d_status)) { return MSCOMP_ARG_ERROR; }
	if (p->in_total_max && !d_in) { return MSCOMP_ARG_ERROR; }
	if (p->n_units == 0) { return MSCOMP_OK; }
	mscomp_amd_ctx* c = p->ctx;
	DeviceGuard g(c->device);
	if (!g.ok) { return MSCOMP_ERRNO; }
	p->ran = true;
	const void* args[8] = { d_in, d_in_off, d_in_len, d_crc, d_status };
	return plan_run(p->run, p->ctx, args, [&] {
		u64* cum; u64* off;
		crc_tables_layout(cum, off, p->tables.p, p->n_units);
		{ KernelTimer t(c, "crc_tables_kernel"); launch_crc_tables(c->stream, p->n_units, p->in_total_max, d_in_off, d_in_len, off, cum, d_status); }
		{ KernelTimer t(c, "crc_seed_kernel"); launch_crc_seeds(c->stream, p->n_units, cum, d_crc, nullptr, nullptr); }
		{ KernelTimer t(c, "crc_kernel"); launch_crc_units(c->stream, p->n_units, d_in, off, cum, d_crc, nullptr, nullptr, nullptr, c->crc_blocks); }
	});
}

MSCompStatus mscomp_amd_layout_dev(mscomp_amd_ctx* c, size_t n_units, const uint64_t* d_cap, uint64_t align, uint64_t* d_off)
{
	if (!c || !d_off || (n_units && !d_cap) || n_units > 0x7FFFFFF0u) { return MSCOMP_ARG_ERROR; }
	DeviceGuard g(c->device);
	if (!g.ok) { return MSCOMP_ERRNO; }
	launch_layout_dev(c->stream, d_cap, (uint32_t)n_units, align, d_off);
	return hipGetLastError() == hipSuccess ? MSCOMP_OK : MSCOMP_ERRNO;
}

MSCompStatus mscomp_amd_plan_layout_dev(mscomp_amd_ctx* c, MSCompFormat format, size_t n_units, const uint64_t* d_in_len, uint64_t align,
                                        uint64_t* d_out_off, uint64_t* d_out_cap)
{
	if (!c || !d_out_off || (n_units && !d_in_len) || n_units > 0x7FFFFFF0u) { return MSCOMP_ARG_ERROR; }
	if (!known_format(format)) { return MSCOMP_ARG_ERROR; }
	DeviceGuard g(c->device);
	if (!g.ok) { return MSCOMP_ERRNO; }
	launch_clayout_dev(c->stream, (int)format, d_in_len, (uint32_t)n_units, align, d_out_off, d_out_cap);
	return hipGetLastError() == hipSuccess ? MSCOMP_OK : MSCOMP_ERRNO;
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

// Compaction from device tables: one scan launch (the offsets of mscomp_amd_layout_dev) and one copy launch on a grid fixed by the CU count.
MSCompStatus mscomp_amd_compact_dev(mscomp_amd_ctx* c, size_t n_units, const uint8_t* d_src, const uint64_t* d_src_off, const uint64_t* d_len,
                                    uint64_t align, uint8_t* d_packed, uint64_t packed_cap, uint64_t* d_packed_off)
{
	if (!c || !d_packed_off || (n_units && (!d_src || !d_src_off || !d_len || !d_packed)) || n_units > 0x7FFFFFF0u) { return MSCOMP_ARG_ERROR; }
	DeviceGuard g(c->device);
	if (!g.ok) { return MSCOMP_ERRNO; }
	launch_compact_dev(c->stream, (uint32_t)n_units, d_src, d_src_off, d_len, align, d_packed, packed_cap, d_packed_off, c->cpd_blocks);
	return hipGetLastError() == hipSuccess ? MSCOMP_OK : MSCOMP_ERRNO;
}

// Stage-level test hook: per-position (len-3 capped at 45, offset) of ONE unit as found by the HIP match finder.
// h_len3/h_off: host arrays of in_len u16. max_off 0x2000 (Xpress) or 0xFFFF (Xpress+Huffman, clip to 64 KiB chunks).
MSCompStatus mscomp_amd_debug_xpress_matches(mscomp_amd_ctx* c, const uint8_t* d_in, size_t in_len, uint32_t max_off, int clip,
                                             uint16_t* h_len3, uint16_t* h_off)
{
	if (!c) { return MSCOMP_ARG_ERROR; }
	const uint64_t z = 0, len = in_len, cap = 0;
	mscomp_amd_plan* p = nullptr;
	MSCompStatus s = mscomp_amd_plan_create(c, MSCOMP_XPRESS, 1, &z, &len, &z, &cap, &p);
	if (s != MSCOMP_OK) { return s; }
	DeviceGuard g(c->device);
	uint16_t* links = static_cast<uint16_t*>(c->links.p); uint16_t* lasthead = static_cast<uint16_t*>(c->lasthead.p);
	uint16_t* mlen3 = static_cast<uint16_t*>(c->mlen3.p); uint16_t* moff = mlen3 + 1;   /* one word per position: length - 3 | offset << 16 (common.h S16) */
	launch_xp_links(c->stream, d_in, p->bt, links, lasthead);
	launch_xp_find(c->stream, d_in, p->bt, links, lasthead, mlen3, moff, max_off, clip);
	bool ok = hipStreamSynchronize(c->stream) == hipSuccess;
	std::vector<uint32_t> words(in_len + 1);
	ok = ok && hipMemcpy(words.data(), mlen3, in_len * 4, hipMemcpyDeviceToHost) == hipSuccess;
	for (size_t i = 0; ok && i < in_len; ++i) { h_len3[i] = (uint16_t)words[i]; h_off[i] = (uint16_t)(words[i] >> 16); }
	mscomp_amd_plan_destroy(p);
	return ok ? MSCOMP_OK : MSCOMP_ERRNO;
}

// Stage-level test hook: HuffmanEncoder<15,512>::CreateCodes (HuffmanEncoder.h:58-107) for n histograms of 512 counts (host arrays)
MSCompStatus mscomp_amd_debug_huff_lengths(mscomp_amd_ctx* c, const uint32_t* h_counts, size_t n, uint8_t* h_lens)
{
	if (!c || (n && (!h_counts || !h_lens)) || n > 0x100000u) { return MSCOMP_ARG_ERROR; }
	if (!n) { return MSCOMP_OK; }
	DeviceGuard g(c->device);
	if (!g.ok || !c->counts.reserve(n * 2048) || !c->lens.reserve(n * 512)) { return MSCOMP_MEM_ERROR; }
	bool ok = hipMemcpyAsync(c->counts.p, h_counts, n * 2048, hipMemcpyHostToDevice, c->stream) == hipSuccess;
	if (ok) { launch_xh_huff_debug(c->stream, static_cast<const uint32_t*>(c->counts.p), static_cast<uint8_t*>(c->lens.p), (uint32_t)n); }
	ok = ok && hipMemcpyAsync(h_lens, c->lens.p, n * 512, hipMemcpyDeviceToHost, c->stream) == hipSuccess && hipStreamSynchronize(c->stream) == hipSuccess;
	return ok ? MSCOMP_OK : MSCOMP_ERRNO;
}

// ... and HuffmanEncoder<15,512>::CreateCodesSlow (HuffmanEncoder.h:129-226) by the fallback kernel's own package-merge. Counts on the symbols
// 0..0x100 only, as a fallback chunk has them: the kernel's package pool is sized for 257 leaves, so any other histogram is an argument error.
MSCompStatus mscomp_amd_debug_huff_lengths_slow(mscomp_amd_ctx* c, const uint32_t* h_counts, size_t n, uint8_t* h_lens)
{
	if (!c || (n && (!h_counts || !h_lens)) || n > 0x100000u) { return MSCOMP_ARG_ERROR; }
	for (size_t i = 0; i < n; ++i) { for (size_t s = 0x101; s < 512; ++s) { if (h_counts[i * 512 + s]) { return MSCOMP_ARG_ERROR; } } }
	if (!n) { return MSCOMP_OK; }
	DeviceGuard g(c->device);
	if (!g.ok || !c->counts.reserve(n * 2048) || !c->lens.reserve(n * 512)) { return MSCOMP_MEM_ERROR; }
	bool ok = hipMemcpyAsync(c->counts.p, h_counts, n * 2048, hipMemcpyHostToDevice, c->stream) == hipSuccess;
	if (ok) { launch_xh_huff_slow_debug(c->stream, static_cast<const uint32_t*>(c->counts.p), static_cast<uint8_t*>(c->lens.p), (uint32_t)n); }
	ok = ok && hipMemcpyAsync(h_lens, c->lens.p, n * 512, hipMemcpyDeviceToHost, c->stream) == hipSuccess && hipStreamSynchronize(c->stream) == hipSuccess;
	return ok ? MSCOMP_OK : MSCOMP_ERRNO;
}

int mscomp_amd_debug_hooks_enabled(void) { return test_hooks_on() ? 1 : 0; }
// Test hook: which Xpress parse/emit kernel runs (0 = chosen by batch size, 1 = one wave per unit, 2 = four waves per unit).
void mscomp_amd_debug_set_xpress_emit(int mode) { if (!test_hooks_on()) { return; } set_xpress_emit_mode(mode); g_mode_epoch.fetch_add(1, std::memory_order_acq_rel); }
uint32_t mscomp_amd_debug_lzd_walked(mscomp_amd_ctx* c)
{
	if (!c) { return 0xFFFFFFFFu; }
	DeviceGuard g(c->device);
	if (!g.ok || hipStreamSynchronize(c->stream) != hipSuccess) { return 0xFFFFFFFFu; }
	return lzd_read_walked();
}

// The LZNT1 dictionary flavour is a property of a PLAN, fixed when the plan is created (the reference fixes it when the library is built,
// config.h:83-88): from its context's setting (mscomp_amd_ctx_set_lznt1_sa_dict) or, when the context has none, from the process default below.
// Changing either never touches a plan that exists, so callers that run plans concurrently keep their bytes. The one-shot entries (ms_compress,
// ms_deflate: no context argument) and the host-batch entry create their plans per call and follow the process default of that moment.
void mscomp_amd_set_lznt1_sa_dict(int on) { g_lznt1_sa.store(on ? 1 : 0, std::memory_order_relaxed); }
int  mscomp_amd_get_lznt1_sa_dict(void) { return g_lznt1_sa.load(std::memory_order_relaxed); }
MSCompStatus mscomp_amd_ctx_set_lznt1_sa_dict(mscomp_amd_ctx* c, int on)
{
	if (!c || on < -1 || on > 1) { return MSCOMP_ARG_ERROR; }
	c->lznt1_sa = on;
	return MSCOMP_OK;
}
int mscomp_amd_debug_lzg_open(mscomp_amd_ctx* c, uint64_t words, uint32_t* out)
{	// test hook: the open-word counters of the last lzglobal.hip run (`words` = the plan's word count: sum of capacity + 64 over the units taken)
	if (!c || !out || !c->lzg_words.p) { return -1; }
	DeviceGuard g(c->device);
	if (!g.ok || hipStreamSynchronize(c->stream) != hipSuccess) { return -1; }
	LzgTables t;
	lzg_words_layout(t, c->lzg_words.p, words, 0);
	const uint32_t* open = c->dbg_lzg_open ? c->dbg_lzg_open : t.open;   // (a dev plan with large units keeps them behind the words of its bound)
	return hipMemcpy(out, open, LZG_PASSES * 4, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
int mscomp_amd_debug_plan_paths(mscomp_amd_plan* p, uint32_t out[3])
{	// test hook: units on the segment walk, units on the all-CU stage, candidate slots with token scratch, as of the plan's last execution: the
	// host's counts for a host plan, the path pass's for a dev plan with large units (read back), none for any other dev plan
	if (!p || !out) { return -1; }
	DeviceGuard g(p->ctx->device);
	if (!g.ok || hipStreamSynchronize(p->ctx->stream) != hipSuccess) { return -1; }
	out[0] = p->xps_big; out[1] = p->lzg_big; out[2] = (uint32_t)(p->xhc_scr < 0xFFFFFFFFull ? p->xhc_scr : 0xFFFFFFFFull);
	if (!p->large) { return 0; }
	out[0] = out[1] = out[2] = 0;
	if (!p->ran) { return 0; }
	uint64_t scr = 0;
	if (p->xps_big && hipMemcpy(&out[0], p->paths.xps_cnt, 4, hipMemcpyDeviceToHost) != hipSuccess) { return -1; }
	if (p->lzg_big && hipMemcpy(&out[1], p->paths.lzg_cnt, 4, hipMemcpyDeviceToHost) != hipSuccess) { return -1; }
	if (p->xhc_scr && hipMemcpy(&scr, p->scr_prefix + p->n_units, 8, hipMemcpyDeviceToHost) != hipSuccess) { return -1; }
	out[2] = (uint32_t)(scr < 0xFFFFFFFFull ? scr : 0xFFFFFFFFull);
	return 0;
}
int mscomp_amd_debug_decode_modes(mscomp_amd_ctx* c, uint32_t* out, size_t cap)
{	// test hook: the per-unit path verdicts of the last decompress or size execution on c (note_modes)
	if (!c || (cap && !out)) { return -1; }
	DeviceGuard g(c->device);
	if (!g.ok || hipStreamSynchronize(c->stream) != hipSuccess) { return -1; }
	uint32_t n = c->dbg_mode_n;
	if (c->dbg_mode_cnt && hipMemcpy(&n, c->dbg_mode_cnt, 4, hipMemcpyDeviceToHost) != hipSuccess) { return -1; }   // (a dev plan with large units: the streams its last execution took)
	if (n && cap && hipMemcpy(out, c->dbg_mode, (n < cap ? n : cap) * 4, hipMemcpyDeviceToHost) != hipSuccess) { return -1; }
	return (int)n;
}
void mscomp_amd_debug_set_xpress_decoder(int mode) { if (!test_hooks_on()) { return; } g_xpd_mode.store(mode, std::memory_order_relaxed); g_mode_epoch.fetch_add(1, std::memory_order_acq_rel); }
void mscomp_amd_debug_set_finder(int mode) { if (!test_hooks_on()) { return; } g_finder_mode.store(mode, std::memory_order_relaxed); g_mode_epoch.fetch_add(1, std::memory_order_acq_rel); }
void mscomp_amd_debug_set_one_shot(int mode) { if (!test_hooks_on()) { return; } g_one_zero_copy.store(mode == 1 ? 0 : 1, std::memory_order_relaxed); }
// Test hook: which LZNT1 chunk kernel (0 = default, 1 = one wave per chunk, 2 = four waves per chunk).
void mscomp_amd_debug_set_lznt1(int mode) { if (!test_hooks_on()) { return; } set_lznt1_mode(mode); g_mode_epoch.fetch_add(1, std::memory_order_acq_rel); }
// Test hook: 1 = the order-independent form of the LZNT1 bucket sort and the Xpress chain links on every device (what a device that fails the
// lane-order self-check gets), 0 = back to one atomic per 64 positions
void mscomp_amd_debug_set_serial_atomics(int on) { if (!test_hooks_on()) { return; } set_serial_atomics(-1, on); g_mode_epoch.fetch_add(1, std::memory_order_acq_rel); }
// Test hook: at most n blocks for the LZNT1 placement (util.hip concat_slots_kernel), so that a block takes a second tile in a small batch; 0 = the device's grid
void mscomp_amd_debug_set_place_blocks(int n) { if (!test_hooks_on()) { return; } set_place_blocks(n); g_mode_epoch.fetch_add(1, std::memory_order_acq_rel); }

// Hardware self-check (see util.hip): lanes whose returning LDS atomic was NOT served in lane order, summed over
// blocks x rounds x 64 lanes x {add, exchange}; 0 on gfx950. 0xFFFFFFFF = the check could not run.
uint32_t mscomp_amd_debug_lds_lane_order(mscomp_amd_ctx* c, uint32_t seed, uint32_t blocks, uint32_t rounds, uint32_t nkeys)
{
	if (!c || nkeys == 0 || nkeys > 2048u) { return 0xFFFFFFFFu; }
	DeviceGuard g(c->device);
	if (!c->slot_size.reserve(64)) { return 0xFFFFFFFFu; }
	return run_lds_lane_order_check(c->stream, seed, blocks, rounds, nkeys, static_cast<uint32_t*>(c->slot_size.p));
}

// Hardware self-check (see util.hip): results of v_alignbyte_b32, over 256 low bytes x 16 settings of the bits above them x 4 dword pairs x
// {vector, scalar} shift operand, that differ from {hi, lo} >> 8 (operand & 3); 0 on gfx950. 0xFFFFFFFF = the check could not run.
uint32_t mscomp_amd_debug_alignbyte(mscomp_amd_ctx* c, uint32_t seed)
{
	if (!c) { return 0xFFFFFFFFu; }
	DeviceGuard g(c->device);
	if (!c->slot_size.reserve(ALIGNBYTE_CHECK_WORDS * sizeof(uint32_t))) { return 0xFFFFFFFFu; }
	return run_alignbyte_check(c->stream, seed, static_cast<uint32_t*>(c->slot_size.p));
}

// ---- drop-in one-shot path (host pointers): H2D, one-unit batch on the GPU, D2H. No CPU encoder exists here. ----
namespace {

// One context per calling host thread (the reference is reentrant: SURVEY.md 8b "Threading"), destroyed with its thread. The
// plans of recent calls are kept: a caller that compresses buffers of one size (pages, records, fixed blocks) pays the table
// upload once and gets the captured hipGraph from its second call on.
struct OneShotTls {
	mscomp_amd_ctx* ctx = nullptr;
	hipStream_t exec = nullptr, h2d = nullptr, d2h = nullptr;   // non-blocking streams: kernels, uploads, downloads
	std::vector<hipEvent_t> ev;                         // two per slice of a pipelined call
	uint64_t* h_len = nullptr; int32_t* h_st = nullptr; size_t h_cap = 0;   // pinned: per-slice results
	DevBuf d_meta;
	struct Entry { MSCompFormat format; bool decompress; uint64_t in_len, out_cap; mscomp_amd_plan* plan; uint64_t used; };
	std::vector<Entry> plans;
	uint64_t tick = 0;
	void drop()
	{
		for (auto& e : plans) { mscomp_amd_plan_destroy(e.plan); }
		plans.clear();
		if (ctx) { mscomp_amd_ctx_destroy(ctx); ctx = nullptr; }
		for (auto e : ev) { (void)hipEventDestroy(e); }
		ev.clear();
		if (h_len) { (void)hipHostFree(h_len); h_len = nullptr; h_st = nullptr; h_cap = 0; }
		d_meta.release();
		if (exec) { (void)hipStreamDestroy(exec); exec = nullptr; }
		if (h2d) { (void)hipStreamDestroy(h2d); h2d = nullptr; }
		if (d2h) { (void)hipStreamDestroy(d2h); d2h = nullptr; }
	}
	bool slices(size_t n)                               // events, pinned result slots and device result slots for n slices
	{
		while (ev.size() < 2 * n) { hipEvent_t e = nullptr; if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) { return false; } ev.push_back(e); }
		if (h_cap < n) {
			if (h_len) { (void)hipHostFree(h_len); h_len = nullptr; h_cap = 0; }
			void* q = nullptr;
			if (hipHostMalloc(&q, n * 16, hipHostMallocDefault) != hipSuccess) { return false; }
			h_len = static_cast<uint64_t*>(q); h_st = reinterpret_cast<int32_t*>(h_len + n); h_cap = n;
		}
		return d_meta.reserve(n * 16);
	}
	~OneShotTls() { drop(); }
	MSCompStatus plan_for(MSCompFormat f, bool dec, uint64_t in_len, uint64_t out_cap, mscomp_amd_plan** out)
	{
		for (auto& e : plans) {
			if (e.format == f && e.decompress == dec && e.in_len == in_len && e.out_cap == out_cap && e.plan->lznt1_sa == (!dec && f == MSCOMP_LZNT1 && lznt1_sa_for(ctx))) { e.used = ++tick; *out = e.plan; return MSCOMP_OK; }
		}
		const uint64_t z = 0;
		mscomp_amd_plan* p = nullptr;
		const MSCompStatus s = plan_create_impl(ctx, f, dec, 1, &z, &in_len, &z, &out_cap, &p);
		if (s != MSCOMP_OK) { return s; }
		p->run.never = true;
		if (plans.size() >= 8) {
			size_t lru = 0;
			for (size_t i = 1; i < plans.size(); ++i) { if (plans[i].used < plans[lru].used) { lru = i; } }
			mscomp_amd_plan_destroy(plans[lru].plan);
			plans.erase(plans.begin() + (long)lru);
		}
		plans.push_back(Entry{ f, dec, in_len, out_cap, p, ++tick });
		*out = p;
		return MSCOMP_OK;
	}
};

OneShotTls& one_shot_tls() { thread_local OneShotTls tls; return tls; }

} // namespace

// ---- the scratch hooks (include/mscomp_amd.h): fill scratch with a byte, count the slack bytes that changed ----
// the buffers a plan owns (owner 0: the plan itself, 1 / 2: the compress / decompress plan inside a block object); a dev plan rewrites all
// of them in every execution, a host plan's hold what its creation uploaded
extern "C++" void msc::scratch_of_plan(mscomp_amd_plan* p, int owner, std::vector<ScratchEnt>& v)
{
	static const char* const names[3][4] = { { "tables", "tokpre", "lzg_tab", "xps_tab" }, { "cplan.tables", "cplan.tokpre", "cplan.lzg_tab", "cplan.xps_tab" },
	                                         { "dplan.tables", "dplan.tokpre", "dplan.lzg_tab", "dplan.xps_tab" } };
	if (!p) { return; }
	DevBuf* const b[4] = { &p->tables, &p->tokpre, &p->lzg_tab, &p->xps_tab };
	for (int i = 0; i < 4; ++i) { v.push_back(ScratchEnt{ names[owner][i], b[i], !p->dev }); }
}
// the target of a hook: its context (null: none, or the hooks are off) and its buffers
static mscomp_amd_ctx* scratch_target(int kind, void* obj, std::vector<ScratchEnt>& v)
{
	if (!test_hooks_on()) { return nullptr; }
	if (kind == MSCOMP_AMD_SCRATCH_CTX) {
		mscomp_amd_ctx* c = obj ? static_cast<mscomp_amd_ctx*>(obj) : one_shot_tls().ctx;
		if (c) { v = c->scratch(); }
		return c;
	}
	if (!obj) { return nullptr; }
	if (kind == MSCOMP_AMD_SCRATCH_PLAN) { mscomp_amd_plan* p = static_cast<mscomp_amd_plan*>(obj); scratch_of_plan(p, 0, v); return p->ctx; }
	return scratch_of_object(kind, obj, v);
}
int mscomp_amd_debug_scratch_names(const char** names, int cap)
{
	if (!test_hooks_on() || (cap > 0 && !names)) { return -1; }
#define MSC_X(n) #n,
	static const char* const all[] = { MSC_CTX_BUFS(MSC_X) };      // (the list mscomp_amd_ctx::scratch() is made from)
#undef MSC_X
	const int n = (int)(sizeof all / sizeof all[0]);
	for (int i = 0; i < n && i < cap; ++i) { names[i] = all[i]; }
	return n;
}
int mscomp_amd_debug_scratch_poison(int kind, void* obj, int slack_only, int byte)
{
	std::vector<ScratchEnt> v;
	mscomp_amd_ctx* c = scratch_target(kind, obj, v);
	if (!c) { return -1; }
	if (!slack_only) { for (const ScratchEnt& e : v) { if (e.keeps) { return -1; } } }   // a host plan's tables are uploaded once: only their slack may go
	DeviceGuard g(c->device);
	if (!g.ok) { return -1; }
	int filled = 0;
	for (const ScratchEnt& e : v) {
		const size_t from = slack_only ? e.b->asked : 0;
		if (!e.b->p || from >= e.b->cap) { continue; }
		if (hipMemsetAsync(static_cast<uint8_t*>(e.b->p) + from, byte & 0xFF, e.b->cap - from, c->stream) != hipSuccess) { (void)hipGetLastError(); return -1; }
		++filled;
	}
	return filled;
}
int mscomp_amd_debug_scratch_report(int kind, void* obj, int byte, mscomp_amd_scratch_rec* recs, int cap)
{
	std::vector<ScratchEnt> v;
	mscomp_amd_ctx* c = scratch_target(kind, obj, v);
	if (!c || (cap > 0 && !recs)) { return -1; }
	DeviceGuard g(c->device);
	if (!g.ok || hipStreamSynchronize(c->stream) != hipSuccess) { return -1; }
	std::vector<uint8_t> host;
	for (int i = 0; i < (int)v.size() && i < cap; ++i) {
		const DevBuf& b = *v[(size_t)i].b;
		recs[i].name = v[(size_t)i].name; recs[i].asked = b.asked; recs[i].cap = b.cap; recs[i].changed = 0;
		if (!b.p || b.asked >= b.cap) { continue; }
		host.resize(b.cap - b.asked);
		if (hipMemcpy(host.data(), static_cast<const uint8_t*>(b.p) + b.asked, host.size(), hipMemcpyDeviceToHost) != hipSuccess) { (void)hipGetLastError(); return -1; }
		for (uint8_t x : host) { recs[i].changed += x != (uint8_t)byte; }
	}
	return (int)v.size();
}

// Page-locking of caller buffers for the large host-pointer calls. hipHostRegister refuses a range that overlaps a registered one, and a range
// one thread unregisters while another thread's copy of the same pages is in flight would pull the pages from under that copy (two threads may
// legally compress the SAME input at once: the reference only forbids aliasing in / out). So registrations go through this table: the same range
// is shared (counted), an overlapping but different range waits until the other call has released its own, and a range that cannot be registered
// at all (locked-memory limits) is simply not pinned -- the copies then go through the runtime's staging buffers.
struct HostPins {
	struct Ent { const uint8_t* b; size_t n; int refs; std::vector<std::thread::id> owners; };
	std::mutex mu; std::condition_variable cv; std::vector<Ent> ents;
	bool pin(const void* ptr, size_t n)                       // true: the range is page-locked (and mapped) until unpin
	{
		if (!ptr || !n) { return false; }
		const uint8_t* b = static_cast<const uint8_t*>(ptr);
		const std::thread::id me = std::this_thread::get_id();
		std::unique_lock<std::mutex> lk(mu);
		for (;;) {
			bool overlap = false;
			for (auto& e : ents) {
				if (e.b == b && e.n == n) { ++e.refs; e.owners.push_back(me); return true; }
				if (b < e.b + e.n && e.b < b + n) {
					// a different range that overlaps one THIS thread holds (a call whose in and out overlap): waiting would wait for ourselves --
					// the range is simply not pinned and its copies go through the runtime's staging buffers
					for (auto& o : e.owners) { if (o == me) { return false; } }
					overlap = true;
				}
			}
			if (!overlap) { break; }
			cv.wait(lk);
		}
		// (hipHostRegister of tens of megabytes takes milliseconds and runs under the table's lock: large one-shot calls of different threads
		// register one after the other; their copies and kernels still overlap)
		if (hipHostRegister(const_cast<uint8_t*>(b), n, hipHostRegisterMapped | hipHostRegisterPortable) != hipSuccess) { (void)hipGetLastError(); return false; }
		ents.push_back(Ent{ b, n, 1, { me } });
		return true;
	}
	// A call that does NOT pin its input (the staged paths) but reads a range another thread's call has registered: the runtime then copies
	// from it as from pinned memory (asynchronously), so the registration must outlive that copy. hold() takes a reference on every entry that
	// overlaps the range (the entries are returned and given back with release() once the copy is done).
	std::vector<std::pair<const uint8_t*, size_t>> hold(const void* ptr, size_t n)
	{
		std::vector<std::pair<const uint8_t*, size_t>> held;
		if (!ptr || !n) { return held; }
		const uint8_t* b = static_cast<const uint8_t*>(ptr);
		std::unique_lock<std::mutex> lk(mu);
		for (auto& e : ents) { if (b < e.b + e.n && e.b < b + n) { ++e.refs; held.push_back({ e.b, e.n }); } }
		return held;
	}
	void release(const std::vector<std::pair<const uint8_t*, size_t>>& held)
	{
		std::unique_lock<std::mutex> lk(mu);
		for (auto& h : held) {
			for (size_t i = 0; i < ents.size(); ++i) {
				if (ents[i].b == h.first && ents[i].n == h.second) {
					if (--ents[i].refs == 0) { (void)hipHostUnregister(const_cast<uint8_t*>(ents[i].b)); ents.erase(ents.begin() + (long)i); cv.notify_all(); }
					break;
				}
			}
		}
	}
	void unpin(const void* ptr, size_t n)
	{
		const uint8_t* b = static_cast<const uint8_t*>(ptr);
		const std::thread::id me = std::this_thread::get_id();
		std::unique_lock<std::mutex> lk(mu);
		for (size_t i = 0; i < ents.size(); ++i) {
			if (ents[i].b == b && ents[i].n == n) {
				for (size_t k = 0; k < ents[i].owners.size(); ++k) { if (ents[i].owners[k] == me) { ents[i].owners.erase(ents[i].owners.begin() + (long)k); break; } }
				if (--ents[i].refs == 0) { (void)hipHostUnregister(const_cast<uint8_t*>(b)); ents.erase(ents.begin() + (long)i); cv.notify_all(); }
				return;
			}
		}
	}
};
static HostPins g_pins;
} // extern "C" (the two functions below are C++: they belong to the library's other translation units)
namespace msc {
// for the other host paths of the library (hostbatch.hip): keep every registration that overlaps [ptr, ptr + n) alive until the returned
// token is given back (nullptr: nothing overlapped)
void* host_pins_hold(const void* ptr, size_t n)
{
	auto v = g_pins.hold(ptr, n);
	if (v.empty()) { return nullptr; }
	return new (std::nothrow) std::vector<std::pair<const uint8_t*, size_t>>(std::move(v));
}
void host_pins_release(void* token)
{
	if (!token) { return; }
	auto* v = static_cast<std::vector<std::pair<const uint8_t*, size_t>>*>(token);
	g_pins.release(*v);
	delete v;
}
}
extern "C" {

// one large host buffer through the GPU with the link busy in both directions while the kernels run. LZNT1 chunks
// are independent and the output is their concatenation (lznt1_compress.cpp:262), so the buffer is cut into slices of 1024 chunks:
// slice k + 1 is on its way up (stream h2d) and slice k - 1 on its way down (stream d2h) while slice k is compressed (the
// context's stream); a slice's place in the caller's output is known once the sizes of the slices before it are back (16 bytes per
// slice into pinned memory). The caller's buffers are page-locked for the duration of the call when the runtime allows it
// (hipHostRegister: uploads and downloads then really overlap; measured on the MI355X box: 85 MB both ways at once 0.92 ms pinned,
// 1.7 ms pageable); without it the copies still work.
// Slices of about 24 MiB (6 144 chunks: three rounds of the chunk kernel's 2 048 resident blocks; with 4 MiB slices the kernels ran at a
// third of their batch rate and the call took 4.9 instead of 2.7 ms), equal in size, at least two.
static const size_t ONE_RANGED_MIN = [] { const char* e = getenv("MSCOMP_AMD_ONE_RANGED_MIN_MB"); const long v = e ? atol(e) : 8; return (size_t)(v >= 1 && v <= 65536 ? v : 8) << 20; }();   // Xpress / Xpress+Huffman one-shot calls from this size on go up in ranges (one_shot)
static const uint32_t ONE_RANGE_CHUNKS = [] { const char* e = getenv("MSCOMP_AMD_ONE_RANGE_CHUNKS"); const long v = e ? atol(e) : 256; return (uint32_t)(v >= 1 && v <= 65536 ? v : 256); }();   // 64 KiB chunks per range (256 = 16 MiB; 51 MB, ms per call Xpress / Xpress+Huffman: 32: 5.22 / 5.85, 64: 4.38 / 4.99, 128: 4.04 / 4.65, 256: 3.91 / 4.55, one copy: 4.23 / 4.92)
static const size_t ONE_SLICE = [] { const char* e = getenv("MSCOMP_AMD_ONE_SLICE_MB"); const long v = e ? atol(e) : 24; return (size_t)(v >= 1 && v <= 4096 ? v : 24) << 20; }();   // (a value that is no number of MiB in 1..4096 is ignored)
static MSCompStatus lznt1_compress_pipelined(OneShotTls& tls, const uint8_t* in, size_t in_len, uint8_t* out, size_t* out_len)
{
	mscomp_amd_ctx* c = tls.ctx;
	const size_t cap = *out_len;
	const size_t ns = (in_len + ONE_SLICE / 2) / ONE_SLICE < 2 ? 2 : (in_len + ONE_SLICE / 2) / ONE_SLICE;
	const size_t SL = ((in_len + ns - 1) / ns + 4095) & ~(size_t)4095;          // bytes per slice: whole chunks
	const size_t scap = (lznt1_max_compressed_size(SL) + 2 + 15) & ~(size_t)15;
	if (!tls.slices(ns) || !c->one_in.reserve(in_len + 64) || !c->one_out.reserve(ns * scap + 64)) { return MSCOMP_MEM_ERROR; }
	uint8_t* d_in = static_cast<uint8_t*>(c->one_in.p); uint8_t* d_out = static_cast<uint8_t*>(c->one_out.p);
	uint64_t* d_len = static_cast<uint64_t*>(tls.d_meta.p); int32_t* d_st = reinterpret_cast<int32_t*>(d_len + ns);
	const size_t most = lznt1_max_compressed_size(in_len) + 2, out_span = cap < most ? cap : most;
	const bool reg_in = g_pins.pin(in, in_len);
	const bool reg_out = out_span && g_pins.pin(out, out_span);
	MSCompStatus rs = MSCOMP_OK;
	for (size_t k = 0; k < ns && rs == MSCOMP_OK; ++k) {
		const size_t o = k * SL, len = in_len - o < SL ? in_len - o : SL;
		if (hipMemcpyAsync(d_in + o, in + o, len, hipMemcpyHostToDevice, tls.h2d) != hipSuccess || hipEventRecord(tls.ev[2 * k], tls.h2d) != hipSuccess) { rs = MSCOMP_ERRNO; }
	}
	for (size_t k = 0; k < ns && rs == MSCOMP_OK; ++k) {
		const size_t o = k * SL, len = in_len - o < SL ? in_len - o : SL;
		mscomp_amd_plan* p = nullptr;
		rs = tls.plan_for(MSCOMP_LZNT1, false, len, scap, &p);
		if (rs != MSCOMP_OK) { break; }
		if (hipStreamWaitEvent(tls.exec, tls.ev[2 * k], 0) != hipSuccess) { rs = MSCOMP_ERRNO; break; }
		rs = mscomp_amd_plan_execute(p, d_in + o, d_out + k * scap, d_len + k, d_st + k);
		if (rs != MSCOMP_OK) { break; }
		if (hipMemcpyAsync(tls.h_len + k, d_len + k, 8, hipMemcpyDeviceToHost, tls.exec) != hipSuccess ||
		    hipMemcpyAsync(tls.h_st + k, d_st + k, 4, hipMemcpyDeviceToHost, tls.exec) != hipSuccess ||
		    hipEventRecord(tls.ev[2 * k + 1], tls.exec) != hipSuccess) { rs = MSCOMP_ERRNO; }
	}
	size_t total = 0;
	bool fits = true;
	for (size_t k = 0; k < ns && rs == MSCOMP_OK; ++k) {
		if (hipEventSynchronize(tls.ev[2 * k + 1]) != hipSuccess) { rs = MSCOMP_ERRNO; break; }
		if (tls.h_st[k] != MSCOMP_OK) { rs = (MSCompStatus)tls.h_st[k]; break; }
		const size_t len = (size_t)tls.h_len[k];
		if (fits && total + len <= cap) {
			if (len && hipMemcpyAsync(out + total, d_out + k * scap, len, hipMemcpyDeviceToHost, tls.d2h) != hipSuccess) { rs = MSCOMP_ERRNO; }
		} else { fits = false; }                                    // MSCOMP_BUF_ERROR (lznt1_compress.cpp:251,267): nothing behind the capacity is written
		total += len;
	}
	(void)hipStreamSynchronize(tls.h2d); (void)hipStreamSynchronize(tls.exec);
	if (hipStreamSynchronize(tls.d2h) != hipSuccess && rs == MSCOMP_OK) { rs = MSCOMP_ERRNO; }
	if (reg_in) { g_pins.unpin(in, in_len); }
	if (reg_out) { g_pins.unpin(out, out_span); }
	if (rs != MSCOMP_OK) { return rs; }
	if (!fits) { return MSCOMP_BUF_ERROR; }
	if (cap - total >= 2) { out[total] = 0; out[total + 1] = 0; }   // the uncounted End_of_buffer bytes (lznt1_compress.cpp:270)
	*out_len = total;
	return MSCOMP_OK;
}

// The same call without staging copies (51 MB: 2.28 -> 2.08 ms; MSCOMP_AMD_ONE_ZEROCOPY=0 switches it off): the caller's buffers are page-locked AND mapped, the chunk kernel
// reads its 4 KiB chunks straight from host memory over PCIe (every input byte once, 16 bytes per lane) and the placement kernel writes the
// images straight into the caller's output. One launch for the whole buffer: no slices, no copies in HBM. -100 = could not map (the caller falls
// back to the sliced path).
// (decompress = true works too, but is slower than the staged path for 51 MB: 2.26 instead of 2.01 ms -- the decoder reads its input twice and
// writes its output in 64-byte rows; not used)
static MSCompStatus lznt1_zero_copy(OneShotTls& tls, bool decompress, const uint8_t* in, size_t in_len, uint8_t* out, size_t* out_len)
{
	mscomp_amd_ctx* c = tls.ctx;
	const size_t cap = *out_len;
	const size_t most = decompress ? (in_len / 3 + 1) * 4096 : lznt1_max_compressed_size(in_len) + 2, out_span = cap < most ? cap : most;   // (what the format can produce: see one_shot)
	if (!out_span || !c->one_meta.reserve(64)) { return (MSCompStatus)-100; }
	if (!g_pins.pin(in, in_len)) { return (MSCompStatus)-100; }
	if (!g_pins.pin(out, out_span)) { g_pins.unpin(in, in_len); return (MSCompStatus)-100; }
	void* din = nullptr; void* dout = nullptr;
	MSCompStatus rs = MSCOMP_OK;
	struct { uint64_t len; int32_t st; int32_t pad; } meta = { 0, MSCOMP_ERRNO, 0 };
	if (hipHostGetDevicePointer(&din, const_cast<uint8_t*>(in), 0) != hipSuccess || hipHostGetDevicePointer(&dout, out, 0) != hipSuccess) { (void)hipGetLastError(); rs = (MSCompStatus)-100; }
	if (rs == MSCOMP_OK) {
		uint64_t* d_len = static_cast<uint64_t*>(c->one_meta.p); int32_t* d_st = reinterpret_cast<int32_t*>(d_len + 1);
		mscomp_amd_plan* p = nullptr;
		rs = tls.plan_for(MSCOMP_LZNT1, decompress, in_len, out_span, &p);
		if (rs == MSCOMP_OK) { rs = mscomp_amd_plan_execute(p, static_cast<const uint8_t*>(din), static_cast<uint8_t*>(dout), d_len, d_st); }
		if (rs == MSCOMP_OK && (hipMemcpyAsync(&meta, d_len, sizeof meta, hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess)) { rs = MSCOMP_ERRNO; }
	}
	g_pins.unpin(in, in_len); g_pins.unpin(out, out_span);
	if (rs != MSCOMP_OK) { return rs; }
	if (meta.st != MSCOMP_OK) { return (MSCompStatus)meta.st; }
	*out_len = (size_t)meta.len;
	return MSCOMP_OK;
}

static MSCompStatus one_shot(MSCompFormat format, bool decompress, const uint8_t* in, size_t in_len, uint8_t* out, size_t* out_len)
{
	if (!out_len || (in_len && !in) || (*out_len && !out)) { return MSCOMP_ARG_ERROR; }
	OneShotTls& tls = one_shot_tls();
	int dev = 0;
	if (hipGetDevice(&dev) != hipSuccess) { return MSCOMP_ERRNO; }   // no GPU / no HIP runtime: fail loudly, never fall back
	if (tls.ctx && tls.ctx->device != dev) { tls.drop(); }
	if (!tls.ctx) {
		if (hipStreamCreateWithFlags(&tls.exec, hipStreamNonBlocking) != hipSuccess || hipStreamCreateWithFlags(&tls.h2d, hipStreamNonBlocking) != hipSuccess ||
		    hipStreamCreateWithFlags(&tls.d2h, hipStreamNonBlocking) != hipSuccess) { tls.drop(); return MSCOMP_ERRNO; }
		MSCompStatus s = mscomp_amd_ctx_create(dev, tls.exec, &tls.ctx); if (s != MSCOMP_OK) { tls.drop(); return s; }
	}
	mscomp_amd_ctx* c = tls.ctx;
	DeviceGuard g(c->device);
	const size_t cap = *out_len;
	if (!decompress && format == MSCOMP_LZNT1 && in_len >= ONE_SLICE + ONE_SLICE / 2) {
		// (MSCOMP_AMD_ONE_ZEROCOPY=0 / mscomp_amd_debug_set_one_shot(1): always the sliced path below)
		if (g_one_zero_copy.load(std::memory_order_relaxed)) { const MSCompStatus z = lznt1_zero_copy(tls, false, in, in_len, out, out_len); if ((int)z != -100) { return z; } }
		return lznt1_compress_pipelined(tls, in, in_len, out, out_len);
	}
	// The device copy of the output is sized by what the format can PRODUCE, never by a generous caller capacity (legal in the
	// reference: *out_len = 1 << 40 must not become a hipMalloc of a terabyte). Compression: at most ms_max_compressed_size (+ the
	// two uncounted LZNT1 End_of_buffer bytes), and a unit that fits that bound gets the status and bytes it would get with any larger
	// capacity. LZNT1 decompression: a chunk takes at least 3 bytes and gives at most 4096. Xpress / Xpress+Huffman decompression
	// has no such bound (a 10-byte match token can stand for 4 GiB), so the device capacity starts at 16 x the input and grows only
	// when the decoder says MSCOMP_BUF_ERROR: OK and DATA_ERROR are final at any capacity, because everything the decoders of
	// xpress_decompress.cpp:405-462 / xpress_huff_decompress.cpp:39-162 test before the output runs full is independent of where it ends.
	size_t dev_cap = cap;
	if (!decompress) {
		size_t most = format == MSCOMP_LZNT1 ? lznt1_max_compressed_size(in_len) + 2 : format == MSCOMP_XPRESS ? xpress_max_compressed_size(in_len) : xpress_huff_max_compressed_size(in_len);
		if (most < dev_cap) { dev_cap = most; }
	} else if (format == MSCOMP_LZNT1) {
		const size_t most = (in_len / 3 + 1) * 4096; if (most < dev_cap) { dev_cap = most; }
	} else {
		const size_t first = in_len * 16 + (1u << 20); if (first < dev_cap) { dev_cap = first; }
	}
	if (!c->one_in.reserve(in_len + 64) || !c->one_meta.reserve(64)) { return MSCOMP_MEM_ERROR; }
	uint8_t* d_in = static_cast<uint8_t*>(c->one_in.p);
	uint64_t* d_len = static_cast<uint64_t*>(c->one_meta.p); int32_t* d_st = reinterpret_cast<int32_t*>(d_len + 1);
	// (another thread's large LZNT1 call may have page-locked this very input: keep its registration alive until our copy is through)
	struct Held { std::vector<std::pair<const uint8_t*, size_t>> v; ~Held() { if (!v.empty()) { g_pins.release(v); } } } held{ g_pins.hold(in, in_len) };
	// Xpress / Xpress+Huffman compression of ONE large buffer (round 6): the buffer goes up in ranges of ONE_RANGE_CHUNKS chunks
	// on the upload stream and the match finding of a range -- chain links and Find, the two kernels that can run on part of a unit: a chunk's links
	// and matches depend on the chunks in front of it only -- starts as soon as the range (and the 64 bytes behind it that the last positions compare
	// into) has landed, under the upload of the next one; parse / Huffman / encode (or the Xpress emit kernels) follow over the whole buffer as
	// before: one stream's flag words, and the place of an Xpress+Huffman chunk in the output, couple all chunks. A copy from pageable memory holds
	// the calling thread, not the GPU, so no page-locking is needed for the overlap.
	const bool ranged = !decompress && (format == MSCOMP_XPRESS || format == MSCOMP_XPRESS_HUFF) && in_len >= ONE_RANGED_MIN &&
	                    g_one_zero_copy.load(std::memory_order_relaxed);      // (mscomp_amd_debug_set_one_shot(1) / MSCOMP_AMD_ONE_ZEROCOPY=0: the one-copy path, for A/B runs and tests)
	if (!ranged && in_len && hipMemcpyAsync(d_in, in, in_len, hipMemcpyHostToDevice, c->stream) != hipSuccess) { return MSCOMP_ERRNO; }
	struct { uint64_t len; int32_t st; int32_t pad; } meta;
	for (bool first = true;; first = false) {
		if (!c->one_out.reserve(dev_cap + 64)) { return MSCOMP_MEM_ERROR; }
		mscomp_amd_plan* p = nullptr;
		MSCompStatus s = tls.plan_for(format, decompress, in_len, dev_cap, &p);
		if (s != MSCOMP_OK) { return s; }
		if (ranged && first) {
			const uint32_t nch = p->n_chunks, nr = (nch + ONE_RANGE_CHUNKS - 1u) / ONE_RANGE_CHUNKS;
			if (!tls.slices(nr)) { return MSCOMP_MEM_ERROR; }
			uint16_t* links = static_cast<uint16_t*>(c->links.p); uint16_t* lasthead = static_cast<uint16_t*>(c->lasthead.p);
			uint16_t* mlen3 = static_cast<uint16_t*>(c->mlen3.p); uint16_t* moff = mlen3 + 1;
			const uint32_t max_off = format == MSCOMP_XPRESS ? 0x2000u : 0xFFFFu; const int clip = format == MSCOMP_XPRESS ? 0 : 1;
			if (hipEventRecord(tls.ev[0], c->stream) != hipSuccess || hipStreamWaitEvent(tls.h2d, tls.ev[0], 0) != hipSuccess) { return MSCOMP_ERRNO; }   // (the staging buffer's last reader was on the execution stream)
			for (uint32_t r = 0; r < nr; ++r) {
				const uint32_t c0 = r * ONE_RANGE_CHUNKS, cnt = nch - c0 < ONE_RANGE_CHUNKS ? nch - c0 : ONE_RANGE_CHUNKS;
				const size_t b0 = (size_t)c0 * 65536u + (r ? 64u : 0u);
				size_t b1 = (size_t)(c0 + cnt) * 65536u + 64u; if (b1 > in_len) { b1 = in_len; }
				if (b1 > b0 && hipMemcpyAsync(d_in + b0, in + b0, b1 - b0, hipMemcpyHostToDevice, tls.h2d) != hipSuccess) { return MSCOMP_ERRNO; }
				if (hipEventRecord(tls.ev[1 + r], tls.h2d) != hipSuccess || hipStreamWaitEvent(c->stream, tls.ev[1 + r], 0) != hipSuccess) { return MSCOMP_ERRNO; }
				{ KernelTimer t(c, "xp_links_kernel"); launch_xp_links_range(c->stream, d_in, p->bt, links, lasthead, c0, cnt); }
				{ KernelTimer t(c, "xp_find_kernel"); launch_xp_find_range(c->stream, d_in, p->bt, links, lasthead, mlen3, moff, max_off, clip, c0, cnt); }
			}
			p->matches_ready = true;
		}
		s = mscomp_amd_plan_execute(p, d_in, static_cast<uint8_t*>(c->one_out.p), d_len, d_st);
		p->matches_ready = false;                            // (a cached plan: whatever happened, its next execution finds its matches itself)
		if (s != MSCOMP_OK) { return s; }
		if (hipMemcpyAsync(&meta, d_len, sizeof meta, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
		    hipStreamSynchronize(c->stream) != hipSuccess) { return MSCOMP_ERRNO; }
		if (meta.st == MSCOMP_BUF_ERROR && dev_cap < cap) {          // only the staging was too small: decode again with room
			dev_cap = dev_cap > cap / 16 ? cap : dev_cap * 16;
			continue;
		}
		break;
	}
	if (meta.st != MSCOMP_OK) { return (MSCompStatus)meta.st; }
	size_t copy = (size_t)meta.len;
	if (!decompress && format == MSCOMP_LZNT1 && cap - copy >= 2) { copy += 2; }    // the uncounted End_of_buffer bytes (lznt1_compress.cpp:270)
	if (copy && hipMemcpy(out, c->one_out.p, copy, hipMemcpyDeviceToHost) != hipSuccess) { return MSCOMP_ERRNO; }
	*out_len = (size_t)meta.len;
	return MSCOMP_OK;
}

MSCompStatus lznt1_compress(const uint8_t* in, size_t n, uint8_t* out, size_t* out_len)       { return one_shot(MSCOMP_LZNT1, false, in, n, out, out_len); }
MSCompStatus xpress_compress(const uint8_t* in, size_t n, uint8_t* out, size_t* out_len)      { return one_shot(MSCOMP_XPRESS, false, in, n, out, out_len); }
MSCompStatus xpress_huff_compress(const uint8_t* in, size_t n, uint8_t* out, size_t* out_len) { return one_shot(MSCOMP_XPRESS_HUFF, false, in, n, out, out_len); }

// the decompressors (lznt1_decompress.cpp:293 via internal.h:616-630, ...): same staging, the decoding happens on the GPU
MSCompStatus lznt1_decompress(const uint8_t* in, size_t n, uint8_t* out, size_t* out_len)       { return one_shot(MSCOMP_LZNT1, true, in, n, out, out_len); }
MSCompStatus xpress_decompress(const uint8_t* in, size_t n, uint8_t* out, size_t* out_len)      { return one_shot(MSCOMP_XPRESS, true, in, n, out, out_len); }
MSCompStatus xpress_huff_decompress(const uint8_t* in, size_t n, uint8_t* out, size_t* out_len) { return one_shot(MSCOMP_XPRESS_HUFF, true, in, n, out, out_len); }

#ifndef MSCOMP_AMD_NO_FACADE
MSCompStatus ms_decompress(MSCompFormat format, const uint8_t* in, size_t in_len, uint8_t* out, size_t* out_len)
{
	switch ((int)format) {
	case MSCOMP_LZNT1: case MSCOMP_XPRESS: case MSCOMP_XPRESS_HUFF: return one_shot(format, true, in, in_len, out, out_len);
	case MSCOMP_NONE:                                               // mscomp.cpp:26-32
		if (!out_len || in_len > *out_len) { return out_len ? MSCOMP_BUF_ERROR : MSCOMP_ARG_ERROR; }
		if (in_len) { memcpy(out, in, in_len); }
		*out_len = in_len; return MSCOMP_OK;
	default: return MSCOMP_ARG_ERROR;                                // mscomp.cpp:131
	}
}
MSCompStatus ms_compress(MSCompFormat format, const uint8_t* in, size_t in_len, uint8_t* out, size_t* out_len)
{
	switch ((int)format) {
	case MSCOMP_LZNT1: case MSCOMP_XPRESS: case MSCOMP_XPRESS_HUFF: return one_shot(format, false, in, in_len, out, out_len);
	case MSCOMP_NONE:                                               // the reference's "copy" codec (mscomp.cpp:26-32): host memcpy
		if (!out_len || in_len > *out_len) { return out_len ? MSCOMP_BUF_ERROR : MSCOMP_ARG_ERROR; }
		if (in_len) { memcpy(out, in, in_len); }
		*out_len = in_len; return MSCOMP_OK;
	default: return MSCOMP_ARG_ERROR;                                // mscomp.cpp:115
	}
}
#endif

} // extern "C"
