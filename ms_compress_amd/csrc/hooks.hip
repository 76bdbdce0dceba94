// hooks.hip -- what steers the library from outside a call: the process-wide kernel switches and the environment, and every test hook of
// include/mscomp_amd.h (mscomp_amd_debug_*), the scratch hooks among them. Host code only.
#include "host.h"
#include "envnum.h"
#include <climits>

using namespace msc;
using envnum::ranged; using envnum::is_set; using envnum::starts;

Switches msc::g_sw;

// ---- the environment (in its order): one accessor per variable, the only getenv calls of the library ----
// Each holds its variable's default, range and unit, and the moment it is read: on the accessor's first call, except where noted.
// budgets of optional scratch, in MiB: anything set counts (no digits: 0), a negative number is 0, no upper bound
static uint64_t mib_budget(const char* e, long def) { const long v = ranged(e, LONG_MIN, LONG_MAX, def); return (uint64_t)(v < 0 ? 0 : v) << 20; }
static_assert(XPS_SEG % 1024u == 0 && XPS_WARM % 1024u == 0, "the defaults of the segment walk are whole KiB");
// the process default of the LZNT1 dictionary flavour, the first value of g_sw.lznt1_sa_default: on for any value that does not begin with 0
static int env_lznt1_sa_dict() { const char* e = getenv("MSCOMP_AMD_LZNT1_SA_DICT"); return is_set(e) && !starts(e, 0) && !starts(e, '0'); }
// the all-CU byte stage: default 64 GiB of the 288; 0 switches the path off
uint64_t msc::env_lzg_budget() { static const uint64_t v = mib_budget(getenv("MSCOMP_AMD_LZG_MAX_MB"), 65536); return v; }
// the candidate token scratch: default 32 GiB; 0 = always walk twice
uint64_t msc::env_xhc_scr_budget() { static const uint64_t v = mib_budget(getenv("MSCOMP_AMD_XHC_SCR_MAX_MB"), 32768); return v; }
bool msc::env_no_graph() { static const bool v = is_set(getenv("MSCOMP_AMD_NO_GRAPH")); return v; }
// the first value of g_sw.one_zero_copy: off only for a value that begins with 0
static int env_one_zerocopy() { return !starts(getenv("MSCOMP_AMD_ONE_ZEROCOPY"), '0'); }
// the one-shot path (oneshot.hip): bytes per slice of the sliced LZNT1 call; Xpress / Xpress+Huffman calls from this size on go up in ranges; 64 KiB chunks per range
size_t msc::env_one_slice() { static const size_t v = (size_t)ranged(getenv("MSCOMP_AMD_ONE_SLICE_MB"), 1, 4096, 24) << 20; return v; }
size_t msc::env_one_ranged_min() { static const size_t v = (size_t)ranged(getenv("MSCOMP_AMD_ONE_RANGED_MIN_MB"), 1, 65536, 8) << 20; return v; }
uint32_t msc::env_one_range_chunks() { static const uint32_t v = (uint32_t)ranged(getenv("MSCOMP_AMD_ONE_RANGE_CHUNKS"), 1, 65536, 256); return v; }
// the host batches (hostbatch.hip): input bytes per sub-batch, 0 = unset (by format); sub-batches in flight; largest unit first unless the
// value begins with 0 (asked at every call); the time line on stderr
size_t msc::env_host_batch_bytes() { static const size_t v = (size_t)ranged(getenv("MSCOMP_AMD_HOST_BATCH_MB"), 1, 65536, 0) << 20; return v; }
size_t msc::env_host_slots() { static const size_t v = (size_t)ranged(getenv("MSCOMP_AMD_HOST_SLOTS"), 1, HB_SLOTS, HB_SLOTS); return v; }
bool msc::env_host_order() { return !starts(getenv("MSCOMP_AMD_HOST_ORDER"), '0'); }
bool msc::env_host_trace() { static const bool v = is_set(getenv("MSCOMP_AMD_HOST_TRACE")); return v; }
// The mscomp_amd_debug_set_* hooks pick between bit-identical kernels for the tests. They are process-wide, so the product ignores them unless the
// process asked for them BEFORE the library was loaded (MSCOMP_AMD_TEST_HOOKS=1: tests/conftest.py and the tools do): a deployment cannot have its
// kernels switched under it by a stray call.
bool msc::test_hooks_on() { static const bool v = starts(getenv("MSCOMP_AMD_TEST_HOOKS"), '1'); return v; }
// measurement knobs of the decoders. The segment walk: bytes per segment; the warm-up in front of one, capped by the segment; its rounds of
// redo -- for decompress plans only: a size plan walks XPS_ROUNDS times whatever this says (launch.hip size_launch)
uint32_t msc::env_xps_seg() { static const uint32_t v = (uint32_t)(ranged(getenv("MSCOMP_AMD_XPS_SEG_KB"), 4, 65536, XPS_SEG >> 10) << 10); return v; }
uint32_t msc::env_xps_warm() { static const uint32_t v = (uint32_t)(ranged(getenv("MSCOMP_AMD_XPS_WARM_KB"), 1, 65536, XPS_WARM >> 10) << 10); return v < env_xps_seg() ? v : env_xps_seg(); }
uint32_t msc::env_xps_rounds() { static const uint32_t v = (uint32_t)ranged(getenv("MSCOMP_AMD_XPS_ROUNDS"), 1, 256, XPS_ROUNDS); return v; }
// (both with exclusive bounds: 0 < KiB < 2^20, 0 < hops < 1000) output bytes from which a unit takes the block kernel of lz_copy.hip; hops per pointer pass of lzglobal.hip
uint32_t msc::env_lzb_min_bytes() { static const uint32_t v = (uint32_t)(ranged(getenv("MSCOMP_AMD_LZB_MIN_KB"), 1, (1 << 20) - 1, LZB_MIN_KB) << 10); return v; }
uint32_t msc::env_lzg_hops() { static const uint32_t v = (uint32_t)ranged(getenv("MSCOMP_AMD_LZG_HOPS"), 1, 999, LZG_HOPS); return v; }
// read when the library is loaded, not on first use: the two switches that start from the environment, and the sizes of the one-shot path
static const bool g_env_at_load = [] {
	g_sw.lznt1_sa_default.store(env_lznt1_sa_dict(), std::memory_order_relaxed); g_sw.one_zero_copy.store(env_one_zerocopy(), std::memory_order_relaxed);
	return env_one_ranged_min() && env_one_range_chunks() && env_one_slice();
}();

// ---- the switch hooks: one helper. A switch that changes which kernels a captured graph holds bumps the epoch ----
static void set_switch(std::atomic<int>& word, int value, bool bump = true)
{
	if (!test_hooks_on()) { return; }
	word.store(value, std::memory_order_relaxed);
	if (bump) { g_sw.epoch.fetch_add(1, std::memory_order_acq_rel); }
}

extern "C" {

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
void mscomp_amd_debug_set_xpress_emit(int mode) { set_switch(g_sw.xpress_emit, mode); }
uint32_t mscomp_amd_debug_lzd_walked(mscomp_amd_ctx* c)
{
	if (!c) { return 0xFFFFFFFFu; }
	DeviceGuard g(c->device);
	if (!g.ok || hipStreamSynchronize(c->stream) != hipSuccess) { return 0xFFFFFFFFu; }
	return lzd_read_walked();
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
void mscomp_amd_debug_set_xpress_decoder(int mode) { set_switch(g_sw.xpd, mode); }
void mscomp_amd_debug_set_finder(int mode) { set_switch(g_sw.finder, mode); }
void mscomp_amd_debug_set_one_shot(int mode) { set_switch(g_sw.one_zero_copy, mode == 1 ? 0 : 1, false); }   // (no kernel of a plan depends on it: no bump)
// Test hook: which LZNT1 chunk kernel (0 = default, 1 = one wave per chunk, 2 = four waves per chunk).
void mscomp_amd_debug_set_lznt1(int mode) { set_switch(g_sw.lznt1, mode); }
// Test hook: 1 = the order-independent form of the LZNT1 bucket sort and the Xpress chain links on every device (what a device that fails the
// lane-order self-check gets), 0 = back to one atomic per 64 positions
// (no switch of the table: util.hip keeps the hook beside the per-device verdicts it overrides)
void mscomp_amd_debug_set_serial_atomics(int on) { if (!test_hooks_on()) { return; } set_serial_atomics(-1, on); g_sw.epoch.fetch_add(1, std::memory_order_acq_rel); }
// Test hook: at most n blocks for the LZNT1 placement (util.hip concat_slots_kernel), so that a block takes a second tile in a small batch; 0 = the device's grid
void mscomp_amd_debug_set_place_blocks(int n) { set_switch(g_sw.place_cap, n > 0 ? n : 0); }

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
		mscomp_amd_ctx* c = obj ? static_cast<mscomp_amd_ctx*>(obj) : one_shot_ctx();
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

} // extern "C"
