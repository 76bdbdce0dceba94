// host.h -- what the host files of the library share (ctx, plan, launch, plan_dev, hooks, oneshot, blockobj, hostbatch .hip): the context,
// the plan, their helpers, plan_run and what one host file takes from another; the kernel files take the switch table and the environment
// accessors from it. Internal: not installed, not part of include/. What it adds to namespace msc is not exported (hidden visibility).
#pragma once
#include "../../include/mscomp_amd.h"
#include "kernels.h"
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#pragma GCC visibility push(hidden)
namespace msc {

// The process-wide kernel switches (hooks.hip defines the object, beside the mscomp_amd_debug_set_* hooks that store into it): each picks
// between bit-identical kernels for the tests, and the launchers read theirs with a relaxed load -- any thread may call a hook while other
// threads execute plans. `epoch` is the process-wide half of a captured graph's age: a hipGraph of a plan holds raw scratch pointers and a
// kernel choice, and two counters say when it is stale: the context's own epoch (bumped whenever one of ITS device buffers moves; a context
// is used by one host thread at a time, so a plain counter) and this one, bumped by every hook that switches kernels.
struct Switches {
	std::atomic<int> finder{1};                        // 1 = default (Xpress units up to 64 KiB: the lazy finder, xpress_lazy.hip), 2 = Find for every position everywhere
	std::atomic<int> xpd{0};                           // Xpress decompression: 0 = tokens a flag word at a time + copy kernels (default; large streams by segments), 1 = xpd_kernel (a token at a time, bytes in the same wave), 2 = as 0 without the segments
	std::atomic<int> lznt1{0};                         // LZNT1 chunk kernel: 0 = default, 1 = one wave per chunk, 2 = four waves per chunk
	std::atomic<int> xpress_emit{0};                   // Xpress parse/emit: 0 = by batch size, 1 = one wave per unit, 2 / 3 = 4 / 16 waves per unit, 4 = a block per super-block
	std::atomic<int> place_cap{0};                     // at most this many blocks for the LZNT1 placement (util.hip concat_slots_kernel), 0 = the device's grid
	std::atomic<int> one_zero_copy{1};                 // large host-pointer calls: 1 = caller buffers mapped, one launch / uploads in ranges (default), 0 = slices on three streams / one copy (MSCOMP_AMD_ONE_ZEROCOPY=0)
	std::atomic<int> lznt1_sa_default{0};              // 1 = LZNT1 compresses with the suffix-array dictionary flavour (lznt1_sa.hip; the reference's MSCOMP_WITH_LZNT1_SA_DICT build) where a context says nothing (MSCOMP_AMD_LZNT1_SA_DICT)
	std::atomic<uint64_t> epoch{1};
};
extern Switches g_sw;

struct DevBuf {
	void* p = nullptr; size_t cap = 0;
	size_t asked = 0;                                  // the largest n reserve was asked for since the buffer was last empty: [asked, cap) is slack no kernel may touch (the scratch hooks)
	uint64_t* epoch = nullptr;                         // the owning context's epoch (null for plan-owned tables)
	bool reserve(size_t n)
	{
		if (n > asked) { asked = n; }
		if (n <= cap) { return true; }
		if (epoch) { ++*epoch; }
		if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
		const size_t want = n + n / 8 + 256;
		if (hipMalloc(&p, want) != hipSuccess) { p = nullptr; asked = 0; return false; }
		cap = want; return true;
	}
	void release() { if (p) { (void)hipFree(p); if (epoch) { ++*epoch; } } p = nullptr; cap = 0; asked = 0; }
};
// A buffer handed out column by column, in the order asked for. The same code run from a null base counts the bytes, so a layout is
// written down once. u64 columns first, from an 8-byte-aligned base: every one of them stays aligned (pad8 in front of one that follows a
// narrower column).
struct Carve {
	uintptr_t at;
	explicit Carve(const void* base) : at(reinterpret_cast<uintptr_t>(base)) {}
	template <class T> T* col(size_t n) { T* p = reinterpret_cast<T*>(at); at += n * sizeof(T); return p; }
	u64* q(size_t n) { return col<u64>(n); } uint32_t* w(size_t n) { return col<uint32_t>(n); } int32_t* i(size_t n) { return col<int32_t>(n); }
	uint16_t* h(size_t n) { return col<uint16_t>(n); } uint8_t* b(size_t n) { return col<uint8_t>(n); }
	void pad8() { at = (at + 7) & ~(uintptr_t)7; }         // (a u32 list in whole u64 slots)
};
inline bool known_format(MSCompFormat f) { return f == MSCOMP_LZNT1 || f == MSCOMP_XPRESS || f == MSCOMP_XPRESS_HUFF; }

// one buffer of a scratch hook's target (mscomp_amd_debug_scratch_*): `keeps` = it holds what its creation uploaded (a host plan's tables)
struct ScratchEnt { const char* name; DevBuf* b; bool keeps; };

struct ProfRec { const char* name; hipEvent_t a, b; };

// The launch sequence of one call as a hipGraph (plan_run): captured on the call's second execution, replayed while its N argument words,
// the context's scratch and the kernel switches stay where they were. Destroyed on the context's device, its stream idle.
template <size_t N> struct GraphRun {
	hipGraphExec_t exec = nullptr;
	const void* args[N] = {};
	uint64_t epoch = 0, mode = 0;                      // mscomp_amd_ctx::epoch and g_sw.epoch when `exec` was captured
	uint32_t executions = 0;
	bool never = false;                                // never replays: a call with nothing to report on; a one-shot plan (its buffer addresses change: it would be re-captured every time)
	~GraphRun() { if (exec) { (void)hipGraphExecDestroy(exec); } }
};

} // namespace msc
#pragma GCC visibility pop

struct mscomp_amd_ctx {
	int device = 0;
	uint32_t cpd_blocks = 0;                           // the fixed grid of mscomp_amd_compact_dev on this device (asked once, here: never inside a capture)
	uint32_t crc_blocks = 0;                           // ... and that of the CRC kernel (crc32.hip)
	hipStream_t stream = nullptr;
	msc::DevBuf slots, slot_size, prefix, tile_sums;   // chunk scratch (grow-only, shared by all plans of the ctx)
	msc::DevBuf lzrec;                                 // LZNT1 parse records per chunk (LZNT1_REC bytes: match tokens per window)
	msc::DevBuf links, lasthead, mlen3;                // Xpress-family match finder scratch (per 64 KiB link chunk; mlen3: one word per position, length - 3 | offset << 16)
	msc::DevBuf wtok, wmat, wfar;                      // Xpress parse records per 64-position window (token mask, match mask, far length)
	msc::DevBuf wrec, sbrec;                           // ... state / counts / prefixes per window (6 x u32), per super-block (tot 4 x u32, pre 3 x u64, seams)
	msc::DevBuf tokbits, counts, extra, lens, codes, fb_list, fbflag;   // Xpress+Huffman per-chunk scratch
	msc::DevBuf dz_cin, dz_csize, dz_unit;             // LZNT1 decompression: header offset / decoded size per chunk slot, per-unit records
	msc::DevBuf dz_scr;                                // Xpress+Huffman decompression: token scratch of the candidates of multi-chunk buffers
	msc::DevBuf dz_tok, dz_ntok, dz_xhc;               // Xpress+Huffman decompression: 32-bit tokens of every unit, token counts, candidate chunk records
	msc::DevBuf lzg_bsum, lzg_dir, lzg_words;          // tokens -> bytes of large units by all CUs (lzglobal.hip): token block sums, tile directory, a word per output byte + pass counters
	msc::DevBuf xps_buf;                               // large Xpress streams by segments: segment records | mode per stream | done per unit
	msc::DevBuf cp_tab;                                // compaction: out_off (u64) | tile_prefix (u32) of the batch being packed
	msc::DevBuf one_in, one_out, one_meta;             // staging of the host-pointer one-shot path
	void* h_tab = nullptr; size_t h_tab_cap = 0;       // pinned staging of a plan's tables: they go up stream-ordered, plan_create does not wait for the stream
	hipEvent_t h_tab_ev = nullptr; bool h_tab_busy = false;   // (a stream that shares a hardware queue with a busy one would make that wait as long as the other's kernels)
	std::vector<msc::DevBuf> table_pool;               // table buffers of destroyed plans, reused by the next plan (hipFree waits for the whole device: it would stall pipelines that create a plan per batch)
	uint64_t epoch = 1;                                // bumped when one of the buffers above moves (captured graphs are stale then)
	int lznt1_sa = -1;                                 // LZNT1 dictionary flavour of the plans this context creates: -1 = the process default at plan creation, 0 / 1 = set for this context
	const uint32_t* dbg_mode = nullptr; uint32_t dbg_mode_n = 0;   // where the last decompress / size execution left its per-unit path verdicts (mscomp_amd_debug_decode_modes)
	const uint32_t* dbg_lzg_open = nullptr;            // the open-word counters of the last execution when a dev plan with large units ran it (they lie behind the words of its BOUND)
	const uint32_t* dbg_mode_cnt = nullptr;            // ... and, for a dev plan with large units, where its path pass left their number (device memory; dbg_mode_n is then the bound)
	bool profiling = false;
	std::vector<msc::ProfRec> recs;
	std::vector<hipEvent_t> free_events;
	// every buffer above, once: bufs() and the names the scratch hooks report come from this one list
#define MSC_CTX_BUFS(X) X(slots) X(slot_size) X(prefix) X(tile_sums) X(lzrec) X(links) X(lasthead) X(mlen3) X(wtok) X(wmat) X(wfar) X(wrec) X(sbrec) \
	X(tokbits) X(counts) X(extra) X(lens) X(codes) X(fb_list) X(fbflag) X(dz_cin) X(dz_csize) X(dz_unit) X(dz_tok) X(dz_ntok) X(dz_xhc) X(dz_scr) \
	X(lzg_bsum) X(lzg_dir) X(lzg_words) X(xps_buf) X(cp_tab) X(one_in) X(one_out) X(one_meta)
	std::vector<msc::DevBuf*> bufs()
	{
#define MSC_X(n) &n,
		return { MSC_CTX_BUFS(MSC_X) };
#undef MSC_X
	}
	std::vector<msc::ScratchEnt> scratch()
	{
#define MSC_X(n) { #n, &n, false },
		return { MSC_CTX_BUFS(MSC_X) };
#undef MSC_X
	}
	mscomp_amd_ctx() { for (msc::DevBuf* b : bufs()) { b->epoch = &epoch; } }
};

struct mscomp_amd_plan {
	mscomp_amd_ctx* ctx = nullptr;
	MSCompFormat format = MSCOMP_NONE;
	bool decompress = false;
	bool sizing = false;                               // a decompressed-size plan (mscomp_amd_plan_create_size): out_cap holds the limits, nothing is decoded
	bool dev = false;                                  // a plan whose tables are built on the device at every execution (mscomp_amd_plan_create_decompress_dev / _compress_dev; with sizing: _size_dev)
	bool crc = false;                                  // a CRC plan (mscomp_amd_plan_create_crc_dev): a dev plan without a format; tables = cum (u64 x (n_units + 1)) | off (u64 x n_units)
	bool large = false;                                // ... with MSCOMP_AMD_DEV_LARGE_UNITS: the tables of the optional paths are built there too (xhc_scr, lzg_*, xps_big / xps_seg hold the bounds
	                                                   // they were reserved for, 0 = the path is off for the plan; the counts of an execution are in paths.xps_cnt / lzg_cnt, device memory)
	uint64_t in_total_max = 0, out_total_max = 0;      // ... and the bounds its scratch was reserved for
	uint32_t n_units = 0, n_chunks = 0;
	uint64_t total_in = 0, max_unit = 0;               // (max_unit of a compress dev plan: the largest unit it takes)
	bool lznt1_sa = false;                             // LZNT1: the suffix-array dictionary flavour -- fixed when the plan is created: a plan never changes its bytes under a running caller
	bool matches_ready = false;                        // the caller has run the links + find kernels of this execution itself, range by range (the pipelined one-shot call): compress_launch skips them once
	msc::DevBuf tables;                                // in_off | in_len | out_off | out_cap | chunk_prefix; dev plans: what their table pass writes (tables_layout)
	msc::DevBuf tokpre;                                // decompression by tokens (host plans): first token slot | first candidate slot | first token-scratch slot of every unit (n_units + 1 u64 each)
	uint32_t xhc_slots = 0;                            // candidate chunk slots of the batch
	uint64_t xhc_scr = 0;                              // token-scratch slots (candidates of multi-chunk buffers), 0 = none
	msc::DevBuf lzg_tab;                               // lzglobal.hip: unit (u32 x n_big, padded) | tb_prefix | tile_prefix | word_prefix (u64 x (n_big + 1) each)
	uint32_t lzg_big = 0, lzg_tb = 0, lzg_tiles = 0;   // units taken by that path (0: not used), their token blocks and tiles
	uint64_t lzg_words = 0;
	msc::DevBuf xps_tab;                               // xps_*: unit (u32 x n_big, padded) | seg_prefix (u64 x (n_big + 1))
	uint32_t xps_big = 0, xps_seg = 0, xps_seg_bytes = 0, xps_warm_bytes = 0;
	msc::DevPaths paths{};                             // the columns of xps_tab / lzg_tab and the bounds above, set when they are reserved: what a dev plan's path pass writes
	// what the launch code reads, resolved when the plan is created (the launch functions do not know where a creator put it): the columns of
	// `tables`; the prefixes, in tokpre for host plans and in `tables` for dev plans; reject (u32 x n_units), written by a dev plan's table pass
	msc::BatchTables bt{};
	msc::u64* tok_prefix = nullptr; msc::u64* cand_prefix = nullptr; msc::u64* scr_prefix = nullptr;
	uint32_t* reject = nullptr;
	msc::GraphRun<8> run;                              // the graph of the plan's execute call (a dev plan's eight pointers are the most an execute call takes)
	bool ran = false;                                  // executed at least once (mscomp_amd_debug_plan_paths: a dev plan's counts are those of its last execution)
	// (on the plan's device, its stream idle. mscomp_amd_plan_destroy hands `tables` to the context's pool first)
	~mscomp_amd_plan() { tables.release(); tokpre.release(); lzg_tab.release(); xps_tab.release(); }
};

#pragma GCC visibility push(hidden)
namespace msc {

// ---- the layouts of every plan and context buffer with more than one column ----
// One function per buffer, the only place that knows a column's offset: it fills the struct the launch code reads, from `base` on, and
// returns where the columns end. From a null base that is their byte count: what the reserve() sites ask for, plus the pad they name. Host
// code that builds a table before its upload runs the same function over its staging memory. Counts for a host plan, bounds for a dev plan.

// `tables` of a plan, writable (the launch code reads them through p->bt and the plan's prefix fields). A host plan uploads
//   in_off | in_len | out_off | out_cap (u64 x n each) | chunk_prefix (u32 x (n + 1))
// and a dev plan holds what its table pass (devplan.hip) writes each time:
//   san (4 x n u64: in_off | in_len | out_off | out_cap, zero for a rejected unit) | chunk prefix (u32, n + 1) | decompress and size plans:
//   token prefix | candidate prefix (u64, n + 1 each) | Xpress+Huffman decompress plans with large units: token-scratch prefix (u64, n + 1) |
//   reject (u32, n)
// with bt.n_chunks = the bound (the kernels that are gridded by chunks return past chunk_prefix[n_units]).
struct PlanCols { u64* in_off; u64* in_len; u64* out_off; u64* out_cap; uint32_t* chunk_prefix; u64* tok_prefix; u64* cand_prefix; u64* scr_prefix; uint32_t* reject; };
inline uintptr_t tables_layout(PlanCols& t, void* base, size_t n, bool dev, bool decompress, bool scr)
{
	Carve k(base);
	t = {};
	t.in_off = k.q(n); t.in_len = k.q(n); t.out_off = k.q(n); t.out_cap = k.q(n); t.chunk_prefix = k.w(n + 1); k.pad8();
	if (dev && decompress) { k.q(1); t.tok_prefix = k.q(n + 1); t.cand_prefix = k.q(n + 1); }   // (one slot in front of them stays unused)
	if (dev && scr) { t.scr_prefix = k.q(n + 1); }
	if (dev) { t.reject = k.w(n); k.pad8(); }
	return k.at;
}
inline uintptr_t crc_tables_layout(u64*& cum, u64*& off, void* base, size_t n) { Carve k(base); cum = k.q(n + 1); off = k.q(n); return k.at; }   // `tables` of a CRC plan
// `tokpre` of a host decode plan: `rows` of its three (one for Xpress, none for an Xpress size plan)
inline uintptr_t tokpre_layout(PlanCols& t, void* base, size_t n, int rows)
{ Carve k(base); t.tok_prefix = rows ? k.q(n + 1) : nullptr; t.cand_prefix = rows == 3 ? k.q(n + 1) : nullptr; t.scr_prefix = rows == 3 ? k.q(n + 1) : nullptr; return k.at; }
// `lzg_tab` and `xps_tab`, writable (DevPaths; the launches of the paths read them through LzgTables / XpsTables): the units taken in whole
// u64 slots, their prefixes and, for a dev plan with large units (cnt), the counts of an execution behind them
inline uintptr_t lzg_tab_layout(DevPaths& d, void* base, size_t nb, bool cnt)
{ Carve k(base); d.lzg_unit = k.w(nb); k.pad8(); d.lzg_tb_prefix = k.q(nb + 1); d.lzg_tile_prefix = k.q(nb + 1); d.lzg_word_prefix = k.q(nb + 1); d.lzg_cnt = cnt ? k.w(4) : nullptr; return k.at; }
inline uintptr_t xps_tab_layout(DevPaths& d, void* base, size_t nb, bool cnt) { Carve k(base); d.xps_unit = k.w(nb); k.pad8(); d.xps_seg_prefix = k.q(nb + 1); d.xps_cnt = cnt ? k.w(2) : nullptr; return k.at; }
// the context's scratch, as its members above say: nw windows, ns super-blocks
inline uintptr_t wrec_layout(XpressWinBufs& b, void* base, size_t nw) { Carve k(base); b.wecur = k.w(nw); b.weF = k.w(nw); b.wsum = k.w(nw); b.wnr = k.w(nw); b.ws0 = k.w(nw); b.ws1 = k.w(nw); return k.at; }
inline uintptr_t sbrec_layout(XpressWinBufs& b, void* base, size_t ns) { Carve k(base); b.sbpre = k.q(ns * 3); b.seampos = k.q(ns * 16 * 2); b.sbtot = k.w(ns * 4); b.seam = k.w(ns * 16 * 8); b.used = k.w(ns * 2); return k.at; }
// dz_unit: LZD_K speculated chains per segment, five columns | the true chain per segment, two | stop, irregular per unit (+ 1 global flag)
inline uintptr_t dz_unit_layout(LzdBufs& b, void* base, size_t n_units, size_t n_chunks)
{
	Carve k(base);
	const size_t nk = n_chunks * LZD_K;
	b.segL = k.w(nk); b.segE = k.w(nk); b.segcnt = k.w(nk); b.segstop = k.w(nk); b.segoff = k.w(nk); b.selcnt = k.w(n_chunks); b.seloff = k.w(n_chunks);
	b.stop = k.w(n_units + 1); b.irregular = k.w(n_units + 1); return k.at;
}
// dz_xhc: the records of `cands` candidate chunk slots, u64 columns first | candidate count, path verdict per unit (n_units + 1 each)
inline uintptr_t dz_xhc_layout(XhcBufs& xb, void* base, size_t n_units, size_t cands)
{
	Carve k(base);
	xb.res_prod = k.q(cands); xb.res_ntok = k.q(cands); xb.tok_off = k.q(cands); xb.cand_pos = k.w(cands); xb.res_end = k.w(cands); xb.res_reach = k.w(cands);
	xb.res_state = k.w(cands); xb.cand_cnt = k.w(n_units + 1); xb.mode = k.w(n_units + 1); return k.at;
}
inline uintptr_t xps_buf_layout(XpsTables& x, void* base, size_t n_seg, size_t nb, size_t n_units) { Carve k(base); x.seg = k.b(n_seg * XPS_SEG_BYTES); x.mode = k.w(nb); x.done = k.w(n_units); return k.at; }
inline uintptr_t lzg_dir_layout(LzgTables& g, void* base, size_t tiles) { Carve k(base); g.dir_tok = k.w(tiles); g.dir_pos = k.w(tiles); return k.at; }
inline uintptr_t lzg_words_layout(LzgTables& g, void* base, size_t words, size_t tiles) { Carve k(base); g.words = k.w(words); g.open = k.w(LZG_PASSES); g.tile_pass = k.b(tiles); return k.at; }
// fb_list: 16 counters | the chunks the fallback kernel takes (one slot per chunk, and one)
inline uintptr_t fb_list_layout(uint32_t*& count, uint32_t*& list, void* base, size_t n_chunks) { Carve k(base); count = k.w(16); list = k.w(n_chunks + 1); return k.at; }
// cp_tab of mscomp_amd_compact_batch, its tile prefix in whole u64 slots
inline uintptr_t cp_tab_layout(u64*& off, uint32_t*& tile_prefix, void* base, size_t n) { Carve k(base); off = k.q(n); tile_prefix = k.w(n + 1); k.pad8(); return k.at; }

struct DeviceGuard {
	int prev = -1; bool ok = true;
	explicit DeviceGuard(int dev) { if (hipGetDevice(&prev) != hipSuccess) { ok = false; return; } if (prev != dev) { ok = hipSetDevice(dev) == hipSuccess; } }
	~DeviceGuard() { int cur = -1; if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) { (void)hipSetDevice(prev); } }
};

inline hipEvent_t get_event(mscomp_amd_ctx* c)
{
	if (!c->free_events.empty()) { hipEvent_t e = c->free_events.back(); c->free_events.pop_back(); return e; }
	hipEvent_t e = nullptr; (void)hipEventCreate(&e); return e;
}
struct KernelTimer {
	mscomp_amd_ctx* c; ProfRec r;
	KernelTimer(mscomp_amd_ctx* ctx, const char* name) : c(ctx), r{name, nullptr, nullptr}
	{ if (c->profiling) { r.a = get_event(c); r.b = get_event(c); (void)hipEventRecord(r.a, c->stream); } }
	~KernelTimer() { if (c->profiling) { (void)hipEventRecord(r.b, c->stream); c->recs.push_back(r); } }
};

// ---- what one host file takes from another: defined in the file named, where the comments are ----
// hooks.hip: the gate of the test hooks, the environment (one accessor per MSCOMP_AMD_* variable: INTEGRATION.md 5), a plan's own buffers
#define HB_SLOTS 8                                     // sub-batches in flight per device range (hostbatch.hip), the most and the default of MSCOMP_AMD_HOST_SLOTS
bool test_hooks_on();
uint64_t env_lzg_budget(); uint64_t env_xhc_scr_budget(); bool env_no_graph(); size_t env_one_slice(); size_t env_one_ranged_min(); uint32_t env_one_range_chunks();
size_t env_host_batch_bytes(); size_t env_host_slots(); bool env_host_order(); bool env_host_trace();
uint32_t env_xps_seg(); uint32_t env_xps_warm(); uint32_t env_xps_rounds(); uint32_t env_lzb_min_bytes(); uint32_t env_lzg_hops();
void scratch_of_plan(mscomp_amd_plan* p, int owner, std::vector<ScratchEnt>& v);
// ctx.hip
bool lznt1_sa_for(const mscomp_amd_ctx* c);
uint64_t optional_scratch_budget(uint64_t env_cap, size_t already_held);
// plan.hip
bool reserve_tables(mscomp_amd_plan* p);
bool reserve_compress_scratch(mscomp_amd_ctx* c, MSCompFormat format, size_t n_units, size_t n_chunks, bool lznt1_sa);
bool reserve_decode_scratch(mscomp_amd_ctx* c, MSCompFormat format, size_t n_units, size_t n_chunks, uint64_t slots, uint64_t cands, bool store);
bool reserve_xps(mscomp_amd_plan* p, size_t nb, uint64_t sg);
bool reserve_lzg(mscomp_amd_plan* p, size_t nb, uint64_t tb, uint64_t tl, uint64_t wd);
MSCompStatus plan_create_impl(mscomp_amd_ctx* c, MSCompFormat format, bool decompress, size_t n_units, const uint64_t* in_off, const uint64_t* in_len,
                              const uint64_t* out_off, const uint64_t* out_cap, mscomp_amd_plan** out, bool sizing = false);
// launch.hip
void note_modes(mscomp_amd_plan* p);
void decode_launch(mscomp_amd_plan* p, const uint8_t* d_in, uint8_t* d_out, uint64_t* d_out_len, int32_t* d_status);
void compress_launch(mscomp_amd_plan* p, const uint8_t* d_in, uint8_t* d_out, uint64_t* d_out_len, int32_t* d_status);
void size_launch(mscomp_amd_plan* p, const uint8_t* d_in, uint64_t* d_out_len, uint64_t* d_need, int32_t* d_status);
// plan_dev.hip
bool decode_dev_counts(MSCompFormat format, uint64_t N, uint64_t in_total_max, uint64_t O, bool sizing, uint64_t& I, uint64_t& chunks, uint64_t& toks, uint64_t& cands);
void dev_launch(mscomp_amd_plan* p, const uint8_t* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len,
                uint8_t* d_out, const uint64_t* d_out_off, const uint64_t* d_out_cap, uint64_t* d_out_len, int32_t* d_status);
// oneshot.hip: the calling thread's one-shot context (null: it has made no such call); host_pins_hold / _release are below this block
mscomp_amd_ctx* one_shot_ctx();
// blockobj.hip: the buffers of a block object (kind: MSCOMP_AMD_SCRATCH_BLOCKS ..) and its context; null: no such object
mscomp_amd_ctx* scratch_of_object(int kind, void* obj, std::vector<ScratchEnt>& v);

// what opens every plan creator: *out cleared, then the context, the unit count and the format (a CRC plan has none: true)
inline bool creator_args(mscomp_amd_ctx* c, size_t n_units, bool format_ok, mscomp_amd_plan** out)
{
	if (!out) { return false; }
	*out = nullptr;
	return c && n_units <= 0x7FFFFFF0u && format_ok;
}

// One execution of a call: its launches, given as `launch`. A call that is executed repeatedly replays them as one hipGraph (the gaps between
// the 4-9 launches are ~3 % of an LZNT1 pass): captured in the call's record `r` on the second execution and again whenever a word of
// `args`, the ctx scratch or a kernel switch moved. Plain launches instead: on the first execution (one-time function attributes are set
// there), while profiling (the per-kernel events are not part of a graph), with MSCOMP_AMD_NO_GRAPH, for records that never replay, and while
// the caller captures the ctx stream (the launches then go into the caller's graph; a stream whose capture state cannot be read counts as
// captured). Only executions that may replay are counted.
extern "C++" template <class Launch, size_t N>
static MSCompStatus plan_run(GraphRun<N>& r, mscomp_amd_ctx* c, const void* const (&args)[N], const Launch& launch)
{
	hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
	if (hipStreamIsCapturing(c->stream, &cs) != hipSuccess) { (void)hipGetLastError(); cs = hipStreamCaptureStatusActive; }
	if (cs == hipStreamCaptureStatusNone && !env_no_graph() && !r.never && !c->profiling && ++r.executions >= 2) {
		const uint64_t mode_now = g_sw.epoch.load(std::memory_order_acquire);
		const bool same = r.exec && r.epoch == c->epoch && r.mode == mode_now && memcmp(r.args, args, sizeof args) == 0;
		if (!same) {
			if (r.exec) { (void)hipGraphExecDestroy(r.exec); r.exec = nullptr; }
			hipGraph_t graph = nullptr;
			if (hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal) == hipSuccess) {
				launch();
				const hipError_t ee = hipStreamEndCapture(c->stream, &graph);
				if (ee == hipSuccess && graph && hipGraphInstantiate(&r.exec, graph, nullptr, nullptr, 0) == hipSuccess) {
					r.epoch = c->epoch; r.mode = mode_now; memcpy(r.args, args, sizeof args);
				} else { r.exec = nullptr; }
				if (graph) { (void)hipGraphDestroy(graph); }
			}
			(void)hipGetLastError();
		}
		if (r.exec) { return hipGraphLaunch(r.exec, c->stream) == hipSuccess ? MSCOMP_OK : MSCOMP_ERRNO; }
	}
	launch();
	return hipGetLastError() == hipSuccess ? MSCOMP_OK : MSCOMP_ERRNO;
}

} // namespace msc
#pragma GCC visibility pop

namespace msc {
// oneshot.hip, for the other host paths (hostbatch.hip): keep every registration (page-lock) that a large one-shot call holds on caller memory
// and that overlaps [ptr, ptr + n) alive until the returned token is given back (nullptr: nothing overlapped). Dynamic symbols of the library: outside the hidden block.
void* host_pins_hold(const void* ptr, size_t n);
void host_pins_release(void* token);
}
