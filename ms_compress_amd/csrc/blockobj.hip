// blockobj.hip -- the block objects of the C-ABI (include/mscomp_amd.h, mscomp_amd_search.h, mscomp_amd_match_digest.h): containers, readers, searchers, writers, splicers and dedupers. Host orchestration only, as
// plan_dev.hip: each call runs the launches of inner dev plans (dev_launch) between its own passes, through plan_run.
#include "host.h"
#include "../../include/mscomp_amd_search.h"
#include "../../include/mscomp_amd_match_digest.h"

using namespace msc;

#pragma GCC visibility push(hidden)                     // this file's helpers: not exported, as what host.h adds to namespace msc

// The checks every create starts with, on arguments alone: MSCOMP_ARG_ERROR before MSCOMP_MEM_ERROR, both before the context is used.
static bool block_size_ok(uint32_t block_size) { return block_size >= 4096u && block_size <= 524288u && !(block_size & (block_size - 1u)); }
static bool create_args_ok(const mscomp_amd_ctx* c, MSCompFormat format, uint32_t block_size, uint32_t flags) { return c && !flags && block_size_ok(block_size) && known_format(format); }
static bool count_ok(uint64_t n) { return n <= 0x7FFFFFF0u; }

// Every destroy: on the object's device, its stream idle, `release` gives up what o (may be null) holds on the device; the delete, its graphs.
template <class T, class Release> static void destroy_object(T* o, const Release& release)
{
	if (!o) { return; }
	DeviceGuard g(o->ctx->device);
	(void)hipStreamSynchronize(o->ctx->stream);
	release();
	delete o;
}

// The inner dev plans of an object that decodes or encodes blocks as units, and what they work on: dplan decodes n_d units within `total`
// bytes on either side (a container: from the caller's bytes; else into the cache), cplan encodes n_c units of at most `unit` bytes within
// `total` into the staging area. A plan without units and a buffer without bytes stay null. The object's calls run the plans' launches
// (dev_launch) between their own passes, through plan_run with a record per call, so the inner plans never capture: the graph is the
// call's, or the caller's.
struct InnerPlans {
	mscomp_amd_plan* dplan = nullptr; mscomp_amd_plan* cplan = nullptr;
	DevBuf cache, stage;
	void destroy() { mscomp_amd_plan_destroy(dplan); mscomp_amd_plan_destroy(cplan); dplan = cplan = nullptr; cache.release(); stage.release(); }
	// a call is about to run these plans' launches (mscomp_amd_debug_decode_modes, mscomp_amd_debug_plan_paths)
	void mark_ran(bool decode = true, bool encode = true)
	{
		if (decode && dplan) { note_modes(dplan); dplan->ran = true; }
		if (encode && cplan) { cplan->ran = true; }
	}
	// the object's tables (`tab`) and the buffers, then the plans; on the first failure nothing is held, `tab` neither
	MSCompStatus create(mscomp_amd_ctx* c, DevBuf& tab, uint64_t tab_bytes, uint64_t cache_bytes, uint64_t stage_bytes, uint64_t total, MSCompFormat format_d, uint64_t n_d,
	                    MSCompFormat format_c, uint64_t n_c, uint64_t unit, bool compress_first = false)
	{
		MSCompStatus st = tab.reserve(tab_bytes) && (!cache_bytes || cache.reserve(cache_bytes)) && (!stage_bytes || stage.reserve(stage_bytes)) ? MSCOMP_OK : MSCOMP_MEM_ERROR;
		for (int i = 0; i < 2 && st == MSCOMP_OK; ++i) {
			if ((i == 0) != compress_first) { if (n_d) { st = mscomp_amd_plan_create_decompress_dev(c, format_d, n_d, total, total, &dplan); } }
			else if (n_c) { st = mscomp_amd_plan_create_compress_dev(c, format_c, n_c, total, unit, &cplan); }   // (fixes the LZNT1 dictionary flavour)
		}
		if (st != MSCOMP_OK) { (void)hipGetLastError(); destroy(); tab.release(); }
		return st;
	}
};

// The views of a call, checked and packed as the kernels take them: with their checksums if they are wanted and every view has them, which
// with_crc says. False: a view with a null table, or with stored bytes at a null address.
static bool pack_views(const mscomp_amd_blocks_view* src, uint32_t n_src, bool want_crc, SpliceView* out, bool& with_crc)
{
	with_crc = want_crc;
	for (uint32_t i = 0; i < n_src; ++i) {
		const mscomp_amd_blocks_view& v = src[i];
		if (v.n_res && (!v.d_block_first || !v.d_block_off || !v.d_res_len || (v.packed_len && !v.d_packed))) { return false; }
		with_crc = with_crc && v.d_block_crc;
	}
	for (uint32_t i = 0; i < n_src; ++i) {
		const mscomp_amd_blocks_view& v = src[i];
		out[i] = { v.d_packed, v.packed_len, v.d_block_first, v.d_block_off, v.d_res_len, with_crc ? v.d_block_crc : nullptr, v.n_res, v.n_blocks_table };
	}
	return true;
}
// The graph key of a call that takes views: every field of them (the sources are read on the host and go into the kernel arguments by
// value), then the rest of its arguments.
template <size_t N, size_t R> static void view_args(const void* (&args)[N], const SpliceView* v, const void* const (&rest)[R])
{
	static_assert(N > R && (N - R) * sizeof(void*) % sizeof(SpliceView) == 0, "whole views, then the rest");
	memcpy(args, v, (N - R) * sizeof(void*)); memcpy(args + (N - R), rest, sizeof rest);
}

// The CRC-32 of n units: crc[u] over the len[u] bytes at base + off[u]; cum (n + 1) is scratch. The table pass, the seeds, the bytes.
static void crc_seeds(mscomp_amd_ctx* c, uint32_t n, u64 in_total_max, const u64* len, u64* cum, int32_t* status, uint32_t* crc, const u64* after, uint32_t* fac)
{
	{ KernelTimer k(c, "crc_tables_kernel"); launch_crc_tables(c->stream, n, in_total_max, nullptr, len, nullptr, cum, status); }
	{ KernelTimer k(c, "crc_seed_kernel"); launch_crc_seeds(c->stream, n, cum, crc, after, fac); }
}
static void crc_pass(mscomp_amd_ctx* c, uint32_t n, const uint8_t* base, const u64* off, const u64* len, u64* cum, uint32_t* crc)
{
	crc_seeds(c, n, ~(u64)0, len, cum, nullptr, crc, nullptr, nullptr);
	{ KernelTimer k(c, "crc_kernel"); launch_crc_units(c->stream, n, base, off, cum, crc, nullptr, nullptr, nullptr, c->crc_blocks); }
}

#pragma GCC visibility pop

// ---- block containers (include/mscomp_amd.h; kernels: blocks.hip) ----
// A container owns two inner dev plans over blocks as units -- compress: n_blocks_max units of at most block_size bytes; decompress: the same
// number of units within in_total_max bytes on either side --, a staging area for the compressed blocks and its own tables.
struct mscomp_amd_blocks {
	mscomp_amd_ctx* ctx = nullptr;
	MSCompFormat format = MSCOMP_NONE;
	uint32_t shift = 0, n_res = 0, n_blocks = 0;       // block_size = 1 << shift; n_blocks = n_blocks_max
	uint64_t in_total_max = 0;
	InnerPlans in;                                     // (no cache; the staged compressed blocks: in_total_max + 16 n_res bytes)
	GraphRun<8> crun; GraphRun<11> drun; GraphRun<6> krun; GraphRun<8> vrun; GraphRun<15> srun;   // compress, decompress, crc, check, salvage
	DevBuf tab;                                        // BlocksTab
	BlocksTab t{};
};

// the columns of a container's tables from `base` on (n resources, m blocks at most); returns where they end: from a null base, their bytes
static uintptr_t blocks_tab(BlocksTab& t, void* base, size_t n, size_t m)
{
	Carve k(base);
	t.res_a = k.q(n); t.res_b = k.q(n); t.unit_first = k.q(n + 1);
	t.in_off = k.q(m); t.in_len = k.q(m); t.out_off = k.q(m); t.out_cap = k.q(m); t.ulen = k.q(m); t.aux_a = k.q(m); t.aux_b = k.q(m);
	t.rstat = k.i(n); t.ustat = k.i(m); t.act = k.w(m); t.ucrc = k.w(m);
	return k.at;
}

MSCompStatus mscomp_amd_blocks_create(mscomp_amd_ctx* c, MSCompFormat format, uint32_t block_size, size_t n_res, uint64_t in_total_max, uint32_t flags,
                                      mscomp_amd_blocks** out)
{
	if (!out) { return MSCOMP_ARG_ERROR; }
	*out = nullptr;
	if (!create_args_ok(c, format, block_size, flags) || !count_ok(n_res)) { return MSCOMP_ARG_ERROR; }
	const uint64_t by_bytes = in_total_max / block_size;
	if (by_bytes > 0x7FFFFFF0ull - n_res) { return MSCOMP_MEM_ERROR; }   // (checked before the context is used; in_total_max < 2^50 from here on)
	const uint64_t M = n_res + by_bytes;
	DeviceGuard g(c->device);
	if (!g.ok) { return MSCOMP_ERRNO; }
	std::unique_ptr<mscomp_amd_blocks> b(new (std::nothrow) mscomp_amd_blocks());
	if (!b) { return MSCOMP_MEM_ERROR; }
	b->ctx = c; b->format = format; b->shift = (uint32_t)__builtin_ctz(block_size); b->n_res = (uint32_t)n_res; b->n_blocks = (uint32_t)M; b->in_total_max = in_total_max;
	b->crun.never = b->drun.never = b->krun.never = b->vrun.never = b->srun.never = n_res == 0;
	const MSCompStatus st = b->in.create(c, b->tab, blocks_tab(b->t, nullptr, n_res, M) + 64, 0, in_total_max + 16 * (uint64_t)n_res + 64, in_total_max, format, M, format, M,
	                                     block_size, true);
	if (st != MSCOMP_OK) { return st; }
	blocks_tab(b->t, b->tab.p, n_res, M);
	*out = b.release();
	return MSCOMP_OK;
}

void mscomp_amd_blocks_destroy(mscomp_amd_blocks* b) { destroy_object(b, [b] { b->in.destroy(); b->tab.release(); }); }

uint64_t mscomp_amd_blocks_bound(const mscomp_amd_blocks* b) { return b ? b->n_blocks : 0; }

MSCompStatus mscomp_amd_blocks_compress(mscomp_amd_blocks* b, const uint8_t* d_in, const uint64_t* d_res_off, const uint64_t* d_res_len,
                                        uint8_t* d_packed, uint64_t packed_cap, uint64_t* d_block_first, uint64_t* d_block_off, int32_t* d_status)
{
	if (!b || !d_block_first || !d_block_off || (b->n_res && (!d_res_off || !d_res_len || !d_status))) { return MSCOMP_ARG_ERROR; }
	if (b->in_total_max && (!d_in || !d_packed)) { return MSCOMP_ARG_ERROR; }
	mscomp_amd_ctx* c = b->ctx;
	DeviceGuard g(c->device);
	if (!g.ok) { return MSCOMP_ERRNO; }
	b->in.mark_ran(false, true);
	const void* args[8] = { d_in, d_res_off, d_res_len, d_packed, reinterpret_cast<const void*>((uintptr_t)packed_cap), d_block_first, d_block_off, d_status };
	return plan_run(b->crun, c, args, [&] {
		const BlocksTab& t = b->t;
		uint8_t* stage = static_cast<uint8_t*>(b->in.stage.p);
		{ KernelTimer k(c, "bk_ctables"); launch_blocks_ctables(c->stream, b->n_res, b->n_blocks, b->shift, b->in_total_max, d_res_off, d_res_len, d_block_first, t); }
		if (b->in.cplan) { dev_launch(b->in.cplan, d_in, t.in_off, t.in_len, stage, t.out_off, t.out_cap, t.ulen, t.ustat); }
		{ KernelTimer k(c, "bk_select_kernel"); launch_blocks_select(c->stream, b->n_res, b->n_blocks, packed_cap, d_in, stage, d_block_first, t, d_block_off, d_status); }
		{ KernelTimer k(c, "cpd_copy_kernel"); launch_pack_ptrs(c->stream, b->n_blocks, t.aux_b, t.aux_a, d_block_off, d_packed, packed_cap, c->cpd_blocks); }
	});
}

MSCompStatus mscomp_amd_blocks_decompress(mscomp_amd_blocks* b, const uint8_t* d_packed, uint64_t packed_len, const uint64_t* d_block_first,
                                          const uint64_t* d_block_off, const uint64_t* d_res_len, const uint64_t* d_range,
                                          uint8_t* d_out, const uint64_t* d_out_off, const uint64_t* d_out_cap, uint64_t* d_out_len, int32_t* d_status)
{
	if (!b || !d_block_first || !d_block_off || (b->n_res && (!d_res_len || !d_out_off || !d_out_cap || !d_out_len || !d_status))) { return MSCOMP_ARG_ERROR; }
	if (b->in_total_max && (!d_packed || !d_out)) { return MSCOMP_ARG_ERROR; }
	if (b->n_res == 0) { return MSCOMP_OK; }               // (nothing to report on)
	mscomp_amd_ctx* c = b->ctx;
	DeviceGuard g(c->device);
	if (!g.ok) { return MSCOMP_ERRNO; }
	b->in.mark_ran(true, false);
	const void* args[11] = { d_packed, reinterpret_cast<const void*>((uintptr_t)packed_len), d_block_first, d_block_off, d_res_len, d_range,
	                         d_out, d_out_off, d_out_cap, d_out_len, d_status };
	return plan_run(b->drun, c, args, [&] {
		const BlocksTab& t = b->t;
		{ KernelTimer k(c, "bk_dtables"); launch_blocks_dtables(c->stream, b->n_res, b->n_blocks, b->shift, b->in_total_max, packed_len, d_res_len, d_block_first, d_block_off,
		                                                        d_range, d_out_off, d_out_cap, nullptr, t); }
		if (b->in.dplan) { dev_launch(b->in.dplan, d_packed, t.in_off, t.in_len, d_out, t.out_off, t.out_cap, t.ulen, t.ustat); }
		{ KernelTimer k(c, "bk_rawcopy_kernel"); launch_blocks_rawcopy(c->stream, b->n_blocks, b->shift, d_packed, d_out, t, c->cpd_blocks); }
		{ KernelTimer k(c, "bk_dfold_kernel"); launch_blocks_dfold(c->stream, b->n_res, t, d_out_len, d_status); }
	});
}

// The checksums of a container: both calls are a table pass of their own, the CRC table pass and the CRC kernel over the blocks as units
// (crc32.hip), on the container's tables -- every column is a temporary of one call, so the ones compress and decompress use serve here too:
//   crc     t.unit_first = block_first, t.in_off / t.in_len = the blocks (bk_cunits_kernel), t.aux_a .. = cum (m + 1), t.act = resource of a block,
//           t.ulen = the resource's bytes behind it, t.ucrc = x^(8 times that), t.res_a .. = the running sum the resources' seeds are made with (n + 1)
//   check   t.unit_first / t.res_b = units and first block of the clipped ranges, t.in_off / t.in_len = the blocks in d_out, t.ulen = their entry
//           of d_block_crc, t.aux_a .. = cum, t.ucrc = what was read
MSCompStatus mscomp_amd_blocks_crc(mscomp_amd_blocks* b, const uint8_t* d_data, const uint64_t* d_res_off, const uint64_t* d_res_len,
                                   uint32_t* d_block_crc, uint32_t* d_res_crc, int32_t* d_status)
{
	if (!b || (b->n_blocks && !d_block_crc) || (b->n_res && (!d_res_off || !d_res_len || !d_status))) { return MSCOMP_ARG_ERROR; }
	if (b->in_total_max && !d_data) { return MSCOMP_ARG_ERROR; }
	if (b->n_res == 0) { return MSCOMP_OK; }               // (no resource, no block: n_blocks_max is 0 too)
	mscomp_amd_ctx* c = b->ctx;
	DeviceGuard g(c->device);
	if (!g.ok) { return MSCOMP_ERRNO; }
	const void* args[6] = { d_data, d_res_off, d_res_len, d_block_crc, d_res_crc, d_status };
	return plan_run(b->krun, c, args, [&] {
		const BlocksTab& t = b->t;
		{ KernelTimer k(c, "bk_ctables"); launch_blocks_ctables(c->stream, b->n_res, b->n_blocks, b->shift, b->in_total_max, d_res_off, d_res_len, t.unit_first, t); }
		{ KernelTimer k(c, "bk_crcgroups_kernel"); launch_blocks_crcgroups(c->stream, b->n_res, b->n_blocks, b->shift, d_res_len, t.unit_first, t); }
		// the resources' statuses and seeds (the check of bk_cres_kernel once more, with the seed of an empty unit for a rejected resource), then the blocks' seeds and factors
		crc_seeds(c, b->n_res, b->in_total_max, d_res_len, t.res_a, d_status, d_res_crc, nullptr, nullptr);
		crc_seeds(c, b->n_blocks, ~(u64)0, t.in_len, t.aux_a, nullptr, d_block_crc, t.ulen, d_res_crc ? t.ucrc : nullptr);
		{ KernelTimer k(c, "crc_kernel"); launch_crc_units(c->stream, b->n_blocks, d_data, t.in_off, t.aux_a, d_block_crc, t.act, t.ucrc, d_res_crc, c->crc_blocks); }
	});
}

MSCompStatus mscomp_amd_blocks_check(mscomp_amd_blocks* b, const uint8_t* d_out, const uint64_t* d_out_off, const uint64_t* d_res_len,
                                     const uint64_t* d_block_first, const uint64_t* d_range, const uint32_t* d_block_crc,
                                     uint64_t* d_out_len, int32_t* d_status)
{
	if (!b || !d_block_first || (b->n_blocks && !d_block_crc) || (b->n_res && (!d_out_off || !d_res_len || !d_out_len || !d_status))) { return MSCOMP_ARG_ERROR; }
	if (b->in_total_max && !d_out) { return MSCOMP_ARG_ERROR; }
	if (b->n_res == 0) { return MSCOMP_OK; }
	mscomp_amd_ctx* c = b->ctx;
	DeviceGuard g(c->device);
	if (!g.ok) { return MSCOMP_ERRNO; }
	const void* args[8] = { d_out, d_out_off, d_res_len, d_block_first, d_range, d_block_crc, d_out_len, d_status };
	return plan_run(b->vrun, c, args, [&] {
		const BlocksTab& t = b->t;
		{ KernelTimer k(c, "bk_ktables"); launch_blocks_ktables(c->stream, b->n_res, b->n_blocks, b->shift, b->in_total_max, d_res_len, d_block_first, d_range, d_out_off, d_status, t); }
		crc_pass(c, b->n_blocks, d_out, t.in_off, t.in_len, t.aux_a, t.ucrc);
		{ KernelTimer k(c, "bk_kfold_kernel"); launch_blocks_kfold(c->stream, b->n_res, t.ucrc, d_block_crc, 1, t, d_out_len, d_status); }
	});
}

// Salvage, the container's fifth call: decompress's passes with d_range = NULL and the mask up to the raw copy, then a verdict per row where
// decompress folds them away. The columns after the raw copy:
//   salvage t.in_off / t.in_len = the blocks in d_out the CRC kernels read, t.out_off = the unit's row, t.aux_a .. = cum, t.ucrc = what was read and
//           then the unit's verdict; t.ustat / t.ulen / t.act live from the inner plan to the verdict, t.unit_first / t.rstat / t.res_a to the fold
static_assert(SV_GOOD == MSCOMP_AMD_BLOCK_GOOD && SV_TABLE == MSCOMP_AMD_BLOCK_TABLE && SV_DECODE == MSCOMP_AMD_BLOCK_DECODE && SV_CRC == MSCOMP_AMD_BLOCK_CRC &&
              SV_SKIPPED == MSCOMP_AMD_BLOCK_SKIPPED, "the verdicts the header states");
MSCompStatus mscomp_amd_blocks_salvage(mscomp_amd_blocks* b, const uint8_t* d_packed, uint64_t packed_len, const uint64_t* d_block_first, const uint64_t* d_block_off,
                                       const uint64_t* d_res_len, const uint32_t* d_block_crc, const uint32_t* d_only, uint8_t* d_out, const uint64_t* d_out_off,
                                       const uint64_t* d_out_cap, uint64_t* d_out_len, uint32_t* d_bad, uint32_t* d_verdict, uint64_t* d_count, int32_t* d_status)
{
	if (!b || !d_block_first || !d_block_off || (b->n_res && (!d_res_len || !d_out_off || !d_out_cap || !d_out_len || !d_bad || !d_verdict || !d_count || !d_status))) { return MSCOMP_ARG_ERROR; }
	if (b->in_total_max && (!d_packed || !d_out)) { return MSCOMP_ARG_ERROR; }
	if (b->n_res == 0) { return MSCOMP_OK; }               // (nothing to report on: no resource, no row, and d_count is not written)
	mscomp_amd_ctx* c = b->ctx;
	DeviceGuard g(c->device);
	if (!g.ok) { return MSCOMP_ERRNO; }
	b->in.mark_ran(true, false);
	const void* args[15] = { d_packed, reinterpret_cast<const void*>((uintptr_t)packed_len), d_block_first, d_block_off, d_res_len, d_block_crc, d_only,
	                         d_out, d_out_off, d_out_cap, d_out_len, d_bad, d_verdict, d_count, d_status };
	return plan_run(b->srun, c, args, [&] {
		const BlocksTab& t = b->t;
		{ KernelTimer k(c, "bk_dtables"); launch_blocks_dtables(c->stream, b->n_res, b->n_blocks, b->shift, b->in_total_max, packed_len, d_res_len, d_block_first, d_block_off,
		                                                        nullptr, d_out_off, d_out_cap, d_only, t); }
		if (b->in.dplan) { dev_launch(b->in.dplan, d_packed, t.in_off, t.in_len, d_out, t.out_off, t.out_cap, t.ulen, t.ustat); }
		{ KernelTimer k(c, "bk_rawcopy_kernel"); launch_blocks_rawcopy(c->stream, b->n_blocks, b->shift, d_packed, d_out, t, c->cpd_blocks); }
		{ KernelTimer k(c, "bk_sunits_kernel"); launch_blocks_sunits(c->stream, b->n_res, b->n_blocks, b->shift, d_block_first, d_out_off, t, d_verdict, d_count); }
		if (d_block_crc) { crc_pass(c, b->n_blocks, d_out, t.in_off, t.in_len, t.aux_a, t.ucrc); }
		{ KernelTimer k(c, "bk_sverdict_kernel"); launch_blocks_sverdict(c->stream, b->n_res, b->n_blocks, d_block_crc, t, d_verdict); }
		{ KernelTimer k(c, "bk_szero_kernel"); launch_blocks_szero(c->stream, b->n_blocks, b->shift, d_out, t, c->cpd_blocks); }
		{ KernelTimer k(c, "bk_sfold_kernel"); launch_blocks_sfold(c->stream, b->n_res, t, d_out_len, d_bad, d_status, d_count); }
	});
}

// ---- block readers and writers (include/mscomp_amd.h; kernels: reader.hip, writer.hip) ----
// What a reader is and a writer starts from: one inner decompress dev plan over blocks_max units within blocks_max B bytes on either
// side, the cache those units are decoded into and its own tables. Everything is sized by what one call may touch, nothing by what the
// container holds but the 4 bytes per entry of its block table. A call runs the inner plan's launches (dev_launch) and the CRC kernels
// between its own passes, as a container does.
struct BlockAccess {
	mscomp_amd_ctx* ctx = nullptr;
	MSCompFormat format = MSCOMP_NONE;
	uint32_t shift = 0, n_res = 0, nbt = 0, n_req = 0, m = 0;   // block_size = 1 << shift; nbt = n_blocks_table; m = blocks_max
	InnerPlans in;                                     // (plans: null when blocks_max is 0; cache, a writer's staging area: blocks_max slots of block_size bytes)
	DevBuf tab;                                        // ReaderTab, a writer's extras behind it
	ReaderTab t{};
	bool ran = false;
};
struct mscomp_amd_reader : BlockAccess { GraphRun<12> run; };
// A writer adds an inner compress dev plan over the same units (a dirty block is compressed from its cache slot into its staging slot), the
// staging area and four more columns. Its call runs the reader's passes up to the fold, then its own. Its second call, resize, runs on
// the same scratch with a record of its own (write and resize keep separate graphs) and two columns per resource.
struct mscomp_amd_writer : BlockAccess {
	GraphRun<16> run; GraphRun<14> rrun;               // write, resize
	uint32_t* head = nullptr; uint32_t* next = nullptr; uint32_t* dirty = nullptr; uint64_t* addr = nullptr;   // the rest of WriterTab
	uint64_t* ru_first = nullptr; int32_t* rstat = nullptr;                          // the rest of ResizeTab
	bool resized = false;                              // the last execution was a resize (mscomp_amd_writer_counts)
};

// a's columns from `base` on, a writer's (w, else null) behind the reader's; returns where they end: from a null base, their bytes
static uintptr_t access_tab(BlockAccess* a, mscomp_amd_writer* w, void* base)
{
	const size_t n = a->n_req, m = a->m, nbt = a->nbt;
	Carve k(base);
	ReaderTab& t = a->t;
	t.q_off = k.q(n); t.q_want = k.q(n); t.q_j0 = k.q(n); t.q_len = k.q(n); t.unit_first = k.q(n + 1);
	t.in_off = k.q(m); t.in_len = k.q(m); t.out_off = k.q(m); t.out_cap = k.q(m); t.ulen = k.q(m); t.src = k.q(m); t.clen = k.q(m); t.cum = k.q(m + 1);
	if (w) { w->ru_first = k.q((size_t)a->n_res + 1); w->addr = k.q(nbt); }
	t.q_stat = k.i(n); t.ustat = k.i(m);
	t.act = k.w(m); t.owner = k.w(m); t.uq = k.w(m); t.ublk = k.w(m); t.ucrc = k.w(m);
	t.own = k.w(nbt); t.cnt = k.w(w ? 4 : 2);
	if (w) { w->next = k.w(m); w->dirty = k.w(m); w->head = k.w(nbt); w->rstat = k.i(a->n_res); }
	return k.at;
}

// Both creates, from the checks on: a is the caller's new object (null: out of memory, said where the caller would have found out), w the
// same object when it is a writer. On failure nothing is held.
static MSCompStatus access_create(BlockAccess* a, mscomp_amd_writer* w, mscomp_amd_ctx* c, MSCompFormat format, uint32_t block_size, size_t n_res,
                                  uint64_t n_blocks_table, size_t n_req, uint64_t blocks_max, uint32_t flags)
{
	if (!create_args_ok(c, format, block_size, flags) || !count_ok(n_res) || !count_ok(n_blocks_table) || !count_ok(n_req) || !count_ok(blocks_max)) { return MSCOMP_ARG_ERROR; }
	const uint64_t M = blocks_max, bytes = M * block_size;                // (< 2^50)
	uint64_t I = 0, chunks = 0, toks = 0, cands = 0;
	if (!decode_dev_counts(format, M, bytes, bytes, false, I, chunks, toks, cands)) { return MSCOMP_MEM_ERROR; }   // (what the inner plan would refuse: checked before the context is used)
	DeviceGuard g(c->device);
	if (!g.ok) { return MSCOMP_ERRNO; }
	if (!a) { return MSCOMP_MEM_ERROR; }
	a->ctx = c; a->format = format; a->shift = (uint32_t)__builtin_ctz(block_size); a->n_res = (uint32_t)n_res; a->nbt = (uint32_t)n_blocks_table;
	a->n_req = (uint32_t)n_req; a->m = (uint32_t)M;
	const uint64_t slots = M ? bytes + 64 : 0;
	const MSCompStatus st = a->in.create(c, a->tab, access_tab(a, w, nullptr) + 64, slots, w ? slots : 0, bytes, format, M, format, w ? M : 0, block_size);
	if (st == MSCOMP_OK) { access_tab(a, w, a->tab.p); }
	return st;
}
// units, distinct blocks, and the decoded (a reader) or re-encoded (a writer) blocks of a's last execution (read back; none before the first,
// none for a table a writer refused)
static int access_counts(BlockAccess* a, mscomp_amd_writer* w, uint32_t out[3])
{
	if (!a || !out) { return -1; }
	DeviceGuard g(a->ctx->device);
	if (!g.ok || hipStreamSynchronize(a->ctx->stream) != hipSuccess) { return -1; }
	out[0] = out[1] = out[2] = 0;
	if (!a->ran) { return 0; }
	uint64_t units = 0;
	uint32_t cnt[4] = {};
	const uint64_t* d_units = w && w->resized ? w->ru_first + a->n_res : a->t.unit_first + a->n_req;   // (a resize numbers its units per resource)
	if (hipMemcpy(&units, d_units, 8, hipMemcpyDeviceToHost) != hipSuccess) { return -1; }
	if (hipMemcpy(cnt, a->t.cnt, w ? 16 : 8, hipMemcpyDeviceToHost) != hipSuccess) { return -1; }
	if (!w || (cnt[3] == 0 && a->m)) { out[0] = (uint32_t)units; out[1] = cnt[0]; out[2] = cnt[w ? 2 : 1]; }   // (a resize: cnt[0] = its changed blocks, each decoded or read raw once)
	return 0;
}

// The reader's front passes, which a writer runs too. Admission: checks 1-5 per request (d_out_cap null: without the capacity rule, a
// writer's admission), then one owner per covering block and the inner plan's unit tables.
static void access_admit(BlockAccess* a, const uint8_t* d_packed, uint64_t packed_len, const uint64_t* d_block_first, const uint64_t* d_block_off,
                         const uint64_t* d_res_len, const uint64_t* d_req, const uint64_t* d_out_cap)
{
	mscomp_amd_ctx* c = a->ctx;
	{ KernelTimer k(c, "rd_req_kernel"); launch_reader_requests(c->stream, a->n_req, a->n_res, a->nbt, a->m, a->shift, d_res_len, d_block_first, d_req, d_out_cap, a->t); }
	{ KernelTimer k(c, "rd_units"); launch_reader_units(c->stream, a->n_req, a->nbt, a->m, a->shift, packed_len, d_packed, static_cast<uint8_t*>(a->in.cache.p), d_block_off, a->t); }
}
// Decode and judge: the owners' blocks decoded into the cache, checksummed (d_block_crc may be null), then status and length per request.
static void access_decode(BlockAccess* a, const uint8_t* d_packed, const uint32_t* d_block_crc, uint64_t* d_len, int32_t* d_status)
{
	mscomp_amd_ctx* c = a->ctx;
	const ReaderTab& t = a->t;
	if (a->in.dplan) { dev_launch(a->in.dplan, d_packed, t.in_off, t.in_len, static_cast<uint8_t*>(a->in.cache.p), t.out_off, t.out_cap, t.ulen, t.ustat); }
	if (d_block_crc && a->m) { crc_pass(c, a->m, nullptr, t.src, t.clen, t.cum, t.ucrc); }   // the owners' blocks lie under two bases: their addresses go in as offsets from a null one
	if (a->n_req) { KernelTimer k(c, "rd_fold_kernel"); launch_reader_fold(c->stream, a->n_req, d_block_crc, t, d_len, d_status); }
}

MSCompStatus mscomp_amd_reader_create(mscomp_amd_ctx* c, MSCompFormat format, uint32_t block_size, size_t n_res, uint64_t n_blocks_table, size_t n_req,
                                      uint64_t blocks_max, uint32_t flags, mscomp_amd_reader** out)
{
	if (!out) { return MSCOMP_ARG_ERROR; }
	*out = nullptr;
	std::unique_ptr<mscomp_amd_reader> r(new (std::nothrow) mscomp_amd_reader());
	const MSCompStatus st = access_create(r.get(), nullptr, c, format, block_size, n_res, n_blocks_table, n_req, blocks_max, flags);
	if (st == MSCOMP_OK) { r->run.never = n_req == 0; *out = r.release(); }
	return st;
}
void mscomp_amd_reader_destroy(mscomp_amd_reader* r) { destroy_object(r, [r] { r->in.destroy(); r->tab.release(); }); }

MSCompStatus mscomp_amd_reader_read(mscomp_amd_reader* r, const uint8_t* d_packed, uint64_t packed_len, const uint64_t* d_block_first,
                                    const uint64_t* d_block_off, const uint64_t* d_res_len, const uint32_t* d_block_crc, const uint64_t* d_req,
                                    uint8_t* d_out, const uint64_t* d_out_off, const uint64_t* d_out_cap, uint64_t* d_out_len, int32_t* d_status)
{
	if (!r || !d_block_first || !d_block_off || (r->n_res && !d_res_len)) { return MSCOMP_ARG_ERROR; }
	if (r->n_req && (!d_req || !d_out_off || !d_out_cap || !d_out_len || !d_status)) { return MSCOMP_ARG_ERROR; }
	if (r->m && (!d_packed || !d_out)) { return MSCOMP_ARG_ERROR; }
	if (r->n_req == 0) { return MSCOMP_OK; }               // (nothing to report on)
	mscomp_amd_ctx* c = r->ctx;
	DeviceGuard g(c->device);
	if (!g.ok) { return MSCOMP_ERRNO; }
	r->in.mark_ran(); r->ran = true;
	const void* args[12] = { d_packed, reinterpret_cast<const void*>((uintptr_t)packed_len), d_block_first, d_block_off, d_res_len, d_block_crc, d_req,
	                         d_out, d_out_off, d_out_cap, d_out_len, d_status };
	return plan_run(r->run, c, args, [&] {
		access_admit(r, d_packed, packed_len, d_block_first, d_block_off, d_res_len, d_req, d_out_cap);
		access_decode(r, d_packed, d_block_crc, d_out_len, d_status);
		{ KernelTimer k(c, "rd_gather_kernel"); launch_reader_gather(c->stream, r->n_req, r->m, r->shift, d_out, d_out_off, r->t, c->cpd_blocks); }
	});
}

int mscomp_amd_reader_counts(mscomp_amd_reader* r, uint32_t out[3]) { return access_counts(r, nullptr, out); }

// ---- block searchers (include/mscomp_amd_search.h; kernels: search.hip, the reader's passes in reader.hip) ----
// A searcher is a reader core -- the inner decompress dev plan, the cache, the reader's tables -- beside columns of its own in a
// second buffer: the pattern tables and one running-sum entry per (unit, tile) item of blocks_max units. Its call is the reader's with
// another admission in front and the scan passes in place of the gather.
static_assert(SR_PAT_MAX == MSCOMP_AMD_SEARCH_PAT_MAX && SR_LEN_MAX == MSCOMP_AMD_SEARCH_LEN_MAX, "the bounds the header states");
struct mscomp_amd_searcher : BlockAccess {
	GraphRun<14> run;
	uint32_t n_pat = 0, len_max = 0;
	uint64_t hits_max = 0;
	DevBuf cols;                                       // SearchTab
	SearchTab s{};
};
// the searcher's columns from `base` on (items: blocks_max << (shift - SR_TILE_SHIFT)); returns where they end: from a null base, their bytes
static uintptr_t search_tab(SearchTab& s, void* base, uint64_t items)
{
	Carve k(base);
	s.mask = k.q(4 * 256); s.aux = k.q(8); s.poff = k.q(SR_PAT_MAX); s.first = k.q((size_t)items + 1); s.plen = k.w(SR_PAT_MAX);
	return k.at;
}

MSCompStatus mscomp_amd_searcher_create(mscomp_amd_ctx* c, MSCompFormat format, uint32_t block_size, size_t n_res, uint64_t n_blocks_table, size_t n_req,
                                        uint64_t blocks_max, uint32_t n_pat, uint32_t len_max, uint64_t hits_max, uint32_t flags, mscomp_amd_searcher** out)
{
	if (!out) { return MSCOMP_ARG_ERROR; }
	*out = nullptr;
	if (!create_args_ok(c, format, block_size, flags) || !count_ok(n_res) || !count_ok(n_blocks_table) || !count_ok(n_req) || !count_ok(blocks_max)) { return MSCOMP_ARG_ERROR; }
	if (n_pat < 1 || n_pat > SR_PAT_MAX || len_max < 1 || len_max > SR_LEN_MAX || !count_ok(hits_max)) { return MSCOMP_ARG_ERROR; }
	std::unique_ptr<mscomp_amd_searcher> sr(new (std::nothrow) mscomp_amd_searcher());
	MSCompStatus st = access_create(sr.get(), nullptr, c, format, block_size, n_res, n_blocks_table, n_req, blocks_max, flags);
	if (st != MSCOMP_OK) { return st; }
	DeviceGuard g(c->device);
	const uint64_t items = blocks_max << (sr->shift - SR_TILE_SHIFT);      // (< 2^38)
	if (!g.ok || !sr->cols.reserve(search_tab(sr->s, nullptr, items) + 64)) {
		(void)hipGetLastError();
		sr->in.destroy(); sr->tab.release();
		return g.ok ? MSCOMP_MEM_ERROR : MSCOMP_ERRNO;
	}
	search_tab(sr->s, sr->cols.p, items);
	sr->n_pat = n_pat; sr->len_max = len_max; sr->hits_max = hits_max; sr->run.never = n_req == 0;
	*out = sr.release();
	return MSCOMP_OK;
}
void mscomp_amd_searcher_destroy(mscomp_amd_searcher* sr) { destroy_object(sr, [sr] { sr->in.destroy(); sr->tab.release(); sr->cols.release(); }); }

MSCompStatus mscomp_amd_searcher_search(mscomp_amd_searcher* sr, const uint8_t* d_packed, uint64_t packed_len, const uint64_t* d_block_first,
                                        const uint64_t* d_block_off, const uint64_t* d_res_len, const uint32_t* d_block_crc, const uint64_t* d_req,
                                        const uint8_t* d_pat, const uint64_t* d_pat_off, uint64_t* d_hits, uint64_t* d_req_hits, uint64_t* d_count,
                                        int32_t* d_pat_status, int32_t* d_status)
{
	if (!sr || !d_block_first || !d_block_off || (sr->n_res && !d_res_len)) { return MSCOMP_ARG_ERROR; }
	if (sr->n_req && (!d_req || !d_req_hits || !d_status)) { return MSCOMP_ARG_ERROR; }
	if (!d_pat || !d_pat_off || !d_count || !d_pat_status || (sr->hits_max && !d_hits) || (sr->m && !d_packed)) { return MSCOMP_ARG_ERROR; }
	if (sr->n_req == 0) { return MSCOMP_OK; }              // (nothing to report on)
	mscomp_amd_ctx* c = sr->ctx;
	DeviceGuard g(c->device);
	if (!g.ok) { return MSCOMP_ERRNO; }
	sr->in.mark_ran(); sr->ran = true;
	const void* args[14] = { d_packed, reinterpret_cast<const void*>((uintptr_t)packed_len), d_block_first, d_block_off, d_res_len, d_block_crc, d_req,
	                         d_pat, d_pat_off, d_hits, d_req_hits, d_count, d_pat_status, d_status };
	return plan_run(sr->run, c, args, [&] {
		const ReaderTab& t = sr->t;
		const SearchTab& s = sr->s;
		// the reader's passes with the searcher's admission: the look-ahead's blocks are units as any other
		{ KernelTimer k(c, "sr_req_kernel"); launch_search_requests(c->stream, sr->n_req, sr->n_res, sr->nbt, sr->m, sr->shift, sr->len_max - 1u, d_res_len, d_block_first, d_req, t); }
		{ KernelTimer k(c, "rd_units"); launch_reader_units(c->stream, sr->n_req, sr->nbt, sr->m, sr->shift, packed_len, d_packed, static_cast<uint8_t*>(sr->in.cache.p), d_block_off, t); }
		{ KernelTimer k(c, "sr_pat_kernel"); launch_search_patterns(c->stream, sr->n_pat, sr->len_max, d_pat, d_pat_off, s, d_pat_status); }
		access_decode(sr, d_packed, d_block_crc, d_req_hits, d_status);    // (the fold's lengths land in d_req_hits: the sum pass overwrites every one)
		// the searcher's own: count, sum, emit
		{ KernelTimer k(c, "sr_count_kernel"); launch_search_count(c->stream, sr->n_req, sr->m, sr->shift, sr->n_pat, sr->len_max, d_pat, s, t, c->cpd_blocks); }
		{ KernelTimer k(c, "sr_sum_kernel"); launch_search_sum(c->stream, sr->n_req, sr->shift, sr->hits_max, s, t, d_req_hits, d_count); }
		{ KernelTimer k(c, "sr_emit_kernel"); launch_search_emit(c->stream, sr->n_req, sr->m, sr->shift, sr->n_pat, sr->len_max, sr->hits_max, d_pat, s, t, d_hits, c->cpd_blocks); }
	});
}

int mscomp_amd_searcher_counts(mscomp_amd_searcher* sr, uint32_t out[3]) { return access_counts(sr, nullptr, out); }

MSCompStatus mscomp_amd_writer_create(mscomp_amd_ctx* c, MSCompFormat format, uint32_t block_size, size_t n_res, uint64_t n_blocks_table, size_t n_req,
                                      uint64_t blocks_max, uint32_t flags, mscomp_amd_writer** out)
{
	if (!out) { return MSCOMP_ARG_ERROR; }
	*out = nullptr;
	std::unique_ptr<mscomp_amd_writer> w(new (std::nothrow) mscomp_amd_writer());
	const MSCompStatus st = access_create(w.get(), w.get(), c, format, block_size, n_res, n_blocks_table, n_req, blocks_max, flags);
	if (st == MSCOMP_OK) { w->run.never = n_req == 0; w->rrun.never = n_res == 0; *out = w.release(); }
	return st;
}
void mscomp_amd_writer_destroy(mscomp_amd_writer* w) { destroy_object(w, [w] { w->in.destroy(); w->tab.release(); }); }

MSCompStatus mscomp_amd_writer_write(mscomp_amd_writer* w, const uint8_t* d_packed, uint64_t packed_len, const uint64_t* d_block_first,
                                     const uint64_t* d_block_off, const uint64_t* d_res_len, const uint32_t* d_block_crc, const uint64_t* d_req,
                                     const uint8_t* d_src, const uint64_t* d_src_off, uint8_t* d_new_packed, uint64_t new_cap, uint64_t* d_new_block_off,
                                     uint32_t* d_new_block_crc, uint64_t* d_written, int32_t* d_status, int32_t* d_res_status)
{
	if (!w || !d_block_first || !d_block_off || !d_new_block_off || (w->n_res && (!d_res_len || !d_res_status))) { return MSCOMP_ARG_ERROR; }
	if (w->n_req && (!d_req || !d_src_off || !d_written || !d_status)) { return MSCOMP_ARG_ERROR; }
	if ((w->m && !d_src) || ((w->m || w->nbt) && (!d_packed || !d_new_packed))) { return MSCOMP_ARG_ERROR; }
	if ((d_block_crc == nullptr) != (d_new_block_crc == nullptr)) { return MSCOMP_ARG_ERROR; }
	mscomp_amd_ctx* c = w->ctx;
	DeviceGuard g(c->device);
	if (!g.ok) { return MSCOMP_ERRNO; }
	w->in.mark_ran(); w->ran = true; w->resized = false;
	const void* args[16] = { d_packed, reinterpret_cast<const void*>((uintptr_t)packed_len), d_block_first, d_block_off, d_res_len, d_block_crc, d_req,
	                         d_src, d_src_off, d_new_packed, reinterpret_cast<const void*>((uintptr_t)new_cap), d_new_block_off, d_new_block_crc,
	                         d_written, d_status, d_res_status };
	return plan_run(w->run, c, args, [&] {
		const ReaderTab& t = w->t;
		const WriterTab wt = { t, w->head, w->next, w->dirty, w->addr };
		uint8_t* cache = static_cast<uint8_t*>(w->in.cache.p); uint8_t* stage = static_cast<uint8_t*>(w->in.stage.p);
		// the reader's passes: admission (without its capacity rule), owners, the owners' blocks decoded, checksummed and judged
		access_admit(w, d_packed, packed_len, d_block_first, d_block_off, d_res_len, d_req, nullptr);
		{ KernelTimer k(c, "wr_link"); launch_writer_link(c->stream, w->n_req, w->nbt, w->m, wt); }
		access_decode(w, d_packed, d_block_crc, d_written, d_status);
		// the writer's own: patch, re-encode and checksum the dirty blocks, lay out, move
		{ KernelTimer k(c, "wr_patch"); launch_writer_patch(c->stream, w->n_req, w->m, w->shift, d_src, d_src_off, cache, wt, c->cpd_blocks); }
		if (w->in.cplan) { dev_launch(w->in.cplan, cache, t.in_off, t.in_len, stage, t.out_off, t.out_cap, t.ulen, t.ustat); }
		if (d_block_crc && w->m) { crc_pass(c, w->m, nullptr, t.src, t.clen, t.cum, t.ucrc); }
		{ KernelTimer k(c, "wr_layout_kernel"); launch_writer_layout(c->stream, w->n_req, w->n_res, w->nbt, w->m, w->shift, packed_len, new_cap, d_packed, stage, cache, d_block_first,
		                                                             d_block_off, d_block_crc, wt, d_new_block_off, d_new_block_crc, d_written, d_status, d_res_status); }
		{ KernelTimer k(c, "bk_move_kernel"); launch_blocks_move(c->stream, w->nbt, new_cap, d_new_block_off, w->addr, d_new_packed, c->cpd_blocks); }
	});
}

int mscomp_amd_writer_counts(mscomp_amd_writer* w, uint32_t out[3]) { return access_counts(w, w, out); }

// The writer's second call. Per resource: rules 0-3 and the units (the changed block, the fresh blocks); the changed blocks decoded into
// their cache slots, checksummed and judged (rule 4); the units' new data trimmed and zero-filled in the cache; the compress plan and the CRC
// kernels over them; the layout over the NEW table rows (rule 8); the move.
MSCompStatus mscomp_amd_writer_resize(mscomp_amd_writer* w, const uint8_t* d_packed, uint64_t packed_len, const uint64_t* d_block_first,
                                      const uint64_t* d_block_off, const uint64_t* d_res_len, const uint32_t* d_block_crc, const uint64_t* d_want_len,
                                      uint8_t* d_new_packed, uint64_t new_cap, uint64_t* d_new_block_first, uint64_t* d_new_block_off,
                                      uint32_t* d_new_block_crc, uint64_t* d_new_res_len, int32_t* d_res_status)
{
	if (!w || !d_block_first || !d_block_off || !d_new_block_first || !d_new_block_off) { return MSCOMP_ARG_ERROR; }
	if (w->n_res && (!d_res_len || !d_want_len || !d_new_res_len || !d_res_status)) { return MSCOMP_ARG_ERROR; }
	if ((w->m || w->nbt) && (!d_packed || !d_new_packed)) { return MSCOMP_ARG_ERROR; }
	if ((d_block_crc == nullptr) != (d_new_block_crc == nullptr)) { return MSCOMP_ARG_ERROR; }
	mscomp_amd_ctx* c = w->ctx;
	DeviceGuard g(c->device);
	if (!g.ok) { return MSCOMP_ERRNO; }
	w->in.mark_ran(); w->ran = true; w->resized = true;
	const void* args[14] = { d_packed, reinterpret_cast<const void*>((uintptr_t)packed_len), d_block_first, d_block_off, d_res_len, d_block_crc, d_want_len,
	                         d_new_packed, reinterpret_cast<const void*>((uintptr_t)new_cap), d_new_block_first, d_new_block_off, d_new_block_crc,
	                         d_new_res_len, d_res_status };
	return plan_run(w->rrun, c, args, [&] {
		const ReaderTab& t = w->t;
		const ResizeTab rt = { { t, w->head, w->next, w->dirty, w->addr }, w->ru_first, w->rstat };
		uint8_t* cache = static_cast<uint8_t*>(w->in.cache.p); uint8_t* stage = static_cast<uint8_t*>(w->in.stage.p);
		{ KernelTimer k(c, "rs_units"); launch_resize_units(c->stream, w->n_res, w->nbt, w->m, w->shift, packed_len, d_packed, cache, d_block_first, d_block_off,
		                                                    d_res_len, d_want_len, rt); }
		if (w->in.dplan) { dev_launch(w->in.dplan, d_packed, t.in_off, t.in_len, cache, t.out_off, t.out_cap, t.ulen, t.ustat); }
		if (d_block_crc && w->m) { crc_pass(c, w->m, nullptr, t.src, t.clen, t.cum, t.ucrc); }
		{ KernelTimer k(c, "rs_fold_kernel"); launch_resize_fold(c->stream, w->n_res, w->m, w->shift, d_block_first, d_res_len, d_want_len, d_block_crc, rt); }
		{ KernelTimer k(c, "rs_fill"); launch_resize_fill(c->stream, w->n_res, w->m, w->shift, cache, rt, c->cpd_blocks); }
		if (w->in.cplan) { dev_launch(w->in.cplan, cache, t.in_off, t.in_len, stage, t.out_off, t.out_cap, t.ulen, t.ustat); }
		if (d_block_crc && w->m) { crc_pass(c, w->m, nullptr, t.src, t.clen, t.cum, t.ucrc); }
		{ KernelTimer k(c, "rs_layout_kernel"); launch_resize_layout(c->stream, w->n_res, w->nbt, w->shift, packed_len, new_cap, d_packed, stage, cache, d_block_first, d_block_off,
		                                                             d_res_len, d_want_len, d_block_crc, rt, d_new_block_first, d_new_block_off, d_new_block_crc, d_new_res_len, d_res_status); }
		{ KernelTimer k(c, "bk_move_kernel"); launch_blocks_move(c->stream, w->nbt, new_cap, d_new_block_off, w->addr, d_new_packed, c->cpd_blocks); }
	});
}

// ---- block splicers (include/mscomp_amd.h; kernels: splice.hip, the move in blocks.hip) ----
// A splicer holds one column -- the address of every new row's stored bytes -- and the graphs of its calls, keyed by every field of the
// views (view_args).
#pragma GCC visibility push(hidden)                     // (what the creates instantiate over the object -- std::unique_ptr's destructor -- is no export of the library)
struct mscomp_amd_splicer {
	mscomp_amd_ctx* ctx = nullptr;
	uint32_t shift = 0, n_src = 0, n_pick = 0, nbt = 0;    // block_size = 1 << shift; nbt = n_blocks_table of the NEW container
	uint32_t n_ext = 0;                                    // (a splicer made for extents: n_pick is its n_res)
	bool extents = false;                                  // made by mscomp_amd_splicer_create_extents: the scratch holds a SpliceExtTab
	GraphRun<40> run; GraphRun<41> xrun;                   // splice, splice_extents: four views, and eight or nine words
	DevBuf addr;                                           // u64 x nbt; a splicer made for extents: SpliceExtTab, the address column first
	SpliceExtTab t{};
};
#pragma GCC visibility pop
static_assert(sizeof(mscomp_amd_blocks_view) == sizeof(SpliceView) && sizeof(SpliceView) == 8 * sizeof(void*), "a view is eight words of the graph's key");
static_assert(ROW_TILE == MSCOMP_AMD_SPLICE_ROW_TILE, "the row tile the header states");

// the columns of a splicer made for extents from `base` on; returns where they end: from a null base, their bytes
static uintptr_t splice_ext_tab(SpliceExtTab& t, void* base, size_t nbt, size_t n_ext)
{
	Carve k(base);
	t.addr = k.q(nbt); t.ext_row = k.q(n_ext + 1); t.tsum = k.q(row_tiles((uint32_t)nbt)); t.flag = k.w(2);
	return k.at;
}

// both creates, from the null check of `out` on (`extents`: with the scratch of mscomp_amd_splicer_splice_extents)
static MSCompStatus splicer_create(mscomp_amd_ctx* c, uint32_t block_size, uint32_t n_src, size_t n_pick, bool extents, size_t n_ext, uint64_t n_blocks_table,
                                   uint32_t flags, mscomp_amd_splicer** out)
{
	*out = nullptr;
	if (!c || flags || !block_size_ok(block_size)) { return MSCOMP_ARG_ERROR; }
	if (n_src == 0 || n_src > MSCOMP_AMD_SPLICE_SRC_MAX || !count_ok(n_pick) || !count_ok(n_ext) || !count_ok(n_blocks_table)) { return MSCOMP_ARG_ERROR; }
	DeviceGuard g(c->device);
	if (!g.ok) { return MSCOMP_ERRNO; }
	std::unique_ptr<mscomp_amd_splicer> s(new (std::nothrow) mscomp_amd_splicer());
	if (!s) { return MSCOMP_MEM_ERROR; }
	s->ctx = c; s->shift = (uint32_t)__builtin_ctz(block_size); s->n_src = n_src; s->n_pick = (uint32_t)n_pick; s->nbt = (uint32_t)n_blocks_table;
	s->n_ext = (uint32_t)n_ext; s->extents = extents;
	const size_t bytes = extents ? splice_ext_tab(s->t, nullptr, n_blocks_table, n_ext) : 8 * (size_t)n_blocks_table;
	if (!s->addr.reserve(bytes + 64)) { (void)hipGetLastError(); return MSCOMP_MEM_ERROR; }
	if (extents) { splice_ext_tab(s->t, s->addr.p, n_blocks_table, n_ext); }
	*out = s.release();
	return MSCOMP_OK;
}

MSCompStatus mscomp_amd_splicer_create(mscomp_amd_ctx* c, uint32_t block_size, uint32_t n_src, size_t n_pick, uint64_t n_blocks_table, uint32_t flags,
                                       mscomp_amd_splicer** out)
{
	if (!out) { return MSCOMP_ARG_ERROR; }
	return splicer_create(c, block_size, n_src, n_pick, false, 0, n_blocks_table, flags, out);
}

MSCompStatus mscomp_amd_splicer_create_extents(mscomp_amd_ctx* c, uint32_t block_size, uint32_t n_src, size_t n_res, size_t n_ext, uint64_t n_blocks_table,
                                               uint32_t flags, mscomp_amd_splicer** out)
{
	if (!out) { return MSCOMP_ARG_ERROR; }
	return splicer_create(c, block_size, n_src, n_res, true, n_ext, n_blocks_table, flags, out);
}

void mscomp_amd_splicer_destroy(mscomp_amd_splicer* s) { destroy_object(s, [s] { s->addr.release(); }); }

// the views of a splicer's call; false: a view pack_views refuses, or without checksums where the new container gets them
static bool splice_views(const mscomp_amd_splicer* s, const mscomp_amd_blocks_view* src, bool want_crc, SpliceSrc& k)
{
	bool with_crc = false;
	return pack_views(src, s->n_src, want_crc, k.v, with_crc) && with_crc == want_crc;
}

MSCompStatus mscomp_amd_splicer_splice(mscomp_amd_splicer* s, const mscomp_amd_blocks_view* src, const uint64_t* d_pick, uint8_t* d_new_packed, uint64_t new_cap,
                                       uint64_t* d_new_block_first, uint64_t* d_new_block_off, uint32_t* d_new_block_crc, uint64_t* d_new_res_len, int32_t* d_status)
{
	if (!s || !src || !d_new_block_first || !d_new_block_off || (s->nbt && !d_new_packed)) { return MSCOMP_ARG_ERROR; }
	if (s->n_pick && (!d_pick || !d_new_res_len || !d_status)) { return MSCOMP_ARG_ERROR; }
	SpliceSrc k{};
	if (!splice_views(s, src, d_new_block_crc != nullptr, k)) { return MSCOMP_ARG_ERROR; }
	mscomp_amd_ctx* c = s->ctx;
	DeviceGuard g(c->device);
	if (!g.ok) { return MSCOMP_ERRNO; }
	const void* args[40];
	view_args(args, k.v, { d_pick, d_new_packed, reinterpret_cast<const void*>((uintptr_t)new_cap), d_new_block_first, d_new_block_off, d_new_block_crc, d_new_res_len, d_status });
	u64* addr = static_cast<u64*>(s->addr.p);
	return plan_run(s->run, c, args, [&] {
		{ KernelTimer t(c, "sp_layout_kernel"); launch_splice_layout(c->stream, k, s->n_src, s->n_pick, s->nbt, s->shift, new_cap, d_pick, d_new_block_first, d_new_block_off,
		                                                             d_new_block_crc, d_new_res_len, d_status, addr); }
		{ KernelTimer t(c, "bk_move_kernel"); launch_blocks_move(c->stream, s->nbt, new_cap, d_new_block_off, addr, d_new_packed, c->cpd_blocks); }
	});
}

// Splice by extents: the extent pass, the three row passes tiled over the new table, the move.
MSCompStatus mscomp_amd_splicer_splice_extents(mscomp_amd_splicer* s, const mscomp_amd_blocks_view* src, const uint64_t* d_ext_first, const uint64_t* d_ext,
                                               uint8_t* d_new_packed, uint64_t new_cap, uint64_t* d_new_block_first, uint64_t* d_new_block_off,
                                               uint32_t* d_new_block_crc, uint64_t* d_new_res_len, int32_t* d_status)
{
	if (!s || !s->extents || !src || !d_ext_first || !d_new_block_first || !d_new_block_off || (s->nbt && !d_new_packed)) { return MSCOMP_ARG_ERROR; }
	if ((s->n_ext && !d_ext) || (s->n_pick && (!d_new_res_len || !d_status))) { return MSCOMP_ARG_ERROR; }
	SpliceSrc k{};
	if (!splice_views(s, src, d_new_block_crc != nullptr, k)) { return MSCOMP_ARG_ERROR; }
	mscomp_amd_ctx* c = s->ctx;
	DeviceGuard g(c->device);
	if (!g.ok) { return MSCOMP_ERRNO; }
	const void* args[41];
	view_args(args, k.v, { d_ext_first, d_ext, d_new_packed, reinterpret_cast<const void*>((uintptr_t)new_cap), d_new_block_first, d_new_block_off, d_new_block_crc,
	                       d_new_res_len, d_status });
	return plan_run(s->xrun, c, args, [&] {
		{ KernelTimer t(c, "sx_extent_kernel"); launch_splice_extents(c->stream, k, s->n_src, s->n_pick, s->n_ext, s->nbt, s->shift, d_ext_first, d_ext, d_new_block_first,
		                                                              d_new_block_off, d_new_res_len, d_status, s->t); }
		if (s->nbt) {
			{ KernelTimer t(c, "sx_tile_kernel"); launch_splice_tiles(c->stream, k, s->n_pick, s->nbt, d_ext_first, d_ext, d_new_block_first, d_new_block_off, d_new_block_crc, s->t); }
			{ KernelTimer t(c, "sx_tilescan_kernel"); launch_splice_tilescan(c->stream, s->nbt, s->t); }
			{ KernelTimer t(c, "sx_rows_kernel"); launch_splice_rows(c->stream, s->n_pick, s->nbt, new_cap, d_ext_first, d_new_block_first, d_new_block_off, d_new_block_crc, d_status, s->t); }
		}
		{ KernelTimer t(c, "bk_move_kernel"); launch_blocks_move(c->stream, s->nbt, new_cap, d_new_block_off, s->t.addr, d_new_packed, c->cpd_blocks); }
	});
}

// ---- block dedupers (include/mscomp_amd.h; kernels: dedup.hip) ----
// A deduper holds its tables -- sized by the bound of the resources alone -- and the graph of its call, keyed as a splicer's.
#pragma GCC visibility push(hidden)                     // (what the creates instantiate over the object -- std::unique_ptr's destructor -- is no export of the library)
enum DeduperKind {                                      // the call a deduper was made for; it refuses the other four
	DEDUPER_DEDUP,                                         // mscomp_amd_deduper_create: the scratch holds a DedupTab
	DEDUPER_DIFF,                                          // _create_diff: n_res is n_pair, nbt is n_blocks_new, the scratch holds a DiffTab
	DEDUPER_MATCH,                                         // _create_match: n_src stores (0 .. 3), nbn is n_blocks_new, the scratch holds a MatchTab
	DEDUPER_REPAIR,                                        // _create_repair: n_res and nbt (= n_blocks_new) bound the primary, the scratch holds a DiffTab
	DEDUPER_MATCH_DIGEST                                   // _create_match_digest (mscomp_amd_match_digest.h): match's bounds and match's MatchTab
};
struct mscomp_amd_deduper {
	mscomp_amd_ctx* ctx = nullptr;
	uint32_t shift = 0, n_src = 0, n_res = 0, nbt = 0;     // block_size = 1 << shift; the bounds n_res_total and n_blocks_total
	DeduperKind kind = DEDUPER_DEDUP;
	uint32_t nbn = 0;
	GraphRun<37> run; GraphRun<24> frun; GraphRun<39> mrun; // dedup: four views, and five words; diff: two views, and eight; match: four views, and seven
	GraphRun<42> rrun;                                      // repair: four views, four verdict arrays, and six words
	GraphRun<43> grun;                                      // match by digest: four views, four digest columns, and seven words
	DevBuf tab;                                            // DedupTab, DiffTab or MatchTab
	DedupTab t{};
	DiffTab f{};
	MatchTab m{};
};
#pragma GCC visibility pop

// the columns of a deduper's tables from `base` on (n = n_res_total); returns where they end: from a null base, their bytes
static uintptr_t dedup_tab(DedupTab& t, void* base, size_t n)
{
	Carve k(base);
	t.kt.slots = 2 * (u64)n + 64;
	t.ufirst = k.q(n + 1); t.key = k.q(n); t.kt.key = k.q(t.kt.slots);
	t.kt.min = k.w(t.kt.slots); t.slot_of = k.w(n); t.cand = k.w(n); t.flag = k.w(n); t.rlist = k.w(n);
	return k.at;
}

// the columns of a deduper made for diff from `base` on (n = n_pair, m = n_blocks_new); returns where they end: from a null base, their bytes
static uintptr_t diff_tab(DiffTab& t, void* base, size_t n, size_t m)
{
	Carve k(base);
	t.ufirst = k.q(n + 1); t.pfirst = k.q(3 * n); t.tsum = k.q(8 * (size_t)row_tiles((uint32_t)m)); t.verdict = k.w(m);
	return k.at;
}

// the columns of a deduper made for match from `base` on (n = n_res_total, m = n_blocks_total, mn = n_blocks_new); returns where they end:
// from a null base, their bytes
static uintptr_t match_tab(MatchTab& t, void* base, size_t n, size_t m, size_t mn)
{
	Carve k(base);
	const size_t slots = 2 * m + 64;
	t.kt.slots = slots < 0xFFFFFFF0u ? slots : 0xFFFFFFF0u;   // (a slot's index is a 32-bit word, and all-ones is KT_NONE)
	t.ufirst = k.q(n + 1); t.pfirst = k.q(5 * n); t.tsum = k.q(8 * (size_t)row_tiles((uint32_t)mn)); t.kt.key = k.q(slots); t.nref = k.q(1);
	t.kt.min = k.w(slots); t.slot_of = k.w(m); t.flag = k.w(m); t.rep = k.w(m); t.rlist = k.w(m); t.flocal = k.w(mn);
	return k.at;
}

// The five creates: args_ok = the create's own check of its counts; fill(d, base) sets the bounds in d and lays the columns of its tables
// out from `base` on, returning where they end: from a null base, their bytes.
template <class Fill>
static MSCompStatus deduper_create(mscomp_amd_ctx* c, uint32_t block_size, uint32_t flags, mscomp_amd_deduper** out, DeduperKind kind, bool args_ok, Fill fill)
{
	if (!out) { return MSCOMP_ARG_ERROR; }
	*out = nullptr;
	if (!c || flags || !block_size_ok(block_size) || !args_ok) { return MSCOMP_ARG_ERROR; }
	DeviceGuard g(c->device);
	if (!g.ok) { return MSCOMP_ERRNO; }
	std::unique_ptr<mscomp_amd_deduper> d(new (std::nothrow) mscomp_amd_deduper());
	if (!d) { return MSCOMP_MEM_ERROR; }
	d->ctx = c; d->shift = (uint32_t)__builtin_ctz(block_size); d->kind = kind;
	if (!d->tab.reserve(fill(*d, nullptr) + 64)) { (void)hipGetLastError(); return MSCOMP_MEM_ERROR; }
	fill(*d, d->tab.p);
	*out = d.release();
	return MSCOMP_OK;
}

MSCompStatus mscomp_amd_deduper_create(mscomp_amd_ctx* c, uint32_t block_size, uint32_t n_src, size_t n_res_total, uint64_t n_blocks_total, uint32_t flags,
                                       mscomp_amd_deduper** out)
{
	const bool args_ok = n_src != 0 && n_src <= MSCOMP_AMD_SPLICE_SRC_MAX && count_ok(n_res_total) && count_ok(n_blocks_total);
	return deduper_create(c, block_size, flags, out, DEDUPER_DEDUP, args_ok, [&](mscomp_amd_deduper& d, void* base) {
		d.n_src = n_src; d.n_res = (uint32_t)n_res_total; d.nbt = (uint32_t)n_blocks_total;
		return dedup_tab(d.t, base, n_res_total);
	});
}

MSCompStatus mscomp_amd_deduper_create_diff(mscomp_amd_ctx* c, uint32_t block_size, size_t n_pair, uint64_t n_blocks_new, uint32_t flags, mscomp_amd_deduper** out)
{
	return deduper_create(c, block_size, flags, out, DEDUPER_DIFF, count_ok(n_pair) && count_ok(n_blocks_new), [&](mscomp_amd_deduper& d, void* base) {
		d.n_src = 2; d.n_res = (uint32_t)n_pair; d.nbt = (uint32_t)n_blocks_new;
		return diff_tab(d.f, base, n_pair, n_blocks_new);
	});
}

MSCompStatus mscomp_amd_deduper_create_match(mscomp_amd_ctx* c, uint32_t block_size, uint32_t n_src, size_t n_res_total, uint64_t n_blocks_total, uint64_t n_blocks_new,
                                             uint32_t flags, mscomp_amd_deduper** out)
{
	const bool args_ok = n_src < MSCOMP_AMD_SPLICE_SRC_MAX && count_ok(n_res_total) && count_ok(n_blocks_total) && n_blocks_new <= n_blocks_total;
	return deduper_create(c, block_size, flags, out, DEDUPER_MATCH, args_ok, [&](mscomp_amd_deduper& d, void* base) {
		d.n_src = n_src; d.n_res = (uint32_t)n_res_total; d.nbt = (uint32_t)n_blocks_total; d.nbn = (uint32_t)n_blocks_new;
		return match_tab(d.m, base, n_res_total, n_blocks_total, n_blocks_new);
	});
}

// (the checks, the bounds and the scratch of mscomp_amd_deduper_create_match: the passes that are its own read columns the caller brings)
MSCompStatus mscomp_amd_deduper_create_match_digest(mscomp_amd_ctx* c, uint32_t block_size, uint32_t n_src, size_t n_res_total, uint64_t n_blocks_total,
                                                    uint64_t n_blocks_new, uint32_t flags, mscomp_amd_deduper** out)
{
	const bool args_ok = n_src < MSCOMP_AMD_SPLICE_SRC_MAX && count_ok(n_res_total) && count_ok(n_blocks_total) && n_blocks_new <= n_blocks_total;
	return deduper_create(c, block_size, flags, out, DEDUPER_MATCH_DIGEST, args_ok, [&](mscomp_amd_deduper& d, void* base) {
		d.n_src = n_src; d.n_res = (uint32_t)n_res_total; d.nbt = (uint32_t)n_blocks_total; d.nbn = (uint32_t)n_blocks_new;
		return match_tab(d.m, base, n_res_total, n_blocks_total, n_blocks_new);
	});
}

MSCompStatus mscomp_amd_deduper_create_repair(mscomp_amd_ctx* c, uint32_t block_size, uint32_t n_src, size_t n_res, uint64_t n_blocks_new, uint32_t flags,
                                              mscomp_amd_deduper** out)
{
	const bool args_ok = n_src != 0 && n_src <= MSCOMP_AMD_SPLICE_SRC_MAX && count_ok(n_res) && count_ok(n_blocks_new);
	return deduper_create(c, block_size, flags, out, DEDUPER_REPAIR, args_ok, [&](mscomp_amd_deduper& d, void* base) {
		d.n_src = n_src; d.n_res = (uint32_t)n_res; d.nbt = (uint32_t)n_blocks_new;
		return diff_tab(d.f, base, n_res, n_blocks_new);
	});
}

void mscomp_amd_deduper_destroy(mscomp_amd_deduper* d) { destroy_object(d, [d] { d->tab.release(); }); }

// whether every one of the n_views views lies within the deduper's bounds n_res and nbt, and their sums do; n = the resources of the call
static bool views_within(const mscomp_amd_deduper* d, const mscomp_amd_blocks_view* src, uint32_t n_views, uint64_t& n)
{
	uint64_t rows = 0;                                     // (at most four terms below 2^64 / 4 each once checked: no overflow)
	n = 0;
	for (uint32_t i = 0; i < n_views; ++i) {
		if (src[i].n_res > d->n_res || src[i].n_blocks_table > d->nbt) { return false; }
		n += src[i].n_res; rows += src[i].n_blocks_table;
	}
	return n <= d->n_res && rows <= d->nbt;
}

MSCompStatus mscomp_amd_deduper_dedup(mscomp_amd_deduper* d, const mscomp_amd_blocks_view* src, uint64_t* d_rep, uint64_t* d_new_index, uint64_t* d_pick,
                                      uint64_t* d_count, int32_t* d_status)
{
	if (!d || d->kind != DEDUPER_DEDUP || !src || !d_count) { return MSCOMP_ARG_ERROR; }
	SpliceSrc k{};
	bool with_crc = false;                                 // the checksums are used only if every view has them
	if (!pack_views(src, d->n_src, true, k.v, with_crc)) { return MSCOMP_ARG_ERROR; }
	uint64_t n = 0;
	if (!views_within(d, src, d->n_src, n)) { return MSCOMP_ARG_ERROR; }
	if (n && (!d_rep || !d_new_index || !d_pick || !d_status)) { return MSCOMP_ARG_ERROR; }
	mscomp_amd_ctx* c = d->ctx;
	DeviceGuard g(c->device);
	if (!g.ok) { return MSCOMP_ERRNO; }
	const void* args[37];
	view_args(args, k.v, { d_rep, d_new_index, d_pick, d_count, d_status });
	const uint32_t N = (uint32_t)n;
	return plan_run(d->run, c, args, [&] {
		{ KernelTimer t(c, "dd_judge"); launch_dedup_judge(c->stream, k, N, d->n_res, d->nbt, d->shift, d->t, d_status, c->crc_blocks); }
		{ KernelTimer t(c, "dd_keys"); launch_dedup_keys(c->stream, k, N, d->n_res, d->nbt, with_crc, d->t, d_status, c->crc_blocks); }
		{ KernelTimer t(c, "dd_confirm_kernel"); launch_dedup_confirm(c->stream, k, N, d->n_res, d->nbt, d->shift, with_crc, d->t, c->cpd_blocks); }
		{ KernelTimer t(c, "dd_settle_kernel"); launch_dedup_settle(c->stream, k, N, d->n_res, with_crc, d->t, d_rep, d_new_index, d_pick, d_count); }
	});
}

// Diff: the seed, the rows' verdicts from the tables, the compare that confirms the candidates, the three run passes tiled
// over the new rows, the counts.
MSCompStatus mscomp_amd_deduper_diff(mscomp_amd_deduper* d, const mscomp_amd_blocks_view* base, const mscomp_amd_blocks_view* next, const uint64_t* d_pair,
                                     uint64_t* d_delta_ext_first, uint64_t* d_delta_ext, uint64_t* d_patch_ext_first, uint64_t* d_patch_ext, uint64_t* d_changed,
                                     uint64_t* d_count, int32_t* d_status)
{
	if (!d || d->kind != DEDUPER_DIFF || !base || !next || !d_count) { return MSCOMP_ARG_ERROR; }   // (a deduper made for dedup, for match or for repair)
	if (d->n_res && (!d_pair || !d_delta_ext_first || !d_patch_ext_first || !d_changed || !d_status || (d->nbt && (!d_delta_ext || !d_patch_ext)))) { return MSCOMP_ARG_ERROR; }
	const mscomp_amd_blocks_view src[2] = { *base, *next };
	SpliceView v[2];
	bool with_crc = false;                                 // the checksums are used only if both views have them
	if (!pack_views(src, 2, true, v, with_crc)) { return MSCOMP_ARG_ERROR; }
	mscomp_amd_ctx* c = d->ctx;
	DeviceGuard g(c->device);
	if (!g.ok) { return MSCOMP_ERRNO; }
	const void* args[24];
	view_args(args, v, { d_pair, d_delta_ext_first, d_delta_ext, d_patch_ext_first, d_patch_ext, d_changed, d_count, d_status });
	const uint32_t n = d->n_res, m = d->nbt;
	return plan_run(d->frun, c, args, [&] {
		{ KernelTimer t(c, "df_seed_kernel"); launch_diff_seed(c->stream, v[0], v[1], n, m, d->shift, d_pair, d->f, d_status); }
		if (n && m) {
			{ KernelTimer t(c, "df_verdict_kernel"); launch_diff_verdicts(c->stream, v[0], v[1], n, m, d->shift, with_crc, d_pair, d->f, d_status, c->crc_blocks); }
			{ KernelTimer t(c, "df_confirm_kernel"); launch_diff_confirm(c->stream, v[0], v[1], n, m, d->shift, d_pair, d->f, d_status, c->cpd_blocks); }
			{ KernelTimer t(c, "df_runs"); launch_diff_runs(c->stream, v[1], n, m, d_pair, d->f, d_status, d_delta_ext, d_patch_ext); }
		}
		{ KernelTimer t(c, "df_counts_kernel"); launch_diff_counts(c->stream, n, m, d->f, d_delta_ext_first, d_patch_ext_first, d_changed, d_count, c->crc_blocks); }
	});
}

// Match: the key table cleared, the seed, rule 3 over the rows, the rows' keys into the table, the compare that confirms a
// row against its slot's smallest, the settle, the three run passes tiled over next's rows, the counts.
MSCompStatus mscomp_amd_deduper_match(mscomp_amd_deduper* d, const mscomp_amd_blocks_view* store, const mscomp_amd_blocks_view* next, uint64_t* d_delta_ext_first,
                                      uint64_t* d_delta_ext, uint64_t* d_patch_ext_first, uint64_t* d_patch_ext, uint64_t* d_class, uint64_t* d_count, int32_t* d_status)
{
	if (!d || d->kind != DEDUPER_MATCH || !next || !d_count || (d->n_src && !store)) { return MSCOMP_ARG_ERROR; }
	if (d->n_res && (!d_delta_ext_first || !d_patch_ext_first || !d_class || !d_status || (d->nbn && (!d_delta_ext || !d_patch_ext)))) { return MSCOMP_ARG_ERROR; }
	mscomp_amd_blocks_view src[MSCOMP_AMD_SPLICE_SRC_MAX];
	for (uint32_t i = 0; i < d->n_src; ++i) { src[i] = store[i]; }
	src[d->n_src] = *next;
	SpliceSrc k{};
	bool with_crc = false;                                 // the checksums are used only if every view has them
	if (!pack_views(src, d->n_src + 1, true, k.v, with_crc)) { return MSCOMP_ARG_ERROR; }
	uint64_t n = 0;
	if (!views_within(d, src, d->n_src + 1, n) || next->n_blocks_table > d->nbn) { return MSCOMP_ARG_ERROR; }
	mscomp_amd_ctx* c = d->ctx;
	DeviceGuard g(c->device);
	if (!g.ok) { return MSCOMP_ERRNO; }
	const void* args[39];
	view_args(args, k.v, { d_delta_ext_first, d_delta_ext, d_patch_ext_first, d_patch_ext, d_class, d_count, d_status });
	const uint32_t N = (uint32_t)n, n_store = (uint32_t)(n - next->n_res);
	return plan_run(d->mrun, c, args, [&] {
		const MatchTab& t = d->m;
		{ KernelTimer tm(c, "dd_clear_kernel"); launch_dedup_clear(c->stream, t.kt, c->crc_blocks); }
		{ KernelTimer tm(c, "mt_seed_kernel"); launch_match_seed(c->stream, k, N, n_store, d->nbt, d->nbn, d->shift, t, d_status); }
		if (d->nbt) {
			{ KernelTimer tm(c, "dd_rows_kernel"); launch_dedup_rule3(c->stream, k, N, d->nbt, t.ufirst, d_status, c->crc_blocks); }
			{ KernelTimer tm(c, "mt_keys_kernel"); launch_match_keys(c->stream, k, N, d->nbt, d->shift, with_crc, t, d_status, c->crc_blocks); }
			{ KernelTimer tm(c, "mt_confirm_kernel"); launch_match_confirm(c->stream, k, N, d->nbt, d->shift, with_crc, t, c->cpd_blocks); }
			{ KernelTimer tm(c, "mt_settle_kernel"); launch_match_settle(c->stream, k, N, d->shift, with_crc, t); }
		}
		if (d->nbn) { KernelTimer tm(c, "mt_runs"); launch_match_runs(c->stream, k, d->n_src, N, n_store, d->nbn, d->shift, t, d_status, d_delta_ext, d_patch_ext); }
		{ KernelTimer tm(c, "mt_counts_kernel"); launch_match_counts(c->stream, N, n_store, d->nbn, d->nbt != 0, t, d_delta_ext_first, d_patch_ext_first, d_class, d_count, c->crc_blocks); }
	});
}

// Match by digest (include/mscomp_amd_match_digest.h): match's ten launches with keys, confirm and settle over the views'
// digest columns. No kernel dereferences a view's stored bytes: they go in as null, and the packed length alone stays, for rule 3.
MSCompStatus mscomp_amd_deduper_match_digest(mscomp_amd_deduper* d, const mscomp_amd_blocks_view* store, const uint32_t* const* d_store_digest,
                                             const mscomp_amd_blocks_view* next, const uint32_t* d_next_digest, uint64_t* d_delta_ext_first, uint64_t* d_delta_ext,
                                             uint64_t* d_patch_ext_first, uint64_t* d_patch_ext, uint64_t* d_class, uint64_t* d_count, int32_t* d_status)
{
	if (!d || d->kind != DEDUPER_MATCH_DIGEST || !next || !d_count || (d->n_src && (!store || !d_store_digest))) { return MSCOMP_ARG_ERROR; }
	if (d->n_res && (!d_delta_ext_first || !d_patch_ext_first || !d_class || !d_status || (d->nbn && (!d_delta_ext || !d_patch_ext)))) { return MSCOMP_ARG_ERROR; }
	mscomp_amd_blocks_view src[MSCOMP_AMD_SPLICE_SRC_MAX];
	DigestCols cols{};
	for (uint32_t i = 0; i <= d->n_src; ++i) {
		src[i] = i < d->n_src ? store[i] : *next;
		cols.c[i] = i < d->n_src ? d_store_digest[i] : d_next_digest;
		if ((src[i].n_res && !cols.c[i]) || (uintptr_t)cols.c[i] % 16u) { return MSCOMP_ARG_ERROR; }
		src[i].d_packed = nullptr; src[i].packed_len = 0;                  // (pack_views asks for stored bytes where it is told of some)
	}
	SpliceSrc k{};
	bool with_crc = false;                                 // no checksum takes part: the views go without their CRC columns
	if (!pack_views(src, d->n_src + 1, false, k.v, with_crc)) { return MSCOMP_ARG_ERROR; }
	for (uint32_t i = 0; i <= d->n_src; ++i) { k.v[i].packed_len = src[i].packed_len = i < d->n_src ? store[i].packed_len : next->packed_len; }
	uint64_t n = 0;
	if (!views_within(d, src, d->n_src + 1, n) || next->n_blocks_table > d->nbn) { return MSCOMP_ARG_ERROR; }
	mscomp_amd_ctx* c = d->ctx;
	DeviceGuard g(c->device);
	if (!g.ok) { return MSCOMP_ERRNO; }
	const void* args[43];
	view_args(args, k.v, { cols.c[0], cols.c[1], cols.c[2], cols.c[3], d_delta_ext_first, d_delta_ext, d_patch_ext_first, d_patch_ext, d_class, d_count, d_status });
	const uint32_t N = (uint32_t)n, n_store = (uint32_t)(n - next->n_res);
	return plan_run(d->grun, c, args, [&] {
		const MatchTab& t = d->m;
		{ KernelTimer tm(c, "dd_clear_kernel"); launch_dedup_clear(c->stream, t.kt, c->crc_blocks); }
		{ KernelTimer tm(c, "mt_seed_kernel"); launch_match_seed(c->stream, k, N, n_store, d->nbt, d->nbn, d->shift, t, d_status); }
		if (d->nbt) {
			{ KernelTimer tm(c, "dd_rows_kernel"); launch_dedup_rule3(c->stream, k, N, d->nbt, t.ufirst, d_status, c->crc_blocks); }
			{ KernelTimer tm(c, "md_keys_kernel"); launch_match_digest_keys(c->stream, k, cols, N, d->nbt, d->shift, t, d_status, c->crc_blocks); }
			{ KernelTimer tm(c, "md_confirm_kernel"); launch_match_digest_confirm(c->stream, k, cols, N, d->nbt, d->shift, t, c->crc_blocks); }
			{ KernelTimer tm(c, "md_settle_kernel"); launch_match_digest_settle(c->stream, k, cols, N, d->shift, t); }
		}
		if (d->nbn) { KernelTimer tm(c, "mt_runs"); launch_match_runs(c->stream, k, d->n_src, N, n_store, d->nbn, d->shift, t, d_status, d_delta_ext, d_patch_ext); }
		{ KernelTimer tm(c, "mt_counts_kernel"); launch_match_counts(c->stream, N, n_store, d->nbn, d->nbt != 0, t, d_delta_ext_first, d_patch_ext_first, d_class, d_count, c->crc_blocks); }
	});
}

// Repair: the seed, the rows' choices from the tables and the verdicts, the three run passes tiled over the primary's rows
// (the middle one is diff's), the counts.
MSCompStatus mscomp_amd_deduper_repair(mscomp_amd_deduper* d, const mscomp_amd_blocks_view* src, const uint32_t* const* d_verdict, uint64_t* d_ext_first, uint64_t* d_ext,
                                       uint64_t* d_fixed, uint64_t* d_lost, uint64_t* d_count, int32_t* d_status)
{
	if (!d || d->kind != DEDUPER_REPAIR || !src || !d_verdict || !d_count) { return MSCOMP_ARG_ERROR; }   // (a deduper made for dedup, for diff or for match)
	if (d->n_res && (!d_ext_first || !d_fixed || !d_lost || !d_status || (d->nbt && !d_ext))) { return MSCOMP_ARG_ERROR; }
	SpliceSrc k{};
	bool with_crc = false;                                 // the checksums take part only if every view has them
	if (!pack_views(src, d->n_src, true, k.v, with_crc)) { return MSCOMP_ARG_ERROR; }
	const uint32_t* q[4] = { nullptr, nullptr, nullptr, nullptr };
	for (uint32_t i = 0; i < d->n_src; ++i) {
		if (src[i].n_res && src[i].n_blocks_table && !d_verdict[i]) { return MSCOMP_ARG_ERROR; }
		q[i] = d_verdict[i];
	}
	mscomp_amd_ctx* c = d->ctx;
	DeviceGuard g(c->device);
	if (!g.ok) { return MSCOMP_ERRNO; }
	const void* args[42];
	view_args(args, k.v, { q[0], q[1], q[2], q[3], d_ext_first, d_ext, d_fixed, d_lost, d_count, d_status });
	const uint32_t n = d->n_res, m = d->nbt;
	return plan_run(d->rrun, c, args, [&] {
		{ KernelTimer t(c, "rp_seed_kernel"); launch_repair_seed(c->stream, k.v[0], n, m, d->shift, d->f, d_status, d_count); }
		if (n && m) {
			{ KernelTimer t(c, "rp_choice_kernel"); launch_repair_choice(c->stream, k, q, d->n_src, n, m, d->shift, with_crc, d->f, c->crc_blocks); }
			{ KernelTimer t(c, "rp_runs"); launch_repair_runs(c->stream, k, n, m, d->f, d_ext); }
		}
		{ KernelTimer t(c, "rp_counts_kernel"); launch_repair_counts(c->stream, n, m, d->f, d_ext_first, d_fixed, d_lost, d_count, d_status, c->crc_blocks); }
	});
}

// ---- block transcoders (include/mscomp_amd.h; kernels: transcode.hip, the fold in crc32.hip, the move in blocks.hip) ----
// A transcoder holds what a writer holds -- a decompress dev plan for the old format, a compress dev plan for the new one, a cache and a
// staging area -- sized by groups_max groups of G = max(B1, B2) bytes, its tables, and the graph of its call. Slot w of cache and staging
// belongs to the w-th worked group of an execution; a unit's place in it follows from its block's place in the group, so neither inner
// plan's tables are compacted.
struct mscomp_amd_transcoder {
	mscomp_amd_ctx* ctx = nullptr;
	MSCompFormat f1 = MSCOMP_NONE, f2 = MSCOMP_NONE;
	TcDims d{};
	uint32_t dm = 0, em = 0;                           // the units of the inner plans: groups_max G / B1, groups_max G / B2
	InnerPlans in;                                     // (plans: null when groups_max is 0; cache and staging area: groups_max slots of G bytes each)
	GraphRun<12> run;
	DevBuf tab;                                        // TranscodeTab
	TranscodeTab t{};
	bool ran = false;
};

// the columns of a transcoder's tables from `base` on; returns where they end: from a null base, their bytes
static uintptr_t transcode_tab(TranscodeTab& t, void* base, const TcDims& d, size_t dm, size_t em)
{
	const size_t n = d.n_res, ng = d.ngmax, m = d.nbn;
	Carve k(base);
	t.gfirst = k.q(n + 1); t.pfirst = k.q(n + 1);
	t.plen = k.q(m); t.paddr = k.q(m); t.pjf = k.q(m); t.pdl = k.q(m); t.addr = k.q(m); t.tsum = k.q(row_tiles((uint32_t)m));
	t.d_in_off = k.q(dm); t.d_in_len = k.q(dm); t.d_out_off = k.q(dm); t.d_out_cap = k.q(dm); t.d_ulen = k.q(dm);
	t.d_src = k.q(dm); t.d_clen = k.q(dm); t.d_cum = k.q(dm + 1); t.d_row = k.q(dm); t.d_raw = k.q(dm);
	t.e_in_off = k.q(em); t.e_in_len = k.q(em); t.e_out_off = k.q(em); t.e_out_cap = k.q(em); t.e_ulen = k.q(em);
	t.e_src = k.q(em); t.e_clen = k.q(em); t.e_cum = k.q(em + 1);
	t.rstat = k.i(n); t.gres = k.w(ng); t.gwork = k.w(ng); t.gcum = k.w(ng); t.slot_group = k.w(d.gmax);
	t.pkind = k.w(m); t.pcrc = k.w(m);
	t.d_ustat = k.i(dm); t.d_act = k.w(dm); t.d_crc = k.w(dm); t.e_ustat = k.i(em); t.e_crc = k.w(em);
	t.cnt = k.w(4);
	return k.at;
}

MSCompStatus mscomp_amd_transcoder_create(mscomp_amd_ctx* c, MSCompFormat format, uint32_t block_size, MSCompFormat new_format, uint32_t new_block_size, size_t n_res,
                                          uint64_t n_blocks_table, uint64_t n_blocks_new, uint64_t groups_max, uint32_t flags, mscomp_amd_transcoder** out)
{
	if (!out) { return MSCOMP_ARG_ERROR; }
	*out = nullptr;
	if (!create_args_ok(c, format, block_size, flags) || !create_args_ok(c, new_format, new_block_size, flags)) { return MSCOMP_ARG_ERROR; }
	if (!count_ok(n_res) || !count_ok(n_blocks_table) || !count_ok(n_blocks_new) || !count_ok(groups_max)) { return MSCOMP_ARG_ERROR; }
	if (format == new_format && block_size == new_block_size) { return MSCOMP_ARG_ERROR; }   // (nothing to change: a splice)
	TcDims d{};
	d.n_res = (uint32_t)n_res; d.nbt = (uint32_t)n_blocks_table; d.nbn = (uint32_t)n_blocks_new; d.gmax = (uint32_t)groups_max;
	d.s1 = (uint32_t)__builtin_ctz(block_size); d.s2 = (uint32_t)__builtin_ctz(new_block_size); d.sg = d.s1 > d.s2 ? d.s1 : d.s2;
	d.ngmax = d.s2 > d.s1 ? d.nbn : d.nbt;                 // a group holds at least one block of the coarser table
	d.mode = format != MSCOMP_LZNT1 || new_format != MSCOMP_LZNT1 ? TC_GENERIC : d.s2 > d.s1 ? TC_JOIN : TC_SPLIT;
	const uint64_t dm = groups_max << (d.sg - d.s1), em = groups_max << (d.sg - d.s2), bytes = groups_max << d.sg;   // (< 2^50)
	uint64_t I = 0, chunks = 0, toks = 0, cands = 0;
	if (!count_ok(dm) || !count_ok(em) || !decode_dev_counts(format, dm, bytes, bytes, false, I, chunks, toks, cands)) { return MSCOMP_MEM_ERROR; }   // (what the inner plans would refuse: checked before the context is used)
	DeviceGuard g(c->device);
	if (!g.ok) { return MSCOMP_ERRNO; }
	std::unique_ptr<mscomp_amd_transcoder> x(new (std::nothrow) mscomp_amd_transcoder());
	if (!x) { return MSCOMP_MEM_ERROR; }
	x->ctx = c; x->f1 = format; x->f2 = new_format; x->d = d; x->dm = (uint32_t)dm; x->em = (uint32_t)em;
	const uint64_t slots = bytes ? bytes + 64 : 0;
	const MSCompStatus st = x->in.create(c, x->tab, transcode_tab(x->t, nullptr, d, dm, em) + 64, slots, slots, bytes, format, dm, new_format, em, new_block_size);
	if (st != MSCOMP_OK) { return st; }
	transcode_tab(x->t, x->tab.p, d, dm, em);
	*out = x.release();
	return MSCOMP_OK;
}

void mscomp_amd_transcoder_destroy(mscomp_amd_transcoder* x) { destroy_object(x, [x] { x->in.destroy(); x->tab.release(); }); }

// The call: rules 0-3 from the tables, the slots and both inner plans' units, the writer's decode-into-cache /
// encode-into-staging sequence over them with the CRC passes, the new tables tiled over their rows, the move.
MSCompStatus mscomp_amd_transcoder_transcode(mscomp_amd_transcoder* x, const uint8_t* d_packed, uint64_t packed_len, const uint64_t* d_block_first,
                                             const uint64_t* d_block_off, const uint64_t* d_res_len, const uint32_t* d_block_crc,
                                             uint8_t* d_new_packed, uint64_t new_cap, uint64_t* d_new_block_first, uint64_t* d_new_block_off,
                                             uint32_t* d_new_block_crc, int32_t* d_status)
{
	if (!x || !d_block_first || !d_block_off || !d_new_block_first || !d_new_block_off || (x->d.n_res && (!d_res_len || !d_status))) { return MSCOMP_ARG_ERROR; }
	if ((x->d.nbt && !d_packed) || (x->d.nbn && !d_new_packed)) { return MSCOMP_ARG_ERROR; }
	if ((d_block_crc == nullptr) != (d_new_block_crc == nullptr)) { return MSCOMP_ARG_ERROR; }
	mscomp_amd_ctx* c = x->ctx;
	DeviceGuard g(c->device);
	if (!g.ok) { return MSCOMP_ERRNO; }
	x->in.mark_ran(); x->ran = true;
	const void* args[12] = { d_packed, reinterpret_cast<const void*>((uintptr_t)packed_len), d_block_first, d_block_off, d_res_len, d_block_crc, d_new_packed,
	                         reinterpret_cast<const void*>((uintptr_t)new_cap), d_new_block_first, d_new_block_off, d_new_block_crc, d_status };
	return plan_run(x->run, c, args, [&] {
		const TcDims& d = x->d;
		const TranscodeTab& t = x->t;
		const bool with_crc = d_block_crc != nullptr;
		uint8_t* cache = static_cast<uint8_t*>(x->in.cache.p); uint8_t* stage = static_cast<uint8_t*>(x->in.stage.p);
		{ KernelTimer k(c, "tc_res_kernel"); launch_tc_resources(c->stream, d, d_block_first, d_res_len, t); }
		{ KernelTimer k(c, "tc_class_kernel"); launch_tc_classes(c->stream, d, d_packed, packed_len, d_block_first, d_block_off, d_res_len, with_crc, t); }
		{ KernelTimer k(c, "tc_units"); launch_tc_units(c->stream, d, d_packed, cache, d_block_first, d_block_off, d_res_len, with_crc, t); }
		// the worked groups: decoded (or copied) into the cache, held to their old checksums, encoded into the staging area, checksummed
		if (x->in.dplan) { dev_launch(x->in.dplan, d_packed, t.d_in_off, t.d_in_len, cache, t.d_out_off, t.d_out_cap, t.d_ulen, t.d_ustat); }
		{ KernelTimer k(c, "tc_gather_kernel"); launch_tc_gather(c->stream, d, cache, t, c->cpd_blocks); }
		if (with_crc && x->dm) { crc_pass(c, x->dm, nullptr, t.d_src, t.d_clen, t.d_cum, t.d_crc); }   // (addresses as offsets from a null base)
		{ KernelTimer k(c, "tc_judge_kernel"); launch_tc_judge(c->stream, d, d_block_crc, t); }
		if (x->in.cplan) { dev_launch(x->in.cplan, nullptr, t.e_in_off, t.e_in_len, stage, t.e_out_off, t.e_out_cap, t.e_ulen, t.e_ustat); }
		if (with_crc && x->em) { crc_pass(c, x->em, nullptr, t.e_src, t.e_clen, t.e_cum, t.e_crc); }
		if (with_crc && d.mode == TC_JOIN) { KernelTimer k(c, "crc_foldruns_kernel"); launch_crc_fold_runs(c->stream, d.nbn, t.pfirst + d.n_res, d.s1, t.pjf, t.pdl, d_block_crc, t.pcrc); }
		// the new tables and the bytes
		{ KernelTimer k(c, "tc_first_kernel"); launch_tc_first(c->stream, d, d_res_len, t, d_new_block_first, d_new_block_off, d_status); }
		if (d.nbn) {
			const SpliceExtTab rows = { t.addr, nullptr, t.tsum, t.cnt + 3 };
			{ KernelTimer k(c, "tc_tile_kernel"); launch_tc_tiles(c->stream, d, stage, d_res_len, with_crc, t, d_new_block_first, d_new_block_off, d_new_block_crc); }
			{ KernelTimer k(c, "sx_tilescan_kernel"); launch_splice_tilescan(c->stream, d.nbn, rows); }
			{ KernelTimer k(c, "tc_rows_kernel"); launch_tc_rows(c->stream, d, new_cap, t, d_new_block_first, d_new_block_off, d_new_block_crc, d_status); }
		}
		{ KernelTimer k(c, "bk_move_kernel"); launch_blocks_move(c->stream, d.nbn, new_cap, d_new_block_off, t.addr, d_new_packed, c->cpd_blocks); }
	});
}

// new blocks carried, source blocks decoded and new blocks encoded by x's last execution (read back; none before the first, none for a
// refused table)
int mscomp_amd_transcoder_counts(mscomp_amd_transcoder* x, uint32_t out[3])
{
	if (!x || !out) { return -1; }
	DeviceGuard g(x->ctx->device);
	if (!g.ok || hipStreamSynchronize(x->ctx->stream) != hipSuccess) { return -1; }
	out[0] = out[1] = out[2] = 0;
	if (!x->ran) { return 0; }
	uint32_t cnt[4] = {};
	if (hipMemcpy(cnt, x->t.cnt, 16, hipMemcpyDeviceToHost) != hipSuccess) { return -1; }
	if (cnt[3] == 0) { out[0] = cnt[0]; out[1] = cnt[1]; out[2] = cnt[2]; }
	return 0;
}

// ---- block syncers (include/mscomp_amd.h; kernels: sync.hip, the reader's passes in reader.hip) ----
// A syncer is a reader core -- BlockAccess with n_cand_max requests of one block each: the inner decompress dev plan, the cache, the
// reader's tables -- beside tables of its own: the key table and bitmap of the store's checksums, the numberings and boundary registers of
// the units, the words of the scan's tiles, the kept candidates. The per-block-size constants of the scan are written here, once.
// A DIGEST syncer (mscomp_amd_syncer_create_digest) has no reader core: of BlockAccess it holds the bounds alone -- no inner plan, no
// cache, no reader's tables --, and beside the syncer's tables a unit table, the leaf digests and a digest per kept candidate (digest.hip).
struct mscomp_amd_syncer : BlockAccess {
	uint32_t n_units = 0;
	uint64_t in_total_max = 0;
	bool digest = false;                               // confirms by digest: only mscomp_amd_syncer_sync_digest runs on it, and only on it
	GraphRun<20> run;                                  // one view, and twelve words
	DevBuf stab;                                       // SyncTab
	SyncTab s{};
	DevBuf dtab;                                       // a digest syncer's: sync_digest_tab
	DigestTab d{};
	u64* doff = nullptr; u64* dlen = nullptr;          // (d.off, d.len, writable)
};
static_assert(SYNC_TILE == MSCOMP_AMD_SYNC_TILE && SYNC_TILE <= 4096u, "the tile the header states, within the smallest block size");

// the columns of a syncer's tables from `base` on; returns where they end: from a null base, their bytes
static uintptr_t sync_tab(SyncTab& t, void* base, size_t n, size_t nbt, size_t nu, size_t nc, uint64_t in_total_max)
{
	Carve k(base);
	size_t slots = 64;
	uint32_t slot_shift = 32u - 6u;
	while (slots < 2 * nbt + 64) { slots <<= 1; --slot_shift; }          // (at most 2^32: nbt <= 0x7FFFFFF0)
	const size_t tiles = (size_t)(in_total_max / SYNC_TILE) + nu, pieces = (size_t)(in_total_max / SYNC_RUN) + nu;
	t.kt.slots = slots; t.slot_shift = slot_shift; t.tiles_max = (uint32_t)tiles;
	t.ufirst = k.q(n + 1); t.kt.key = k.q(slots); t.cum = k.q(nu + 1); t.uoff = k.q(nu); t.ulen = k.q(nu); t.pfirst = k.q(nu + 1); t.tfirst = k.q(nu + 1);
	t.tword = k.q(8 * tiles); t.cpos = k.q(nc); t.req = k.q(3 * nc); t.qlen = k.q(nc); t.count = k.q(8);
	t.kt.min = k.w(slots); t.bits = k.w(SYNC_BIT_WORDS); t.consts = k.w(SYNC_CONSTS); t.pabs = k.w(pieces); t.traw = k.w(tiles);
	t.cunit = k.w(nc); t.crow = k.w(nc); t.flag = k.w(nc); t.qstat = k.i(nc);
	return k.at;
}

// what a digest syncer adds to them, from `base` on (nc = n_cand_max; y->s laid out): the 16-byte columns first, so that they stay aligned
static uintptr_t sync_digest_tab(mscomp_amd_syncer* y, void* base, size_t nc, uint32_t shift)
{
	Carve k(base);
	y->d.leaf = k.w(4 * (nc << (shift - DG_LEAF_SHIFT))); y->d.out = k.w(4 * nc); y->doff = k.q(nc); y->dlen = k.q(nc);
	y->d.off = y->doff; y->d.len = y->dlen; y->d.count = y->s.count + 2; y->d.n_max = (uint32_t)nc; y->d.shift = shift;   // (count[2]: the kept candidates)
	return k.at;
}

// both creates, from the null check of `out` on. A digest syncer takes no format and reserves no reader core.
static MSCompStatus syncer_create(mscomp_amd_ctx* c, bool digest, MSCompFormat format, uint32_t block_size, size_t n_res, uint64_t n_blocks_table, size_t n_units,
                                  uint64_t in_total_max, uint64_t n_cand_max, uint32_t flags, mscomp_amd_syncer** out)
{
	*out = nullptr;
	if (digest ? !c || flags || !block_size_ok(block_size) : !create_args_ok(c, format, block_size, flags)) { return MSCOMP_ARG_ERROR; }
	if (!count_ok(n_res) || !count_ok(n_blocks_table) || !count_ok(n_units) || !count_ok(n_cand_max)) { return MSCOMP_ARG_ERROR; }
	if (in_total_max >> 50 || !count_ok(in_total_max / SYNC_TILE + n_units)) { return MSCOMP_MEM_ERROR; }   // (the tiles are numbered in 32 bits; checked before the context is used)
	std::unique_ptr<mscomp_amd_syncer> y(new (std::nothrow) mscomp_amd_syncer());
	MSCompStatus st = MSCOMP_OK;
	if (!digest) {
		st = access_create(y.get(), nullptr, c, format, block_size, n_res, n_blocks_table, (size_t)n_cand_max, n_cand_max, flags);
		if (st != MSCOMP_OK) { return st; }
	}
	DeviceGuard g(c->device);
	if (!g.ok) { st = MSCOMP_ERRNO; }
	if (digest) {                                                          // the bounds of BlockAccess, and nothing else of it
		if (!y) { return MSCOMP_MEM_ERROR; }
		y->ctx = c; y->shift = (uint32_t)__builtin_ctz(block_size); y->n_res = (uint32_t)n_res; y->nbt = (uint32_t)n_blocks_table;
		y->n_req = y->m = (uint32_t)n_cand_max; y->digest = true;
	}
	y->n_units = (uint32_t)n_units; y->in_total_max = in_total_max; y->run.never = false;
	if (st == MSCOMP_OK && !y->stab.reserve(sync_tab(y->s, nullptr, n_res, n_blocks_table, n_units, n_cand_max, in_total_max) + 64)) { (void)hipGetLastError(); st = MSCOMP_MEM_ERROR; }
	if (st == MSCOMP_OK && digest && !y->dtab.reserve(sync_digest_tab(y.get(), nullptr, n_cand_max, y->shift) + 64)) { (void)hipGetLastError(); st = MSCOMP_MEM_ERROR; }
	if (st == MSCOMP_OK) {
		sync_tab(y->s, y->stab.p, n_res, n_blocks_table, n_units, n_cand_max, in_total_max);
		if (digest) { sync_digest_tab(y.get(), y->dtab.p, n_cand_max, y->shift); }
		uint32_t consts[SYNC_CONSTS];
		sync_host_consts(y->shift, consts);
		if (hipMemset(y->s.count, 0, 64) != hipSuccess || hipMemcpy(y->s.consts, consts, sizeof consts, hipMemcpyHostToDevice) != hipSuccess) { (void)hipGetLastError(); st = MSCOMP_ERRNO; }
	}
	if (st != MSCOMP_OK) { y->in.destroy(); y->tab.release(); y->stab.release(); y->dtab.release(); return st; }
	*out = y.release();
	return MSCOMP_OK;
}

MSCompStatus mscomp_amd_syncer_create(mscomp_amd_ctx* c, MSCompFormat format, uint32_t block_size, size_t n_res, uint64_t n_blocks_table, size_t n_units,
                                      uint64_t in_total_max, uint64_t n_cand_max, uint32_t flags, mscomp_amd_syncer** out)
{
	if (!out) { return MSCOMP_ARG_ERROR; }
	return syncer_create(c, false, format, block_size, n_res, n_blocks_table, n_units, in_total_max, n_cand_max, flags, out);
}

MSCompStatus mscomp_amd_syncer_create_digest(mscomp_amd_ctx* c, uint32_t block_size, size_t n_res, uint64_t n_blocks_table, size_t n_units, uint64_t in_total_max,
                                             uint64_t n_cand_max, uint32_t flags, mscomp_amd_syncer** out)
{
	if (!out) { return MSCOMP_ARG_ERROR; }
	return syncer_create(c, true, MSCOMP_NONE, block_size, n_res, n_blocks_table, n_units, in_total_max, n_cand_max, flags, out);
}

void mscomp_amd_syncer_destroy(mscomp_amd_syncer* y) { destroy_object(y, [y] { y->in.destroy(); y->tab.release(); y->stab.release(); y->dtab.release(); }); }

// The call: the store's table and bitmap, the units' numberings, the boundary registers, the scan -- tile pass, tile
// scan, runs pass --, the kept candidates' rows through the reader core, the compare, the greedy selection with the lists.
// Both calls; `digest`: which of them. With it, rule 6 is the digest of the window against d_block_digest, the store's
// bytes are never dereferenced -- its view is packed without them -- and the reader core's passes are left out.
static MSCompStatus syncer_run(mscomp_amd_syncer* y, bool digest, const mscomp_amd_blocks_view* store, const uint32_t* d_block_digest, const uint8_t* d_in,
                               const uint64_t* d_in_off, const uint64_t* d_in_len, uint64_t* d_hit_first, uint64_t* d_req, uint64_t* d_req_off, uint64_t* d_lit_first,
                               uint64_t* d_lit, uint64_t* d_count, int32_t* d_res_status, int32_t* d_status)
{
	if (!y || !store || !d_hit_first || !d_lit_first || !d_count || y->digest != digest) { return MSCOMP_ARG_ERROR; }
	if (y->n_units && (!d_in_off || !d_in_len || !d_status || !d_lit)) { return MSCOMP_ARG_ERROR; }
	if ((y->in_total_max && !d_in) || (y->m && (!d_req || !d_req_off)) || (y->n_res && !d_res_status)) { return MSCOMP_ARG_ERROR; }
	SpliceView v[1];
	bool with_crc = false;
	mscomp_amd_blocks_view sv = *store;
	if (digest) { sv.d_packed = nullptr; sv.packed_len = 0; }                 // (the rows are still judged against store->packed_len, below)
	if (!pack_views(&sv, 1, true, v, with_crc) || !with_crc) { return MSCOMP_ARG_ERROR; }   // the checksums are the signature: required
	if (digest) { v[0].packed_len = store->packed_len; }
	if (store->n_res > y->n_res || store->n_blocks_table > y->nbt || (digest && y->nbt && !d_block_digest)) { return MSCOMP_ARG_ERROR; }
	mscomp_amd_ctx* c = y->ctx;
	DeviceGuard g(c->device);
	if (!g.ok) { return MSCOMP_ERRNO; }
	y->in.mark_ran(); y->ran = true;
	const void* args[20];
	view_args(args, v, { d_in, d_in_off, d_in_len, d_hit_first, d_req, d_req_off, d_lit_first, d_lit, d_count, d_res_status, d_status,
	                     static_cast<const void*>(d_block_digest) });
	const uint32_t n = (uint32_t)store->n_res;
	return plan_run(y->run, c, args, [&] {
		const SyncTab& t = y->s;
		SpliceSrc src{};
		src.v[0] = v[0];
		{ KernelTimer k(c, "sy_clear_kernel"); launch_sync_clear(c->stream, t, c->crc_blocks); }
		{ KernelTimer k(c, "sy_seed_kernel"); launch_sync_seed(c->stream, v[0], n, y->shift, t, d_res_status); }
		if (y->nbt && n) {
			{ KernelTimer k(c, "dd_rows_kernel"); launch_dedup_rule3(c->stream, src, n, y->nbt, t.ufirst, d_res_status, c->crc_blocks); }
			{ KernelTimer k(c, "sy_keys_kernel"); launch_sync_keys(c->stream, v[0], n, y->nbt, y->shift, t, d_res_status, c->crc_blocks); }
		}
		{ KernelTimer k(c, "sy_units_kernel"); launch_sync_units(c->stream, y->n_units, y->shift, y->in_total_max, d_in_off, d_in_len, t, d_status); }
		{ KernelTimer k(c, "sy_bounds"); launch_sync_bounds(c->stream, y->n_units, d_in, t, c->crc_blocks); }
		{ KernelTimer k(c, "sy_scan"); launch_sync_scan(c->stream, y->n_units, y->m, y->shift, d_in, t, c->crc_blocks); }
		if (y->m && !digest) {
			{ KernelTimer k(c, "sy_req_kernel"); launch_sync_requests(c->stream, n, y->m, y->shift, t); }
			access_admit(y, v[0].packed, v[0].packed_len, v[0].first, v[0].off, v[0].res_len, t.req, nullptr);
			access_decode(y, v[0].packed, v[0].crc, t.qlen, t.qstat);
			{ KernelTimer k(c, "sy_confirm_kernel"); launch_sync_confirm(c->stream, y->m, y->shift, d_in, t, y->t, c->cpd_blocks); }
		} else if (y->m) {
			{ KernelTimer k(c, "sy_req_kernel"); launch_sync_requests(c->stream, n, y->m, y->shift, t); }
			{ KernelTimer k(c, "sy_dunits_kernel"); launch_sync_digest_units(c->stream, n, y->m, y->shift, t, y->doff, y->dlen); }
			{ KernelTimer k(c, "dg_leaf_kernel"); launch_digest_leaves(c->stream, d_in, y->d, c->crc_blocks); }
			{ KernelTimer k(c, "dg_root_kernel"); launch_digest_roots(c->stream, y->d, y->d.out, 0, nullptr, nullptr); }
			{ KernelTimer k(c, "sy_dcompare_kernel"); launch_sync_digest_compare(c->stream, v[0], n, y->m, d_block_digest, t, y->d.out); }
		}
		// (count[7]: the reader core's count of owners; a digest syncer hashes every kept window once, so the low word of count[2])
		const uint32_t* distinct = !y->m ? nullptr : digest ? reinterpret_cast<const uint32_t*>(t.count + 2) : y->t.cnt;
		{ KernelTimer k(c, "sy_select_kernel"); launch_sync_select(c->stream, y->n_units, y->shift, t, d_status, distinct, d_hit_first, d_req, d_req_off,
		                                                         d_lit_first, d_lit, d_count); }
	});
}

MSCompStatus mscomp_amd_syncer_sync(mscomp_amd_syncer* y, const mscomp_amd_blocks_view* store, const uint8_t* d_in, const uint64_t* d_in_off, const uint64_t* d_in_len,
                                    uint64_t* d_hit_first, uint64_t* d_req, uint64_t* d_req_off, uint64_t* d_lit_first, uint64_t* d_lit, uint64_t* d_count,
                                    int32_t* d_res_status, int32_t* d_status)
{
	return syncer_run(y, false, store, nullptr, d_in, d_in_off, d_in_len, d_hit_first, d_req, d_req_off, d_lit_first, d_lit, d_count, d_res_status, d_status);
}

MSCompStatus mscomp_amd_syncer_sync_digest(mscomp_amd_syncer* y, const mscomp_amd_blocks_view* store, const uint32_t* d_block_digest, const uint8_t* d_in,
                                           const uint64_t* d_in_off, const uint64_t* d_in_len, uint64_t* d_hit_first, uint64_t* d_req, uint64_t* d_req_off,
                                           uint64_t* d_lit_first, uint64_t* d_lit, uint64_t* d_count, int32_t* d_res_status, int32_t* d_status)
{
	return syncer_run(y, true, store, d_block_digest, d_in, d_in_off, d_in_len, d_hit_first, d_req, d_req_off, d_lit_first, d_lit, d_count, d_res_status, d_status);
}

// kept candidates, distinct rows decoded or read, and hits of y's last execution (read back; none before the first)
int mscomp_amd_syncer_counts(mscomp_amd_syncer* y, uint32_t out[3])
{
	if (!y || !out) { return -1; }
	DeviceGuard g(y->ctx->device);
	if (!g.ok || hipStreamSynchronize(y->ctx->stream) != hipSuccess) { return -1; }
	out[0] = out[1] = out[2] = 0;
	if (!y->ran) { return 0; }
	uint64_t cnt[8] = {};
	if (hipMemcpy(cnt, y->s.count, sizeof cnt, hipMemcpyDeviceToHost) != hipSuccess) { return -1; }
	out[0] = (uint32_t)cnt[2]; out[1] = (uint32_t)cnt[7]; out[2] = (uint32_t)cnt[4];
	return 0;
}

// ---- block digesters (include/mscomp_amd.h; kernels: digest.hip, the table passes in blocks.hip) ----
// A digester writes and checks the digest column of a container's blocks, as mscomp_amd_blocks_crc and _check write and check the CRC
// column, with the container's table passes over tables of its own: the columns of BlocksTab those passes touch, a leaf digest per
// possible leaf and -- for check -- a digest per possible block. No inner plan, no staging area.
#pragma GCC visibility push(hidden)
struct mscomp_amd_digester {
	mscomp_amd_ctx* ctx = nullptr;
	uint32_t shift = 0, n_res = 0, n_blocks = 0;       // block_size = 1 << shift; n_blocks = n_blocks_max
	uint64_t in_total_max = 0;
	GraphRun<5> brun; GraphRun<8> krun;                // blocks, check
	DevBuf tab;                                        // digest_tab
	BlocksTab t{};                                     // (the columns the inner plans, compress and decompress alone use stay null)
	DigestTab d{};
};
#pragma GCC visibility pop

// the columns of a digester's tables from `base` on (n resources, m blocks at most), the 16-byte columns first; returns where they end
static uintptr_t digest_tab(mscomp_amd_digester* g, void* base, size_t n, size_t m)
{
	Carve k(base);
	BlocksTab& t = g->t;
	g->d.leaf = k.w(4 * (m << (g->shift - DG_LEAF_SHIFT))); g->d.out = k.w(4 * m);
	t.res_a = k.q(n); t.res_b = k.q(n); t.unit_first = k.q(n + 1);
	t.in_off = k.q(m); t.in_len = k.q(m); t.out_off = k.q(m); t.out_cap = k.q(m); t.ulen = k.q(m);
	t.rstat = k.i(n);
	g->d.off = t.in_off; g->d.len = t.in_len; g->d.count = t.unit_first + n; g->d.n_max = (uint32_t)m; g->d.shift = g->shift;
	return k.at;
}

MSCompStatus mscomp_amd_digester_create(mscomp_amd_ctx* c, uint32_t block_size, size_t n_res, uint64_t in_total_max, uint32_t flags, mscomp_amd_digester** out)
{
	if (!out) { return MSCOMP_ARG_ERROR; }
	*out = nullptr;
	if (!c || flags || !block_size_ok(block_size) || !count_ok(n_res)) { return MSCOMP_ARG_ERROR; }
	if (in_total_max >> 50 || in_total_max / block_size > 0x7FFFFFF0ull - n_res) { return MSCOMP_MEM_ERROR; }   // (checked before the context is used)
	const uint64_t M = n_res + in_total_max / block_size;
	DeviceGuard g(c->device);
	if (!g.ok) { return MSCOMP_ERRNO; }
	std::unique_ptr<mscomp_amd_digester> d(new (std::nothrow) mscomp_amd_digester());
	if (!d) { return MSCOMP_MEM_ERROR; }
	d->ctx = c; d->shift = (uint32_t)__builtin_ctz(block_size); d->n_res = (uint32_t)n_res; d->n_blocks = (uint32_t)M; d->in_total_max = in_total_max;
	d->brun.never = d->krun.never = n_res == 0;
	if (!d->tab.reserve(digest_tab(d.get(), nullptr, n_res, M) + 64)) { (void)hipGetLastError(); return MSCOMP_MEM_ERROR; }
	digest_tab(d.get(), d->tab.p, n_res, M);
	*out = d.release();
	return MSCOMP_OK;
}

void mscomp_amd_digester_destroy(mscomp_amd_digester* d) { destroy_object(d, [d] { d->tab.release(); }); }

// blocks: the container's compress tables (t.unit_first = block_first, t.in_off / t.in_len = the blocks, t.rstat), the leaves, the roots
// straight into the caller's column, with the statuses. check: the container's check tables (t.unit_first / t.res_b = units and first
// block of the clipped ranges, t.in_off / t.in_len = the blocks in d_out, t.ulen = their entry of d_block_digest), the leaves, the roots
// into d.out, the fold.
MSCompStatus mscomp_amd_digester_blocks(mscomp_amd_digester* d, const uint8_t* d_data, const uint64_t* d_res_off, const uint64_t* d_res_len, uint32_t* d_block_digest,
                                        int32_t* d_status)
{
	if (!d || (d->n_blocks && !d_block_digest) || (d->n_res && (!d_res_off || !d_res_len || !d_status))) { return MSCOMP_ARG_ERROR; }
	if (d->in_total_max && !d_data) { return MSCOMP_ARG_ERROR; }
	if (d->n_res == 0) { return MSCOMP_OK; }               // (no resource, no block: n_blocks_max is 0 too)
	mscomp_amd_ctx* c = d->ctx;
	DeviceGuard g(c->device);
	if (!g.ok) { return MSCOMP_ERRNO; }
	const void* args[5] = { d_data, d_res_off, d_res_len, d_block_digest, d_status };
	return plan_run(d->brun, c, args, [&] {
		const BlocksTab& t = d->t;
		{ KernelTimer k(c, "bk_ctables"); launch_blocks_ctables(c->stream, d->n_res, d->n_blocks, d->shift, d->in_total_max, d_res_off, d_res_len, t.unit_first, t); }
		{ KernelTimer k(c, "dg_leaf_kernel"); launch_digest_leaves(c->stream, d_data, d->d, c->crc_blocks); }
		{ KernelTimer k(c, "dg_root_kernel"); launch_digest_roots(c->stream, d->d, d_block_digest, d->n_res, t.rstat, d_status); }
	});
}

MSCompStatus mscomp_amd_digester_check(mscomp_amd_digester* d, const uint8_t* d_out, const uint64_t* d_out_off, const uint64_t* d_res_len, const uint64_t* d_block_first,
                                       const uint64_t* d_range, const uint32_t* d_block_digest, uint64_t* d_out_len, int32_t* d_status)
{
	if (!d || !d_block_first || (d->n_blocks && !d_block_digest) || (d->n_res && (!d_out_off || !d_res_len || !d_out_len || !d_status))) { return MSCOMP_ARG_ERROR; }
	if (d->in_total_max && !d_out) { return MSCOMP_ARG_ERROR; }
	if (d->n_res == 0) { return MSCOMP_OK; }
	mscomp_amd_ctx* c = d->ctx;
	DeviceGuard g(c->device);
	if (!g.ok) { return MSCOMP_ERRNO; }
	const void* args[8] = { d_out, d_out_off, d_res_len, d_block_first, d_range, d_block_digest, d_out_len, d_status };
	return plan_run(d->krun, c, args, [&] {
		const BlocksTab& t = d->t;
		{ KernelTimer k(c, "bk_ktables"); launch_blocks_ktables(c->stream, d->n_res, d->n_blocks, d->shift, d->in_total_max, d_res_len, d_block_first, d_range, d_out_off, d_status, t); }
		{ KernelTimer k(c, "dg_leaf_kernel"); launch_digest_leaves(c->stream, d_out, d->d, c->crc_blocks); }
		{ KernelTimer k(c, "dg_root_kernel"); launch_digest_roots(c->stream, d->d, d->d.out, 0, nullptr, nullptr); }
		{ KernelTimer k(c, "dg_kfold_kernel"); launch_blocks_kfold(c->stream, d->n_res, d->d.out, d_block_digest, 4, t, d_out_len, d_status); }
	});
}

// ---- parity rows (include/mscomp_amd.h; kernels: parity.hip, the CRC unit kernels of crc32.hip) ----
// A parity object holds the table words of both calls and nothing else: no inner plan, no cache, no staging area -- the digester's shape.
#pragma GCC visibility push(hidden)
struct mscomp_amd_parity {
	mscomp_amd_ctx* ctx = nullptr;
	uint32_t block_size = 0;
	GraphRun<15> brun; GraphRun<21> rrun;              // build, rebuild: the view, then the rest
	DevBuf tab;                                        // parity_tab
	ParityTab t{};
};
#pragma GCC visibility pop

// the columns of a parity object's tables from `base` on (t.nbt, t.gmax, t.m set); returns where they end
static uintptr_t parity_tab(ParityTab& t, void* base)
{
	Carve k(base);
	const size_t Q = (size_t)t.gmax * t.m;
	t.plen = k.q(Q); t.clen = k.q(Q); t.cum = k.q(Q + 1); t.fixlen = k.q(t.nbt); t.count = k.q(8);
	t.pcrc = k.w(Q); t.rflag = k.w(t.nbt); t.grec = k.w(6 * (size_t)t.gmax); k.pad8();
	return k.at;
}

MSCompStatus mscomp_amd_parity_create(mscomp_amd_ctx* c, uint32_t block_size, uint64_t n_blocks_table, uint32_t k, uint32_t m, uint32_t flags, mscomp_amd_parity** out)
{
	if (!out) { return MSCOMP_ARG_ERROR; }
	*out = nullptr;
	if (!c || flags || !block_size_ok(block_size) || k < 1u || k > MSCOMP_AMD_PARITY_K_MAX || m < 1u || m > MSCOMP_AMD_PARITY_M_MAX || !count_ok(n_blocks_table)) { return MSCOMP_ARG_ERROR; }
	const uint64_t gmax = (n_blocks_table + k - 1u) / k;
	if (!count_ok(gmax * m)) { return MSCOMP_MEM_ERROR; }                  // (checked before the context is used: the parity rows are CRC units, counted in 32 bits)
	DeviceGuard g(c->device);
	if (!g.ok) { return MSCOMP_ERRNO; }
	std::unique_ptr<mscomp_amd_parity> pr(new (std::nothrow) mscomp_amd_parity());
	if (!pr) { return MSCOMP_MEM_ERROR; }
	pr->ctx = c; pr->block_size = block_size;
	ParityTab& t = pr->t;
	t.nbt = (uint32_t)n_blocks_table; t.gmax = (uint32_t)gmax; t.k = k; t.m = m; t.shift = (uint32_t)__builtin_ctz(block_size);
	if (!pr->tab.reserve(parity_tab(t, nullptr) + 64)) { (void)hipGetLastError(); return MSCOMP_MEM_ERROR; }
	parity_tab(t, pr->tab.p);
	*out = pr.release();
	return MSCOMP_OK;
}

void mscomp_amd_parity_destroy(mscomp_amd_parity* pr) { destroy_object(pr, [pr] { pr->tab.release(); }); }

int mscomp_amd_parity_bound(const mscomp_amd_parity* pr, uint64_t out[2])
{
	if (!pr || !out) { return -1; }
	out[0] = (uint64_t)pr->t.gmax * pr->t.m; out[1] = out[0] * pr->block_size;
	return 0;
}

// The CRC-32 of the parity rows into t.pcrc, t.clen bytes of each: crc_pass with the parity scan for its table pass (a unit table of
// lengths alone needs none of that pass's bounds checks, and the scan takes an eighth of its serial steps)
static void parity_crc(mscomp_amd_ctx* c, const ParityTab& t, uint32_t Q, const uint8_t* par, const u64* par_off)
{
	{ KernelTimer k(c, "pa_scan_kernel"); launch_parity_scan(c->stream, Q, t.clen, t.cum); }
	{ KernelTimer k(c, "crc_seed_kernel"); launch_crc_seeds(c->stream, Q, t.cum, t.pcrc, nullptr, nullptr); }
	{ KernelTimer k(c, "crc_kernel"); launch_crc_units(c->stream, Q, par, par_off, t.cum, t.pcrc, nullptr, nullptr, nullptr, c->crc_blocks); }
}

// what both calls ask of their view: one pack_views takes, and MSCOMP_ARG_ERROR otherwise; `mis`: rule 0's half that the host knows
static bool parity_view(const mscomp_amd_parity* pr, const mscomp_amd_blocks_view* src, SpliceView& v, bool& mis)
{
	bool with_crc = false;
	if (!src || !pack_views(src, 1, false, &v, with_crc)) { return false; }
	mis = src->n_blocks_table != pr->t.nbt;
	return true;
}

MSCompStatus mscomp_amd_parity_build(mscomp_amd_parity* pr, const mscomp_amd_blocks_view* src, uint8_t* d_par, uint64_t par_cap, uint64_t* d_par_off, uint32_t* d_par_crc,
                                     uint32_t* d_row_len, uint64_t* d_par_head, int32_t* d_status)
{
	SpliceView v; bool mis = false;
	if (!pr || !d_par_head || !d_status || !parity_view(pr, src, v, mis)) { return MSCOMP_ARG_ERROR; }
	const ParityTab& t = pr->t;
	const uint32_t Q = t.gmax * t.m;
	if (t.nbt && (!d_par_off || !d_par_crc || !d_row_len || (par_cap && !d_par) || (reinterpret_cast<uintptr_t>(d_par) & 15u))) { return MSCOMP_ARG_ERROR; }
	mscomp_amd_ctx* c = pr->ctx;
	DeviceGuard g(c->device);
	if (!g.ok) { return MSCOMP_ERRNO; }
	const void* args[15];
	view_args(args, &v, { static_cast<const void*>(d_par), reinterpret_cast<const void*>(static_cast<uintptr_t>(par_cap)), static_cast<const void*>(d_par_off),
	                      static_cast<const void*>(d_par_crc), static_cast<const void*>(d_row_len), static_cast<const void*>(d_par_head), static_cast<const void*>(d_status) });
	return plan_run(pr->brun, c, args, [&] {
		if (t.nbt) {
			{ KernelTimer k(c, "pa_rows_kernel"); launch_parity_rows(c->stream, v, t, mis, d_row_len, c->crc_blocks); }
			{ KernelTimer k(c, "pa_groups_kernel"); launch_parity_groups(c->stream, v, t, mis, d_row_len, nullptr, c->crc_blocks); }
			{ KernelTimer k(c, "pa_scan_kernel"); launch_parity_scan(c->stream, Q, t.plen, d_par_off); }
			{ KernelTimer k(c, "pa_units_kernel"); launch_parity_units(c->stream, t, d_par_off, par_cap, c->crc_blocks); }
			{ KernelTimer k(c, "pa_build_kernel"); launch_parity_build(c->stream, v, t, mis, d_row_len, d_par, par_cap, d_par_off, c->crc_blocks); }
			parity_crc(c, t, Q, d_par, d_par_off);
		}
		{ KernelTimer k(c, "pa_head_kernel"); launch_parity_head(c->stream, v, t, mis, d_par_off, par_cap, d_par_crc, d_par_head, d_status, c->crc_blocks); }
	});
}

MSCompStatus mscomp_amd_parity_rebuild(mscomp_amd_parity* pr, const mscomp_amd_blocks_view* src, const uint32_t* d_verdict, const uint8_t* d_par, uint64_t par_len,
                                       const uint64_t* d_par_off, const uint32_t* d_par_crc, const uint32_t* d_row_len, const uint64_t* d_par_head, uint8_t* d_fix_packed,
                                       uint64_t fix_cap, uint64_t* d_fix_block_off, uint32_t* d_fix_verdict, uint64_t* d_count, int32_t* d_status)
{
	SpliceView v; bool mis = false;
	if (!pr || !d_par_head || !d_count || !d_status || !parity_view(pr, src, v, mis)) { return MSCOMP_ARG_ERROR; }
	const ParityTab& t = pr->t;
	const uint32_t Q = t.gmax * t.m;
	if (t.nbt && (!d_verdict || !d_par_off || !d_par_crc || !d_row_len || !d_fix_block_off || !d_fix_verdict || (par_len && !d_par) || (fix_cap && !d_fix_packed) ||
	              (reinterpret_cast<uintptr_t>(d_par) & 15u))) { return MSCOMP_ARG_ERROR; }
	mscomp_amd_ctx* c = pr->ctx;
	DeviceGuard g(c->device);
	if (!g.ok) { return MSCOMP_ERRNO; }
	const void* args[21];
	view_args(args, &v, { static_cast<const void*>(d_verdict), static_cast<const void*>(d_par), reinterpret_cast<const void*>(static_cast<uintptr_t>(par_len)),
	                      static_cast<const void*>(d_par_off), static_cast<const void*>(d_par_crc), static_cast<const void*>(d_row_len), static_cast<const void*>(d_par_head),
	                      static_cast<const void*>(d_fix_packed), reinterpret_cast<const void*>(static_cast<uintptr_t>(fix_cap)), static_cast<const void*>(d_fix_block_off),
	                      static_cast<const void*>(d_fix_verdict), static_cast<const void*>(d_count), static_cast<const void*>(d_status) });
	return plan_run(pr->rrun, c, args, [&] {
		if (t.nbt) { KernelTimer k(c, "pa_groups_kernel"); launch_parity_groups(c->stream, v, t, mis, d_row_len, d_par_head, c->crc_blocks); }
		{ KernelTimer k(c, "pa_check_kernel"); launch_parity_check(c->stream, t, d_par_off, par_len, c->crc_blocks); }
		if (t.nbt) {
			parity_crc(c, t, Q, d_par, d_par_off);
			{ KernelTimer k(c, "pa_damage_kernel"); launch_parity_damage(c->stream, v, t, mis, d_verdict, d_par_off, par_len, d_par_crc, d_row_len, d_par_head, c->crc_blocks); }
			{ KernelTimer k(c, "pa_scan_kernel"); launch_parity_scan(c->stream, t.nbt, t.fixlen, d_fix_block_off); }
			{ KernelTimer k(c, "pa_solve_kernel"); launch_parity_solve(c->stream, v, t, mis, d_par, d_par_off, d_row_len, d_par_head, d_fix_packed, fix_cap, d_fix_block_off, c->crc_blocks); }
		}
		{ KernelTimer k(c, "pa_tail_kernel"); launch_parity_tail(c->stream, v, t, mis, d_par_head, fix_cap, d_fix_block_off, d_fix_verdict, d_count, d_status, c->crc_blocks); }
	});
}

// ---- the scratch hooks' view of the objects above (hooks.hip: mscomp_amd_debug_scratch_*) ----
extern "C++" mscomp_amd_ctx* msc::scratch_of_object(int kind, void* obj, std::vector<ScratchEnt>& v)
{
	const auto access = [&v](BlockAccess* a) { v.push_back(ScratchEnt{ "tab", &a->tab, false }); v.push_back(ScratchEnt{ "cache", &a->in.cache, false }); scratch_of_plan(a->in.dplan, 2, v); };
	switch (kind) {
	case MSCOMP_AMD_SCRATCH_BLOCKS: {
		mscomp_amd_blocks* b = static_cast<mscomp_amd_blocks*>(obj);
		v.push_back(ScratchEnt{ "tab", &b->tab, false }); v.push_back(ScratchEnt{ "stage", &b->in.stage, false });
		scratch_of_plan(b->in.cplan, 1, v); scratch_of_plan(b->in.dplan, 2, v);
		return b->ctx;
	}
	case MSCOMP_AMD_SCRATCH_READER: { mscomp_amd_reader* r = static_cast<mscomp_amd_reader*>(obj); access(r); return r->ctx; }
	case MSCOMP_AMD_SCRATCH_WRITER: {
		mscomp_amd_writer* w = static_cast<mscomp_amd_writer*>(obj);
		access(w); v.push_back(ScratchEnt{ "stage", &w->in.stage, false }); scratch_of_plan(w->in.cplan, 1, v);
		return w->ctx;
	}
	case MSCOMP_AMD_SCRATCH_SPLICER: { mscomp_amd_splicer* s = static_cast<mscomp_amd_splicer*>(obj); v.push_back(ScratchEnt{ "addr", &s->addr, false }); return s->ctx; }
	case MSCOMP_AMD_SCRATCH_DEDUPER: { mscomp_amd_deduper* d = static_cast<mscomp_amd_deduper*>(obj); v.push_back(ScratchEnt{ "tab", &d->tab, false }); return d->ctx; }
	default: return nullptr;
	}
}

// ---- resource CRCs from block CRCs (include/mscomp_amd.h; kernels: crc32.hip) ----
MSCompStatus mscomp_amd_res_crc_dev(mscomp_amd_ctx* c, uint32_t block_size, size_t n_res, uint64_t n_blocks_table, const uint64_t* d_block_first,
                                    const uint64_t* d_res_len, const uint32_t* d_block_crc, uint32_t* d_res_crc, int32_t* d_status)
{
	if (!c || !block_size_ok(block_size) || !count_ok(n_res) || !count_ok(n_blocks_table)) { return MSCOMP_ARG_ERROR; }
	if (n_res && (!d_block_first || !d_res_len || !d_block_crc || !d_res_crc || !d_status)) { return MSCOMP_ARG_ERROR; }
	if (n_res == 0) { return MSCOMP_OK; }                  // (nothing to report on)
	DeviceGuard g(c->device);
	if (!g.ok) { return MSCOMP_ERRNO; }
	{ KernelTimer k(c, "res_crc"); launch_res_crc(c->stream, (uint32_t)n_res, (uint32_t)n_blocks_table, (uint32_t)__builtin_ctz(block_size), d_block_first, d_res_len,
	                                              d_block_crc, d_res_crc, d_status, c->crc_blocks); }
	return hipGetLastError() == hipSuccess ? MSCOMP_OK : MSCOMP_ERRNO;
}
