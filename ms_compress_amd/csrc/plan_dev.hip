// plan_dev.hip -- plans with device tables (include/mscomp_amd.h): created from bounds, tables built on the device by every execution; CRC
// plans, capacity layout and compaction from device tables. Host code only: the table kernels are devplan.hip's, the launches launch.hip's.
// The plan holds its bounds and scratch sized for them; p->tables holds what the table pass (devplan.hip) writes each time (tables_layout).
#include "host.h"

using namespace msc;

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
		const uint64_t nb = N < I / XPS_MIN_IN ? N : I / XPS_MIN_IN, sg = I / env_xps_seg() + nb;
		if (nb && sg < 0x7FFFFFF0ull && !reserve_xps(p, nb, sg)) { return false; }
	}
	if (p->sizing) { return true; }
	const uint64_t B = N < O / LZG_MIN_CAP ? N : O / LZG_MIN_CAP;
	if (B && O < (1ull << 60)) {
		const uint64_t wd = O + 64 * B, tl = (O >> LZG_TILE_SHIFT) + B, tb = toks / 8192 + B;
		const uint64_t budget = optional_scratch_budget(env_lzg_budget(), c->lzg_words.cap);
		if (wd <= budget / 4 && tb < 0x7FFFFFF0ull && tl < 0x7FFFFFF0ull) { (void)reserve_lzg(p, B, tb, tl, wd); }
	}
	if (p->format == MSCOMP_XPRESS_HUFF) {
		const uint64_t S = N < O / 65537u ? N : O / 65537u;
		const uint64_t by_out = O / 65536u + 2 * S, by_len = I / 260u + S, most = by_out < by_len ? by_out : by_len, scr = most + most / 4 + 2 * S;
		const uint64_t budget = optional_scratch_budget(env_xhc_scr_budget(), c->dz_scr.cap);
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
bool msc::decode_dev_counts(MSCompFormat format, uint64_t N, uint64_t in_total_max, uint64_t O, bool sizing, uint64_t& I, uint64_t& chunks, uint64_t& toks, uint64_t& cands)
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
	if (!creator_args(c, n_units, known_format(format), out) || (flags & ~MSCOMP_AMD_DEV_LARGE_UNITS)) { return MSCOMP_ARG_ERROR; }
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

extern "C" {

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
	if (!creator_args(c, n_units, known_format(format), out) || in_unit_max == 0 || in_unit_max > 0xFFFFF000ull) { return MSCOMP_ARG_ERROR; }
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
	if (!creator_args(c, n_units, true, out) || in_total_max >= (1ull << 50)) { return MSCOMP_ARG_ERROR; }   // (distances to a unit's end stay below 2^50: crc32.hip crc_xpow)
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

} // extern "C"
