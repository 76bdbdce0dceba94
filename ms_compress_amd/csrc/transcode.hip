// transcode.hip -- the table passes of a block transcoder (mscomp_amd_transcoder_*, include/mscomp_amd.h): a block container brought to
// another block size or codec. The two big stages are a decompress and a compress dev plan over the blocks of the WORKED groups as units
// (blockobj.hip runs them between these passes, unchanged), the checksums are the CRC kernels' (crc32.hip), and every byte of the new
// container is moved by the one move kernel (blocks.hip). What is new here decides what needs no work at all: an LZNT1 block is the plain
// concatenation of its 4 KiB chunks' images, so an LZNT1 container cut at another size is mostly its old bytes under new tables.
// DESIGN.md 4.17.
#include "kernels.h"

namespace msc {

#define TC_ROW_NONE   0u                                  // a p-row of a group that failed its table checks
#define TC_ROW_CARRY  1u                                  // stored bytes taken from the old container as they lie
#define TC_ROW_ENCODE 2u                                  // encoded from the group's data (stored raw when that does not shrink it)
#define TC_ROW_RAW    3u                                  // a split's new block whose images do not shrink it: stored raw from the decoded source block
#define TC_ACT_COPY   1u                                  // a decode unit's action word (kind | data length << 2): a raw member, copied into the cache
#define TC_ACT_DECODE 2u                                  // ... a member decoded into the cache
#define TC_PIECE_SHIFT 14u                                // the gather moves its bytes in pieces of 16 KiB

__device__ __forceinline__ u64 tc_ceil(u64 L, uint32_t shift) { return (L >> shift) + ((L & (((u64)1 << shift) - 1u)) != 0 ? 1u : 0u); }
__device__ __forceinline__ u64 tc_min(u64 a, u64 b) { return a < b ? a : b; }

// ---- rules 0-2 ----
// One block. Rule 0 over the whole table first; then the resources in tiles of 1024: the block count against ceil(L / B1), the running
// total of ceil(L / B2) against the new table, and -- over the resources that passed -- the numbering of their groups and of their p-rows.
// The slots and the counts of the last execution are cleared here, whatever the verdict: the unit passes write empty units for free slots.
__global__ __launch_bounds__(DV_THREADS) void tc_res_kernel(TcDims d, const u64* __restrict__ block_first, const u64* __restrict__ res_len,
                                                           u64* __restrict__ gfirst, u64* __restrict__ pfirst, int32_t* __restrict__ rstat,
                                                           uint32_t* __restrict__ slot_group, uint32_t* __restrict__ cnt)
{
	__shared__ u64 s_w[2][DV_WAVES];
	const uint32_t tid = threadIdx.x;
	bool bad = tid == 0 && block_first[d.n_res] > d.nbt;
	for (uint32_t i = tid; i < d.n_res; i += DV_THREADS) { bad = bad || block_first[i] > block_first[i + 1u]; }
	const bool refused = __syncthreads_or(bad ? 1 : 0) != 0;
	for (uint32_t i = tid; i < d.gmax; i += DV_THREADS) { slot_group[i] = 0; }
	if (tid == 0) { cnt[0] = cnt[1] = cnt[2] = 0; cnt[3] = refused ? 1u : 0u; gfirst[0] = 0; pfirst[0] = 0; }
	if (refused) {
		for (uint32_t i = tid; i < d.n_res; i += DV_THREADS) { rstat[i] = -2; gfirst[i + 1u] = 0; pfirst[i + 1u] = 0; }   // MSCOMP_ARG_ERROR
		return;
	}
	u64 run[1] = {0}, acc[2] = {0, 0};
	for (uint32_t base = 0; base < d.n_res; base += DV_THREADS) {
		const uint32_t i = base + tid;
		const bool live = i < d.n_res;
		const u64 L = live ? res_len[i] : 0, nb2 = tc_ceil(L, d.s2);
		int32_t st = 0;
		if (live && block_first[i + 1u] - block_first[i] != tc_ceil(L, d.s1)) { st = -3; }   // MSCOMP_DATA_ERROR
		u64 r[1] = {nb2};
		dv_block_scan<1>(r, run, s_w);                                   // the running total up to and including resource i (saturating)
		if (live && st == 0 && r[0] > d.nbn) { st = -2; }
		const bool pass = live && st == 0;
		u64 c[2] = {pass ? tc_ceil(L, d.sg) : 0, pass ? nb2 : 0};
		dv_block_scan<2>(c, acc, s_w);
		if (live) { gfirst[i + 1u] = c[0]; pfirst[i + 1u] = c[1]; rstat[i] = st; }
	}
}

// ---- rule 3 ----
// One thread per group of the resources that passed rules 1 and 2. The members' table entries: 0 < s < e is compressed-stored, s = e
// raw-stored, anything else fails the resource without a byte of it being read. Then the class. On a join a new block whose members all
// shrank is carried: its stored bytes are the members', which lie adjacent. On a split one lane walks the chunk headers of a
// compressed-stored source block -- a chain of at most 128 dependent two-byte loads, latency-bound by design, one lane per block across
// the whole grid -- and a new block whose images sum to less than its data is carried as those images. No read at or behind s.
__global__ __launch_bounds__(64) void tc_class_kernel(TcDims d, const uint8_t* __restrict__ packed, u64 packed_len, const u64* __restrict__ block_first,
                                                     const u64* __restrict__ block_off, const u64* __restrict__ res_len, bool with_crc,
                                                     const u64* __restrict__ gfirst, const u64* __restrict__ pfirst, int32_t* rstat,
                                                     uint32_t* __restrict__ gres, uint32_t* __restrict__ gwork,
                                                     u64* __restrict__ plen, u64* __restrict__ paddr, u64* __restrict__ pjf, u64* __restrict__ pdl, uint32_t* __restrict__ pkind,
                                                     const uint32_t* __restrict__ cnt)
{
	if (cnt[3]) { return; }                                              // rule 0 (the same in every thread)
	const u64 g = (u64)blockIdx.x * 64u + threadIdx.x;
	if (g >= d.ngmax || g >= gfirst[d.n_res]) { return; }
	const uint32_t r = res_of_block(gfirst, d.n_res, g);
	const u64 k = g - gfirst[r], L = res_len[r], G = (u64)1 << d.sg, B1 = (u64)1 << d.s1, B2 = (u64)1 << d.s2;
	const u64 span = tc_min(G, L - (k << d.sg));                         // (k < ceil(L / G))
	const u64 j0 = block_first[r] + (k << (d.sg - d.s1)), p0 = pfirst[r] + (k << (d.sg - d.s2));
	const uint32_t nm = (uint32_t)tc_ceil(span, d.s1), nn = (uint32_t)tc_ceil(span, d.s2);
	for (uint32_t i = 0; i < nn; ++i) { pkind[p0 + i] = TC_ROW_NONE; pjf[p0 + i] = ~(u64)0; }
	bool bad = false, all_comp = true;
	for (uint32_t i = 0; i < nm; ++i) {
		const u64 o0 = block_off[j0 + i], o1 = block_off[j0 + i + 1u], e = tc_min(B1, span - ((u64)i << d.s1));
		if (o1 < o0 || o1 > packed_len || o1 == o0 || o1 - o0 > e) { bad = true; }
		else if (o1 - o0 == e) { all_comp = false; }
	}
	uint32_t work = 0;
	if (!bad && d.mode == TC_JOIN && all_comp) {                         // (one new block per group)
		const u64 o0 = block_off[j0];
		pkind[p0] = TC_ROW_CARRY; plen[p0] = block_off[j0 + nm] - o0; paddr[p0] = (u64)(uintptr_t)(packed + o0);
		if (with_crc) { pjf[p0] = j0; pdl[p0] = span; }
	} else if (!bad && d.mode == TC_SPLIT && all_comp) {                 // (one source block per group)
		const u64 o0 = block_off[j0], s = block_off[j0 + 1u] - o0;
		const uint8_t* __restrict__ q = packed + o0;
		u64 pos = 0;
		bool any_raw = false;
		for (uint32_t i = 0; i < nn && !bad; ++i) {
			const u64 e2 = tc_min(B2, span - ((u64)i << d.s2)), start = pos;
			for (u64 c = (e2 + 4095u) >> 12; c != 0 && !bad; --c) {
				if (pos + 2u > s) { bad = true; break; }
				const uint32_t h = (uint32_t)q[pos] | ((uint32_t)q[pos + 1u] << 8);
				pos += (h & 0x0FFFu) + 3u;
				if (pos > s) { bad = true; }
			}
			if (bad) { break; }
			if (pos - start < e2) { pkind[p0 + i] = TC_ROW_CARRY; plen[p0 + i] = pos - start; paddr[p0 + i] = (u64)(uintptr_t)(q + start); }
			else { pkind[p0 + i] = TC_ROW_RAW; any_raw = true; }
		}
		if (!bad && pos != s) { bad = true; }                              // the images must tile the stored bytes
		work = any_raw || with_crc ? 1u : 0u;
	} else if (!bad) {
		for (uint32_t i = 0; i < nn; ++i) { pkind[p0 + i] = TC_ROW_ENCODE; }
		work = 1u;
	}
	if (bad) { rstat[r] = -3; work = 0; }                                 // MSCOMP_DATA_ERROR (every writer stores the same value)
	gres[g] = r; gwork[g] = work;
}

// ---- rule 4 ----
// One block: the running count of worked groups over the resources that stand (a resource that failed rule 3 is not read: its groups
// count nothing), the budget per resource -- the count only grows, so the resources that keep their slots are a prefix of it --, and
// the group of every slot in use.
__global__ __launch_bounds__(DV_THREADS) void tc_slots_kernel(TcDims d, const u64* __restrict__ gfirst, int32_t* rstat, const uint32_t* __restrict__ gres,
                                                             const uint32_t* __restrict__ gwork, uint32_t* gcum, uint32_t* __restrict__ slot_group, const uint32_t* __restrict__ cnt)
{
	__shared__ u64 s_w[1][DV_WAVES];
	if (cnt[3]) { return; }
	const uint32_t tid = threadIdx.x;
	const u64 ng = tc_min(gfirst[d.n_res], d.ngmax);
	u64 run[1] = {0};
	for (u64 base = 0; base < ng; base += DV_THREADS) {
		const u64 g = base + tid;
		u64 a[1] = {g < ng && gwork[g] && rstat[gres[g]] == 0 ? 1u : 0u};
		dv_block_scan<1>(a, run, s_w);
		if (g < ng) { gcum[g] = (uint32_t)a[0]; }                          // (<= ngmax < 2^31)
	}
	__syncthreads();
	for (uint32_t r = tid; r < d.n_res; r += DV_THREADS) {
		const u64 g1 = tc_min(gfirst[r + 1u], ng);
		if (rstat[r] == 0 && g1 != 0 && gcum[g1 - 1u] > d.gmax) { rstat[r] = -2; }   // MSCOMP_ARG_ERROR
	}
	__syncthreads();
	for (u64 g = tid; g < ng; g += DV_THREADS) {
		if (gwork[g] && rstat[gres[g]] == 0) { slot_group[gcum[g] - 1u] = (uint32_t)g + 1u; }
	}
}

// The unit tables, one thread per possible unit of either inner plan; a unit of a free slot is empty, without room. Decode units: the
// compressed-stored members of a worked group, decoded to their place in the group's cache slot; its raw-stored members are copied there
// when the group has more than one (a join) and read where they lie otherwise. Encode units: the group's new blocks, from the cache slot or
// from the raw-stored source block in d_packed -- the addresses go in as offsets from a null base, as the reader's CRC units do.
__global__ __launch_bounds__(256) void tc_units_kernel(TcDims d, const uint8_t* __restrict__ packed, const uint8_t* __restrict__ cache, const u64* __restrict__ block_first,
                                                      const u64* __restrict__ block_off, const u64* __restrict__ res_len, bool with_crc, TranscodeTab t)
{
	const u64 u = (u64)blockIdx.x * 256u + threadIdx.x;
	const uint32_t lmd = d.sg - d.s1, lme = d.sg - d.s2;
	const u64 dm = (u64)d.gmax << lmd, em = (u64)d.gmax << lme, G = (u64)1 << d.sg;
	bool decoded = false, encoded = false;
	if (u < dm) {
		const uint32_t slot = (uint32_t)(u >> lmd), g1 = t.slot_group[slot];
		const u64 i = u & (((u64)1 << lmd) - 1u);
		u64 io = 0, il = 0, oo = 0, oc = 0, src = 0, cl = 0, row = 0, raw = 0;
		uint32_t act = 0;
		if (g1) {
			const uint32_t r = t.gres[g1 - 1u];
			const u64 k = (u64)(g1 - 1u) - t.gfirst[r], span = tc_min(G, res_len[r] - (k << d.sg));
			if ((i << d.s1) < span) {
				const u64 e = tc_min((u64)1 << d.s1, span - (i << d.s1)), j = block_first[r] + (k << lmd) + i;
				const u64 o0 = block_off[j], s = block_off[j + 1u] - o0, at = ((u64)slot << d.sg) + (i << d.s1);   // (the class pass has checked the entries)
				if (s < e) {
					act = TC_ACT_DECODE | (uint32_t)e << 2; io = o0; il = s; oo = at; oc = e; row = j; decoded = true;
					src = (u64)(uintptr_t)(cache + at); cl = with_crc ? e : 0;
				} else if (lmd != 0) { act = TC_ACT_COPY | (uint32_t)e << 2; oo = at; raw = (u64)(uintptr_t)(packed + o0); }
			}
		}
		t.d_in_off[u] = io; t.d_in_len[u] = il; t.d_out_off[u] = oo; t.d_out_cap[u] = oc; t.d_src[u] = src; t.d_clen[u] = cl; t.d_row[u] = row; t.d_raw[u] = raw;
		t.d_act[u] = act;
	}
	if (u < em) {
		const uint32_t slot = (uint32_t)(u >> lme), g1 = t.slot_group[slot];
		const u64 i = u & (((u64)1 << lme) - 1u);
		u64 io = 0, il = 0, oo = 0, oc = 0, src = 0, cl = 0;
		if (g1) {
			const uint32_t r = t.gres[g1 - 1u];
			const u64 k = (u64)(g1 - 1u) - t.gfirst[r], span = tc_min(G, res_len[r] - (k << d.sg));
			if ((i << d.s2) < span) {
				const u64 e2 = tc_min((u64)1 << d.s2, span - (i << d.s2));
				const uint8_t* data = cache + ((u64)slot << d.sg);
				if (lmd == 0) {                                                 // one source block: raw-stored, its bytes are read where they lie
					const u64 j = block_first[r] + k, o0 = block_off[j];
					if (block_off[j + 1u] - o0 == span) { data = packed + o0; }
				}
				src = (u64)(uintptr_t)(data + (i << d.s2)); cl = with_crc ? e2 : 0;
				if (t.pkind[t.pfirst[r] + (k << lme) + i] == TC_ROW_ENCODE) { io = src; il = e2; oo = ((u64)slot << d.sg) + (i << d.s2); oc = e2 - 1u; encoded = true; }
			}
		}
		t.e_in_off[u] = io; t.e_in_len[u] = il; t.e_out_off[u] = oo; t.e_out_cap[u] = oc; t.e_src[u] = src; t.e_clen[u] = cl;
	}
	const uint32_t nd = (uint32_t)__popcll(__ballot(decoded)), ne = (uint32_t)__popcll(__ballot(encoded));
	if ((threadIdx.x & 63u) == 0) {
		if (nd) { atomicAdd(&t.cnt[1], nd); }
		if (ne) { atomicAdd(&t.cnt[2], ne); }
	}
}

// ---- behind the inner decompress plan ----
// The raw-stored members of the joined groups to their places in the cache, in pieces of 16 KiB handed out round robin to a grid fixed by
// the CU count, as a container's raw copy.
__global__ __launch_bounds__(CPD_THREADS) void tc_gather_kernel(u64 dm, uint32_t ppu_shift, uint8_t* __restrict__ cache, const u64* __restrict__ raw, const u64* __restrict__ dst_off,
                                                               const uint32_t* __restrict__ act)
{
	const u64 items = dm << ppu_shift;
	for (u64 i = blockIdx.x; i < items; i += gridDim.x) {
		const u64 u = i >> ppu_shift;
		const uint32_t a = act[u];
		const u64 at = (i & (((u64)1 << ppu_shift) - 1u)) << TC_PIECE_SHIFT, e = a >> 2;
		if ((a & 3u) != TC_ACT_COPY || at >= e) { continue; }
		cpd_move<false>(cache + dst_off[u] + at, reinterpret_cast<const uint8_t*>((uintptr_t)raw[u]) + at, tc_min(e - at, (u64)1 << TC_PIECE_SHIFT), threadIdx.x);
	}
}

// One thread per decode unit, behind the CRC kernels: a member that did not decode to exactly its data length, or -- with checksums -- not
// to the CRC-32 its row of the old table has, fails its resource.
__global__ __launch_bounds__(256) void tc_judge_kernel(u64 dm, uint32_t lmd, const uint32_t* __restrict__ block_crc, const uint32_t* __restrict__ act,
                                                      const int32_t* __restrict__ ustat, const u64* __restrict__ ulen, const uint32_t* __restrict__ ucrc,
                                                      const u64* __restrict__ row, const uint32_t* __restrict__ slot_group, const uint32_t* __restrict__ gres, int32_t* rstat)
{
	const u64 u = (u64)blockIdx.x * 256u + threadIdx.x;
	if (u >= dm) { return; }
	const uint32_t a = act[u];
	if ((a & 3u) != TC_ACT_DECODE) { return; }
	if (ustat[u] != 0 || ulen[u] != (u64)(a >> 2) || (block_crc && ucrc[u] != block_crc[row[u]])) { rstat[gres[slot_group[u >> lmd] - 1u]] = -3; }   // MSCOMP_DATA_ERROR
}

// ---- rules 5 and 6: the new tables ----
// One block: a resource that failed any rule has no blocks; new_first, the statuses so far, new_off[0].
__global__ __launch_bounds__(DV_THREADS) void tc_first_kernel(TcDims d, const u64* __restrict__ res_len, const int32_t* __restrict__ rstat, const uint32_t* __restrict__ cnt,
                                                             u64* __restrict__ new_first, u64* __restrict__ new_off, int32_t* __restrict__ status)
{
	__shared__ u64 s_w[1][DV_WAVES];
	const uint32_t tid = threadIdx.x;
	const bool refused = cnt[3] != 0;
	if (tid == 0) { new_first[0] = 0; new_off[0] = 0; }
	u64 run[1] = {0};
	for (uint32_t base = 0; base < d.n_res; base += DV_THREADS) {
		const uint32_t i = base + tid;
		const bool live = i < d.n_res;
		const int32_t st = !live ? 0 : refused ? -2 : rstat[i];
		u64 a[1] = {live && st == 0 ? tc_ceil(res_len[i], d.s2) : 0};
		dv_block_scan<1>(a, run, s_w);
		if (live) { new_first[i + 1u] = a[0]; status[i] = st; }
	}
}

// tile of rows: per final row its stored length (kept in new_off[j + 1] until the row pass), its checksum and where its stored bytes lie
// -- a carried row in the old container, an encoded one in the staging area when the inner plan fitted it into e - 1 bytes, any other at its
// data --, and the tile's sum
__global__ __launch_bounds__(DV_THREADS) void tc_tile_kernel(TcDims d, const uint8_t* __restrict__ stage, const u64* __restrict__ res_len, bool with_crc, TranscodeTab t,
                                                            const u64* __restrict__ new_first, u64* __restrict__ new_off, uint32_t* __restrict__ new_crc)
{
	__shared__ u64 s_w[1][DV_WAVES];
	if (t.cnt[3]) { return; }
	const u64 j = (u64)blockIdx.x * DV_THREADS + threadIdx.x;
	const uint32_t lme = d.sg - d.s2;
	u64 len = 0, at = 0;
	uint32_t crc = 0;
	bool carried = false;
	if (j < d.nbn && j < new_first[d.n_res]) {
		const uint32_t r = res_of_block(new_first, d.n_res, j);
		const u64 kb = j - new_first[r], p = t.pfirst[r] + kb, g = t.gfirst[r] + (kb >> lme);
		const u64 e2 = tc_min((u64)1 << d.s2, res_len[r] - (kb << d.s2));
		const u64 v = t.gwork[g] ? ((u64)(t.gcum[g] - 1u) << lme) + (kb & (((u64)1 << lme) - 1u)) : 0;   // its unit, when its group has a slot
		if (t.pkind[p] == TC_ROW_CARRY) {
			carried = true; len = t.plen[p]; at = t.paddr[p];
			if (with_crc) { crc = d.mode == TC_JOIN ? t.pcrc[p] : t.e_crc[v]; }
		} else {
			if (t.e_in_len[v] != 0 && t.e_ustat[v] == 0 && t.e_ulen[v] < e2) { len = t.e_ulen[v]; at = (u64)(uintptr_t)(stage + t.e_out_off[v]); }
			else { len = e2; at = t.e_src[v]; }
			if (with_crc) { crc = t.e_crc[v]; }
		}
	}
	if (j < d.nbn) { new_off[j + 1u] = len; t.addr[j] = at; if (new_crc) { new_crc[j] = crc; } }
	const uint32_t nc = (uint32_t)__popcll(__ballot(carried));
	if ((threadIdx.x & 63u) == 0 && nc) { atomicAdd(&t.cnt[0], nc); }
	u64 a[1] = {len}, sum[1] = {0};
	dv_block_scan<1>(a, sum, s_w);
	if (threadIdx.x == 0) { t.tsum[blockIdx.x] = sum[0]; }
}

// tile of rows: new_off from the sum in front of the tile; a row that ends beyond cap is not moved, and when it is the last row of its
// resource that resource gets MSCOMP_BUF_ERROR (the offsets only grow: the last block tells). A refused table: zeros.
__global__ __launch_bounds__(DV_THREADS) void tc_rows_kernel(TcDims d, u64 cap, const u64* __restrict__ new_first, u64* __restrict__ new_off, uint32_t* __restrict__ new_crc,
                                                            u64* __restrict__ addr, int32_t* __restrict__ status, const u64* __restrict__ tsum, const uint32_t* __restrict__ cnt)
{
	__shared__ u64 s_w[1][DV_WAVES];
	const u64 j = (u64)blockIdx.x * DV_THREADS + threadIdx.x;
	if (cnt[3]) {
		if (j < d.nbn) { new_off[j + 1u] = 0; if (new_crc) { new_crc[j] = 0; } }
		return;
	}
	u64 a[1] = {j < d.nbn ? new_off[j + 1u] : 0}, sum[1] = {blockIdx.x ? tsum[blockIdx.x - 1u] : 0};
	dv_block_scan<1>(a, sum, s_w);
	if (j >= d.nbn) { return; }
	new_off[j + 1u] = a[0];
	if (a[0] > cap && j < new_first[d.n_res]) {
		addr[j] = 0;
		const uint32_t r = res_of_block(new_first, d.n_res, j);
		if (new_first[r + 1u] == j + 1u) { status[r] = -5; }                 // MSCOMP_BUF_ERROR replaces MSCOMP_OK
	}
}

void launch_tc_resources(hipStream_t st, const TcDims& d, const u64* block_first, const u64* res_len, const TranscodeTab& t)
{
	hipLaunchKernelGGL(tc_res_kernel, dim3(1), dim3(DV_THREADS), 0, st, d, block_first, res_len, t.gfirst, t.pfirst, t.rstat, t.slot_group, t.cnt);
}

void launch_tc_classes(hipStream_t st, const TcDims& d, const uint8_t* packed, u64 packed_len, const u64* block_first, const u64* block_off, const u64* res_len,
                       bool with_crc, const TranscodeTab& t)
{
	if (d.ngmax == 0) { return; }
	hipLaunchKernelGGL(tc_class_kernel, dim3((d.ngmax + 63u) / 64u), dim3(64), 0, st, d, packed, packed_len, block_first, block_off, res_len, with_crc, t.gfirst, t.pfirst,
	                   t.rstat, t.gres, t.gwork, t.plen, t.paddr, t.pjf, t.pdl, t.pkind, t.cnt);
}

void launch_tc_units(hipStream_t st, const TcDims& d, const uint8_t* packed, const uint8_t* cache, const u64* block_first, const u64* block_off, const u64* res_len,
                     bool with_crc, const TranscodeTab& t)
{
	hipLaunchKernelGGL(tc_slots_kernel, dim3(1), dim3(DV_THREADS), 0, st, d, t.gfirst, t.rstat, t.gres, t.gwork, t.gcum, t.slot_group, t.cnt);
	const u64 dm = (u64)d.gmax << (d.sg - d.s1), em = (u64)d.gmax << (d.sg - d.s2), m = dm > em ? dm : em;
	if (m == 0) { return; }
	hipLaunchKernelGGL(tc_units_kernel, dim3((uint32_t)((m + 255u) / 256u)), dim3(256), 0, st, d, packed, cache, block_first, block_off, res_len, with_crc, t);
}

void launch_tc_gather(hipStream_t st, const TcDims& d, uint8_t* cache, const TranscodeTab& t, uint32_t blocks)
{
	const u64 dm = (u64)d.gmax << (d.sg - d.s1);
	if (dm == 0 || d.sg == d.s1) { return; }                             // (one source block per group: raw members are read where they lie)
	const uint32_t ppu_shift = d.s1 > TC_PIECE_SHIFT ? d.s1 - TC_PIECE_SHIFT : 0u;
	const u64 items = dm << ppu_shift;
	hipLaunchKernelGGL(tc_gather_kernel, dim3((uint32_t)(items < blocks ? items : blocks)), dim3(CPD_THREADS), 0, st, dm, ppu_shift, cache, t.d_raw, t.d_out_off, t.d_act);
}

void launch_tc_judge(hipStream_t st, const TcDims& d, const uint32_t* block_crc, const TranscodeTab& t)
{
	const u64 dm = (u64)d.gmax << (d.sg - d.s1);
	if (dm == 0) { return; }
	hipLaunchKernelGGL(tc_judge_kernel, dim3((uint32_t)((dm + 255u) / 256u)), dim3(256), 0, st, dm, d.sg - d.s1, block_crc, t.d_act, t.d_ustat, t.d_ulen, t.d_crc, t.d_row,
	                   t.slot_group, t.gres, t.rstat);
}

void launch_tc_first(hipStream_t st, const TcDims& d, const u64* res_len, const TranscodeTab& t, u64* new_first, u64* new_off, int32_t* status)
{
	hipLaunchKernelGGL(tc_first_kernel, dim3(1), dim3(DV_THREADS), 0, st, d, res_len, t.rstat, t.cnt, new_first, new_off, status);
}

void launch_tc_tiles(hipStream_t st, const TcDims& d, const uint8_t* stage, const u64* res_len, bool with_crc, const TranscodeTab& t, const u64* new_first, u64* new_off,
                     uint32_t* new_crc)
{
	hipLaunchKernelGGL(tc_tile_kernel, dim3(row_tiles(d.nbn)), dim3(DV_THREADS), 0, st, d, stage, res_len, with_crc, t, new_first, new_off, new_crc);
}

void launch_tc_rows(hipStream_t st, const TcDims& d, u64 cap, const TranscodeTab& t, const u64* new_first, u64* new_off, uint32_t* new_crc, int32_t* status)
{
	hipLaunchKernelGGL(tc_rows_kernel, dim3(row_tiles(d.nbn)), dim3(DV_THREADS), 0, st, d, cap, new_first, new_off, new_crc, t.addr, status, t.tsum, t.cnt);
}

} // namespace msc
