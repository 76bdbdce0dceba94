// blocks.hip -- the table, select, raw-copy and fold passes of a block container (mscomp_amd_blocks_*, include/mscomp_amd.h): a batch of
// resources cut into blocks of B = 1 << shift bytes, every block compressed on its own or stored raw, packed back to back behind a table of
// offsets. The two big stages are a compress and a decompress dev plan over the blocks as units (blockobj.hip runs them between these passes,
// unchanged); the pack pass is compaction's copy with a source address per unit (devplan.hip cpd_copy_kernel<true>). DESIGN.md 4.7.
#include "kernels.h"

namespace msc {

// ---- compress ----
// One block walks the resources in tiles of 1024: the bounds check (running total of res_len <= in_max; a rejected resource has no blocks),
// block_first (n + 1), and where the resource's compressed blocks are staged: resources back to back in block order, every start rounded up
// to 16, block j at + j * B -- so the staging area is in_max + 16 n bytes whatever the mix of lengths.
__global__ __launch_bounds__(DV_THREADS) void bk_cres_kernel(uint32_t n, uint32_t shift, u64 in_max, const u64* __restrict__ res_len,
                                                            u64* __restrict__ block_first, u64* __restrict__ stage_base, int32_t* __restrict__ rstat)
{
	__shared__ u64 s_w[2][DV_WAVES];
	const uint32_t tid = threadIdx.x;
	const u64 B = (u64)1 << shift;
	u64 run[1] = {0}, cnt[2] = {0, 0};
	if (tid == 0) { block_first[0] = 0; }
	for (uint32_t base = 0; base < n; base += DV_THREADS) {
		const uint32_t i = base + tid;
		const bool live = i < n;
		const u64 len = live ? res_len[i] : 0;
		u64 r[1] = {len};
		dv_block_scan<1>(r, run, s_w);                                   // running total up to and including resource i
		const bool rej = live && r[0] > in_max;
		const u64 L = rej ? 0 : len, room = (L + 15u) & ~(u64)15u;       // (L <= in_max < 2^50, mscomp_amd_blocks_create: no overflow)
		u64 c[2] = {(L + B - 1u) >> shift, room};
		dv_block_scan<2>(c, cnt, s_w);
		if (live) { block_first[i + 1u] = c[0]; stage_base[i] = c[1] - room; rstat[i] = rej ? -2 : 0; }   // MSCOMP_ARG_ERROR
	}
}

// The inner compress plan's unit tables, one thread per possible block: input res_off + j B, staging capacity len - 1 (a block that does not
// shrink is MSCOMP_BUF_ERROR there, and is stored raw). Blocks at or past the real count are empty units without room.
__global__ __launch_bounds__(256) void bk_cunits_kernel(uint32_t n_res, uint32_t nbmax, uint32_t shift, const u64* __restrict__ res_off, const u64* __restrict__ res_len,
                                                       const u64* __restrict__ block_first, const u64* __restrict__ stage_base,
                                                       u64* __restrict__ in_off, u64* __restrict__ in_len, u64* __restrict__ out_off, u64* __restrict__ out_cap)
{
	const uint32_t b = blockIdx.x * 256u + threadIdx.x;
	if (b >= nbmax) { return; }
	const u64 B = (u64)1 << shift;
	u64 io = 0, il = 0, oo = 0, oc = 0;
	if (b < block_first[n_res]) {
		const uint32_t r = res_of_block(block_first, n_res, b);
		const u64 at = (b - block_first[r]) << shift, left = res_len[r] - at;
		io = res_off[r] + at; il = left < B ? left : B; oo = stage_base[r] + at; oc = il - 1u;
	}
	in_off[b] = io; in_len[b] = il; out_off[b] = oo; out_cap[b] = oc;
}

// Select, scan and status in one block: per block the stored form (the staged bytes when the inner plan fitted them into len - 1, the raw
// input otherwise) as a length and a source address, block_off (nbmax + 1; the entries behind the real count repeat the total), and then
// per resource MSCOMP_ARG_ERROR / MSCOMP_BUF_ERROR (its last block ends beyond cap: the pack pass leaves such blocks out) / MSCOMP_OK.
__global__ __launch_bounds__(DV_THREADS) void bk_select_kernel(uint32_t n_res, uint32_t nbmax, u64 cap, const uint8_t* __restrict__ d_in, const uint8_t* __restrict__ stage,
                                                              const u64* __restrict__ block_first, const u64* __restrict__ in_off, const u64* __restrict__ in_len,
                                                              const u64* __restrict__ st_off, const u64* __restrict__ clen, const int32_t* __restrict__ cstat,
                                                              u64* __restrict__ slen, u64* __restrict__ src, u64* block_off,
                                                              const int32_t* __restrict__ rstat, int32_t* __restrict__ d_status)
{
	__shared__ u64 s_w[1][DV_WAVES];
	const uint32_t tid = threadIdx.x;
	u64 run[1] = {0};
	if (tid == 0) { block_off[0] = 0; }
	for (uint32_t base = 0; base < nbmax; base += DV_THREADS) {
		const uint32_t b = base + tid;
		const bool live = b < nbmax;
		const u64 L = live ? in_len[b] : 0;                               // (0 behind the real count)
		const bool comp = L != 0 && cstat[b] == 0 && clen[b] < L;
		u64 v[1] = {comp ? clen[b] : L};
		const u64 s = v[0];
		dv_block_scan<1>(v, run, s_w);
		if (live) {
			block_off[b + 1u] = v[0]; slen[b] = s;
			src[b] = L == 0 ? 0 : (u64)(uintptr_t)(comp ? stage + st_off[b] : d_in + in_off[b]);
		}
	}
	__syncthreads();                                                     // block_off is read back below, by other threads of this block
	for (uint32_t r = tid; r < n_res; r += DV_THREADS) {
		int32_t st = rstat[r];
		const u64 f0 = block_first[r], f1 = block_first[r + 1u];
		if (st == 0 && f1 > f0 && block_off[f1] > cap) { st = -5; }      // MSCOMP_BUF_ERROR (the offsets only grow: the last block tells)
		d_status[r] = st;
	}
}

// ---- decompress ----
#define BK_SKIP   0u
#define BK_COPY   1u
#define BK_DECODE 2u
#define BK_FAIL   3u                                      // (the action word of a unit: kind | data length << 2)

// One block walks the resources: the per-resource checks in their order (bounds -> MSCOMP_ARG_ERROR, block count -> MSCOMP_DATA_ERROR,
// capacity -> MSCOMP_BUF_ERROR), the clipped range and the bytes it stands for, and unit_first (n + 1): the inner plan's units are the
// blocks IN RANGE of the resources that passed, numbered densely in resource order -- a numbering that is this pass's own running sum,
// so that a damaged block_first cannot make two resources share a unit or send the search below astray.
__global__ __launch_bounds__(DV_THREADS) void bk_dres_kernel(uint32_t n, uint32_t nbmax, uint32_t shift, u64 in_max, const u64* __restrict__ res_len,
                                                            const u64* __restrict__ block_first, const u64* __restrict__ range, const u64* __restrict__ out_cap,
                                                            u64* __restrict__ unit_first, u64* __restrict__ rf, u64* __restrict__ want, int32_t* __restrict__ rstat)
{
	__shared__ u64 s_w[1][DV_WAVES];
	const uint32_t tid = threadIdx.x;
	const u64 B = (u64)1 << shift;
	u64 run[1] = {0}, cnt[1] = {0};
	if (tid == 0) { unit_first[0] = 0; }
	for (uint32_t base = 0; base < n; base += DV_THREADS) {
		const uint32_t i = base + tid;
		const bool live = i < n;
		const u64 len = live ? res_len[i] : 0;
		u64 r[1] = {len};
		dv_block_scan<1>(r, run, s_w);
		int32_t st = 0;
		u64 f = 0, c = 0, w = 0;
		if (live) {
			const u64 f0 = block_first[i], f1 = block_first[i + 1u];
			if (r[0] > in_max || f0 > nbmax || f1 > nbmax) { st = -2; }
			else {
				const u64 nblk = (len + B - 1u) >> shift;
				if (f1 - f0 != nblk) { st = -3; }
				else {
					const u64 qf = range ? range[2u * (size_t)i] : 0, qc = range ? range[2u * (size_t)i + 1u] : nblk;
					f = qf < nblk ? qf : nblk; c = qc < nblk - f ? qc : nblk - f;
					if (c) { const u64 end = (f + c) << shift; w = (len < end ? len : end) - (f << shift); }
					if (w > out_cap[i]) { st = -5; }
				}
			}
		}
		u64 k[1] = {st == 0 ? c : 0};
		dv_block_scan<1>(k, cnt, s_w);
		if (live) { unit_first[i + 1u] = k[0]; rf[i] = f; want[i] = w; rstat[i] = st; }
	}
}

// The inner decompress plan's unit tables and the action words, one thread per possible unit. A block whose stored length s equals its data
// length e is copied, 0 < s < e is decoded into capacity e at its final place; everything else -- a decreasing table, an end beyond
// packed_len, s > e, s = 0 -- fails the resource without a byte of the block being read. Only blocks to decode reach the inner plan with a
// length; all other units are empty there, with capacity 0. `only` (salvage's mask over the container's rows, else null): a row it marks
// good is not judged -- BK_SKIP with its data length, nothing read.
__global__ __launch_bounds__(256) void bk_dunits_kernel(uint32_t n_res, uint32_t nbmax, uint32_t shift, u64 packed_len, const u64* __restrict__ res_len,
                                                       const u64* __restrict__ block_first, const u64* __restrict__ block_off, const u64* __restrict__ d_out_off,
                                                       const u64* __restrict__ unit_first, const u64* __restrict__ rf, const uint32_t* __restrict__ only,
                                                       u64* __restrict__ in_off, u64* __restrict__ in_len, u64* __restrict__ out_off, u64* __restrict__ out_cap,
                                                       u64* __restrict__ raw_src, u64* __restrict__ raw_dst, uint32_t* __restrict__ act)
{
	const uint32_t u = blockIdx.x * 256u + threadIdx.x;
	if (u >= nbmax) { return; }
	const u64 B = (u64)1 << shift;
	u64 io = 0, il = 0, oo = 0, oc = 0, rs = 0, rd = 0;
	uint32_t a = BK_SKIP;
	if (u < unit_first[n_res]) {
		const uint32_t r = res_of_block(unit_first, n_res, u);
		const u64 k = u - unit_first[r], jb = rf[r] + k, j = block_first[r] + jb;    // (j < block_first[r + 1] <= nbmax: bk_dres_kernel)
		const u64 left = res_len[r] - (jb << shift), e = left < B ? left : B;
		const u64 o0 = block_off[j], o1 = block_off[j + 1u], dst = d_out_off[r] + (k << shift);
		if (only && only[j] == SV_GOOD) { a = BK_SKIP; }                   // salvage: a row the mask leaves out is an empty unit, with its data length
		else if (o1 < o0 || o1 > packed_len) { a = BK_FAIL; }
		else {
			const u64 s = o1 - o0;
			if (s == e) { a = BK_COPY; rs = o0; rd = dst; }
			else if (s != 0 && s < e) { a = BK_DECODE; io = o0; il = s; oo = dst; oc = e; }
			else { a = BK_FAIL; }
		}
		a |= (uint32_t)e << 2;                                             // (e <= 512 KiB)
	}
	in_off[u] = io; in_len[u] = il; out_off[u] = oo; out_cap[u] = oc; raw_src[u] = rs; raw_dst[u] = rd; act[u] = a;
}

// The raw blocks to their places, in pieces of 16 KiB handed out round robin to a grid fixed by the CU count: one 512 KiB block is moved by
// 32 workgroups, and a unit that is not a raw block costs one load of its action word per piece it could have had.
#define BK_PIECE_SHIFT 14u
__global__ __launch_bounds__(CPD_THREADS) void bk_rawcopy_kernel(uint32_t nbmax, uint32_t ppu_shift, const uint8_t* __restrict__ packed, uint8_t* __restrict__ out,
                                                                const u64* __restrict__ raw_src, const u64* __restrict__ raw_dst, const uint32_t* __restrict__ act)
{
	const u64 items = (u64)nbmax << ppu_shift;
	for (u64 i = blockIdx.x; i < items; i += gridDim.x) {
		const uint32_t u = (uint32_t)(i >> ppu_shift), a = act[u];
		const u64 at = (i & (((u64)1 << ppu_shift) - 1u)) << BK_PIECE_SHIFT, e = a >> 2;
		if ((a & 3u) != BK_COPY || at >= e) { continue; }
		const u64 cnt = e - at < ((u64)1 << BK_PIECE_SHIFT) ? e - at : (u64)1 << BK_PIECE_SHIFT;
		cpd_move<false>(out + raw_dst[u] + at, packed + raw_src[u] + at, cnt, threadIdx.x);
	}
}

// One wave per resource: its units' verdicts (a failed table check; a decoder status other than MSCOMP_OK or a length other than e) folded
// behind the resource's own, into d_status and d_out_len.
__global__ __launch_bounds__(256) void bk_dfold_kernel(uint32_t n_res, const u64* __restrict__ unit_first, const uint32_t* __restrict__ act,
                                                      const u64* __restrict__ dlen, const int32_t* __restrict__ dstat, const int32_t* __restrict__ rstat,
                                                      const u64* __restrict__ want, u64* __restrict__ d_out_len, int32_t* __restrict__ d_status)
{
	const uint32_t r = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
	if (r >= n_res) { return; }
	const int32_t st = rstat[r];
	bool bad = false;
	if (st == 0) {
		for (u64 u = unit_first[r] + lane; u < unit_first[r + 1u]; u += 64u) {
			const uint32_t a = act[u], kind = a & 3u;
			if (kind == BK_FAIL || (kind == BK_DECODE && (dstat[u] != 0 || dlen[u] != (u64)(a >> 2)))) { bad = true; }
		}
	}
	const bool any_bad = __ballot(bad) != 0;
	if (lane == 0) {
		const int32_t s = st != 0 ? st : any_bad ? -3 : 0;                 // MSCOMP_DATA_ERROR
		d_status[r] = s; d_out_len[r] = s == 0 ? want[r] : 0;
	}
}

// ---- checksums (mscomp_amd_blocks_crc / _check; the CRC kernels themselves: crc32.hip) ----
// crc, behind bk_cres_kernel and bk_cunits_kernel, one thread per possible block: the resource a block belongs to and the bytes of the resource
// behind the block -- the second distance, by which the block's parts add up to the CRC of the whole resource in the same pass
__global__ __launch_bounds__(256) void bk_crcgroups_kernel(uint32_t n_res, uint32_t nbmax, uint32_t shift, const u64* __restrict__ res_len, const u64* __restrict__ block_first,
                                                          const u64* __restrict__ in_len, uint32_t* __restrict__ grp, u64* __restrict__ after)
{
	const uint32_t b = blockIdx.x * 256u + threadIdx.x;
	if (b >= nbmax) { return; }
	uint32_t g = 0; u64 a = 0;
	if (b < block_first[n_res]) {
		g = res_of_block(block_first, n_res, b);
		a = res_len[g] - ((b - block_first[g]) << shift) - in_len[b];
	}
	grp[b] = g; after[b] = a;
}

// check: bk_dres_kernel's checks 1 and 2 and its clipped range for the resources that are MSCOMP_OK on entry; the others have no units
__global__ __launch_bounds__(DV_THREADS) void bk_kres_kernel(uint32_t n, uint32_t nbmax, uint32_t shift, u64 in_max, const u64* __restrict__ res_len,
                                                            const u64* __restrict__ block_first, const u64* __restrict__ range, const int32_t* __restrict__ d_status,
                                                            u64* __restrict__ unit_first, u64* __restrict__ rf, int32_t* __restrict__ rstat)
{
	__shared__ u64 s_w[1][DV_WAVES];
	const uint32_t tid = threadIdx.x;
	const u64 B = (u64)1 << shift;
	u64 run[1] = {0}, cnt[1] = {0};
	if (tid == 0) { unit_first[0] = 0; }
	for (uint32_t base = 0; base < n; base += DV_THREADS) {
		const uint32_t i = base + tid;
		const bool live = i < n;
		const u64 len = live ? res_len[i] : 0;
		u64 r[1] = {len};
		dv_block_scan<1>(r, run, s_w);
		int32_t st = BK_LEAVE;
		u64 f = 0, c = 0;
		if (live && d_status[i] == 0) {
			const u64 f0 = block_first[i], f1 = block_first[i + 1u];
			st = 0;
			if (r[0] > in_max || f0 > nbmax || f1 > nbmax) { st = -2; }
			else {
				const u64 nblk = (len + B - 1u) >> shift;
				if (f1 - f0 != nblk) { st = -3; }
				else {
					const u64 qf = range ? range[2u * (size_t)i] : 0, qc = range ? range[2u * (size_t)i + 1u] : nblk;
					f = qf < nblk ? qf : nblk; c = qc < nblk - f ? qc : nblk - f;
				}
			}
		}
		u64 k[1] = {st == 0 ? c : 0};
		dv_block_scan<1>(k, cnt, s_w);
		if (live) { unit_first[i + 1u] = k[0]; rf[i] = f; rstat[i] = st; }
	}
}

// ... one thread per possible unit: where the block lies in the decoded output, its data length, and which entry of d_block_crc it answers to
__global__ __launch_bounds__(256) void bk_kunits_kernel(uint32_t n_res, uint32_t nbmax, uint32_t shift, const u64* __restrict__ res_len, const u64* __restrict__ block_first,
                                                       const u64* __restrict__ d_out_off, const u64* __restrict__ unit_first, const u64* __restrict__ rf,
                                                       u64* __restrict__ in_off, u64* __restrict__ in_len, u64* __restrict__ which)
{
	const uint32_t u = blockIdx.x * 256u + threadIdx.x;
	if (u >= nbmax) { return; }
	const u64 B = (u64)1 << shift;
	u64 io = 0, il = 0, j = 0;
	if (u < unit_first[n_res]) {
		const uint32_t r = res_of_block(unit_first, n_res, u);
		const u64 k = u - unit_first[r], jb = rf[r] + k;
		const u64 left = res_len[r] - (jb << shift);
		j = block_first[r] + jb;                                           // (< block_first[r + 1] <= nbmax: bk_kres_kernel)
		io = d_out_off[r] + (k << shift); il = left < B ? left : B;
	}
	in_off[u] = io; in_len[u] = il; which[u] = j;
}

// ... one wave per resource, behind the CRC kernels (W = 1: an entry is a CRC word) or a digester's root pass (W = 4: a digest): a failed
// table check, or a block whose entry in `read` is not the one given, into d_status and d_out_len. A resource that passes, or was not
// MSCOMP_OK on entry, is not written.
template <uint32_t W>
__global__ __launch_bounds__(256) void bk_kfold_kernel(uint32_t n_res, const u64* __restrict__ unit_first, const u64* __restrict__ which, const uint32_t* __restrict__ read,
                                                      const uint32_t* __restrict__ given, const int32_t* __restrict__ rstat, u64* __restrict__ d_out_len, int32_t* __restrict__ d_status)
{
	const uint32_t r = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
	if (r >= n_res) { return; }
	const int32_t st = rstat[r];
	if (st == BK_LEAVE) { return; }
	bool bad = false;
	if (st == 0) {
		for (u64 u = unit_first[r] + lane; u < unit_first[r + 1u]; u += 64u) {
			const uint32_t* a = read + W * u;
			const uint32_t* b = given + W * which[u];
			#pragma unroll
			for (uint32_t i = 0; i < W; ++i) { if (a[i] != b[i]) { bad = true; } }
		}
	}
	const bool any_bad = __ballot(bad) != 0;
	if (lane == 0 && (st != 0 || any_bad)) { d_status[r] = st != 0 ? st : -3; d_out_len[r] = 0; }   // MSCOMP_DATA_ERROR
}

// ---- salvage (mscomp_amd_blocks_salvage): verdicts per block behind the decompress passes, d_range = NULL ----
// Behind the raw copy, one thread per possible unit: the CRC columns pointed at the blocks in d_out -- a block that was copied, or decoded
// to its length, is read over its e bytes, every other unit is empty --, the row a unit answers to (`which`), every verdict SKIPPED until
// the verdict pass says otherwise, and the four counts cleared. The raw columns and the inner plan's tables are free from here on; ustat,
// ulen and act are not.
__global__ __launch_bounds__(256) void bk_sunits_kernel(uint32_t n_res, uint32_t nbmax, uint32_t shift, const u64* __restrict__ block_first, const u64* __restrict__ d_out_off,
                                                       const u64* __restrict__ unit_first, const uint32_t* __restrict__ act, const u64* __restrict__ dlen,
                                                       const int32_t* __restrict__ dstat, u64* __restrict__ in_off, u64* __restrict__ in_len, u64* __restrict__ which,
                                                       uint32_t* __restrict__ verdict, u64* __restrict__ count)
{
	const uint32_t u = blockIdx.x * 256u + threadIdx.x;
	if (u >= nbmax) { return; }
	if (u == 0) { count[0] = count[1] = count[2] = count[3] = 0; }
	u64 io = 0, il = 0, j = 0;
	if (u < unit_first[n_res]) {
		const uint32_t r = res_of_block(unit_first, n_res, u), a = act[u], kind = a & 3u;
		const u64 k = u - unit_first[r], e = a >> 2;
		j = block_first[r] + k;                                            // (< block_first[r + 1] <= nbmax: bk_dres_kernel)
		io = d_out_off[r] + (k << shift);
		if (kind == BK_COPY || (kind == BK_DECODE && dstat[u] == 0 && dlen[u] == e)) { il = e; }
	}
	in_off[u] = io; in_len[u] = il; which[u] = j; verdict[u] = SV_SKIPPED;
}

// Behind the CRC kernels (or the pass above, without checksums), one thread per possible row: the first of TABLE, DECODE, CRC that applies,
// else GOOD, into d_verdict at the unit's row and -- for the two passes behind -- into the unit's own word, where the CRC-32 stood. A
// masked unit and a unit behind the real count are SKIPPED there.
__global__ __launch_bounds__(256) void bk_sverdict_kernel(uint32_t n_res, uint32_t nbmax, const u64* __restrict__ unit_first, const uint32_t* __restrict__ act,
                                                         const u64* __restrict__ dlen, const int32_t* __restrict__ dstat, const u64* __restrict__ which,
                                                         const uint32_t* __restrict__ block_crc, uint32_t* __restrict__ ucrc, uint32_t* __restrict__ verdict)
{
	const uint32_t u = blockIdx.x * 256u + threadIdx.x;
	if (u >= nbmax) { return; }
	uint32_t v = SV_SKIPPED;
	if (u < unit_first[n_res]) {
		const uint32_t a = act[u], kind = a & 3u;
		if (kind != BK_SKIP) {
			const u64 j = which[u];
			if (kind == BK_FAIL) { v = SV_TABLE; }
			else if (kind == BK_DECODE && (dstat[u] != 0 || dlen[u] != (u64)(a >> 2))) { v = SV_DECODE; }
			else { v = block_crc && ucrc[u] != block_crc[j] ? SV_CRC : SV_GOOD; }
			verdict[j] = v;
		}
	}
	ucrc[u] = v;
}

// The e bytes of every judged bad row zeroed -- a failed decoder may have written inside its capacity --, in the shape of bk_rawcopy_kernel:
// pieces of 16 KiB round robin over a grid fixed by the CU count, 16-byte stores behind a bytewise head.
__global__ __launch_bounds__(CPD_THREADS) void bk_szero_kernel(uint32_t nbmax, uint32_t ppu_shift, uint8_t* __restrict__ out, const u64* __restrict__ dst,
                                                              const uint32_t* __restrict__ act, const uint32_t* __restrict__ uv)
{
	const u64 items = (u64)nbmax << ppu_shift;
	for (u64 i = blockIdx.x; i < items; i += gridDim.x) {
		const uint32_t u = (uint32_t)(i >> ppu_shift), v = uv[u];
		const u64 at = (i & (((u64)1 << ppu_shift) - 1u)) << BK_PIECE_SHIFT, e = act[u] >> 2;
		if (v == SV_GOOD || v == SV_SKIPPED || at >= e) { continue; }
		const u64 cnt = e - at < ((u64)1 << BK_PIECE_SHIFT) ? e - at : (u64)1 << BK_PIECE_SHIFT;
		cpd_move<true>(out + dst[u] + at, nullptr, cnt, threadIdx.x);
	}
}

// One wave per resource: its judged and its bad rows counted, d_out_len = L for every accepted resource whatever its rows say, d_bad,
// d_status, and the resource's share of the four counts (sums of whole numbers: the same from run to run).
__global__ __launch_bounds__(256) void bk_sfold_kernel(uint32_t n_res, const u64* __restrict__ unit_first, const uint32_t* __restrict__ act, const uint32_t* __restrict__ uv,
                                                      const int32_t* __restrict__ rstat, const u64* __restrict__ want, u64* __restrict__ d_out_len,
                                                      uint32_t* __restrict__ d_bad, int32_t* __restrict__ d_status, u64* count)
{
	const uint32_t r = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
	if (r >= n_res) { return; }
	const int32_t st = rstat[r];
	u64 judged = 0, bad = 0, zeroed = 0;
	if (st == 0) {
		for (u64 u = unit_first[r] + lane; u < unit_first[r + 1u]; u += 64u) {
			const uint32_t v = uv[u];
			if (v != SV_SKIPPED) { ++judged; }
			if (v != SV_SKIPPED && v != SV_GOOD) { ++bad; zeroed += act[u] >> 2; }
		}
	}
	#pragma unroll
	for (uint32_t d = 32u; d; d >>= 1) { judged += __shfl_down(judged, d, 64); bad += __shfl_down(bad, d, 64); zeroed += __shfl_down(zeroed, d, 64); }
	if (lane == 0) {
		d_out_len[r] = st == 0 ? want[r] : 0; d_bad[r] = (uint32_t)bad; d_status[r] = st != 0 ? st : bad ? -3 : 0;   // MSCOMP_DATA_ERROR
		unsigned long long* c = reinterpret_cast<unsigned long long*>(count);
		if (judged) { atomicAdd(c, (unsigned long long)judged); }
		if (bad) { atomicAdd(c + 1, (unsigned long long)bad); atomicAdd(c + 2, (unsigned long long)zeroed); atomicAdd(c + 3, 1ull); }
	}
}

// ---- move (the last pass of mscomp_amd_writer_write, _writer_resize and mscomp_amd_splicer_splice) ----
// The only pass over a whole new container, and it knows nothing of where a row's bytes come from: the call's layout pass wrote addr[row],
// the address of the row's stored bytes, or 0 for a row that is not moved (nothing stored, unreadable, or ending beyond cap). The new byte
// range [0, min(total, cap)) is cut into equal slices, one per block of a fixed grid, as compaction cuts it (cpd_copy_kernel); a workgroup
// finds the row its slice starts in and walks on from there, 64 table rows looked at at once, a row per lane. The rows from j on whose
// address lies as far from their new offset as row j's lie back to back at the source too, so they are ONE copy shifted by a constant:
// the untouched rows of an old container, consecutive picks of consecutive resources, raw dirty blocks in consecutive cache slots. A run
// ends where the source, or the place in it, changes. A refused table has new_off all zeros: the range is empty.
__global__ __launch_bounds__(CPD_THREADS) void bk_move_kernel(uint32_t nbt, u64 cap, const u64* __restrict__ new_off, const u64* __restrict__ addr,
                                                             uint8_t* __restrict__ dst)
{
	const uint32_t tid = threadIdx.x, lane = tid & 63u;
	const u64 total = new_off[nbt], range = total < cap ? total : cap;
	u64 per = (range + gridDim.x - 1u) / gridDim.x;
	per = (per + 4095u) & ~(u64)4095u;
	const u64 lo = (u64)blockIdx.x * per;
	if (lo >= range) { return; }
	const u64 hi = range - lo < per ? range : lo + per;
	uint32_t j = 0, b = nbt;                                             // the first row with new_off[j + 1] > lo (there is one: new_off[nbt] > lo)
	while (j < b) { const uint32_t mid = j + (b - j) / 2u; if (new_off[mid + 1u] > lo) { b = mid; } else { j = mid + 1u; } }
	while (j < nbt) {
		const u64 o = new_off[j];
		if (o >= hi) { break; }
		const uint32_t row = j + lane;
		u64 e0 = 0, e1 = 0, at = 0;
		if (row < nbt) { e0 = new_off[row]; e1 = new_off[row + 1u]; at = addr[row]; }
		const u64 at0 = __shfl(at, 0, 64);
		const u64 others = ~__ballot(at != 0 && at - e0 == at0 - o);
		const uint32_t k = others ? (uint32_t)__ffsll((unsigned long long)others) - 1u : 64u;   // rows of the run from j on (the same in every wave of the block)
		if (k == 0) { ++j; continue; }
		const u64 end = __shfl(e1, (int)k - 1, 64);
		j += k;
		const u64 d0 = o > lo ? o : lo, d1 = end < hi ? end : hi;
		if (d0 < d1) { cpd_move<false>(dst + d0, reinterpret_cast<const uint8_t*>((uintptr_t)at0) + (d0 - o), d1 - d0, tid); }
	}
}

void launch_blocks_move(hipStream_t st, uint32_t nbt, u64 cap, const u64* new_off, const u64* addr, uint8_t* dst, uint32_t blocks)
{
	if (nbt == 0) { return; }
	hipLaunchKernelGGL(bk_move_kernel, dim3(blocks), dim3(CPD_THREADS), 0, st, nbt, cap, new_off, addr, dst);
}

void launch_blocks_ctables(hipStream_t st, uint32_t n_res, uint32_t nbmax, uint32_t shift, u64 in_max, const u64* res_off, const u64* res_len,
                           u64* block_first, const BlocksTab& t)
{
	hipLaunchKernelGGL(bk_cres_kernel, dim3(1), dim3(DV_THREADS), 0, st, n_res, shift, in_max, res_len, block_first, t.res_a, t.rstat);
	if (nbmax == 0) { return; }
	hipLaunchKernelGGL(bk_cunits_kernel, dim3((nbmax + 255u) / 256u), dim3(256), 0, st, n_res, nbmax, shift, res_off, res_len, block_first, t.res_a,
	                   t.in_off, t.in_len, t.out_off, t.out_cap);
}

void launch_blocks_select(hipStream_t st, uint32_t n_res, uint32_t nbmax, u64 cap, const uint8_t* d_in, const uint8_t* stage, const u64* block_first,
                          const BlocksTab& t, u64* block_off, int32_t* d_status)
{
	hipLaunchKernelGGL(bk_select_kernel, dim3(1), dim3(DV_THREADS), 0, st, n_res, nbmax, cap, d_in, stage, block_first, t.in_off, t.in_len, t.out_off,
	                   t.ulen, t.ustat, t.aux_a, t.aux_b, block_off, t.rstat, d_status);
}

void launch_blocks_dtables(hipStream_t st, uint32_t n_res, uint32_t nbmax, uint32_t shift, u64 in_max, u64 packed_len, const u64* res_len,
                           const u64* block_first, const u64* block_off, const u64* range, const u64* d_out_off, const u64* d_out_cap, const uint32_t* only,
                           const BlocksTab& t)
{
	hipLaunchKernelGGL(bk_dres_kernel, dim3(1), dim3(DV_THREADS), 0, st, n_res, nbmax, shift, in_max, res_len, block_first, range, d_out_cap,
	                   t.unit_first, t.res_b, t.res_a, t.rstat);
	if (nbmax == 0) { return; }
	hipLaunchKernelGGL(bk_dunits_kernel, dim3((nbmax + 255u) / 256u), dim3(256), 0, st, n_res, nbmax, shift, packed_len, res_len, block_first, block_off, d_out_off,
	                   t.unit_first, t.res_b, only, t.in_off, t.in_len, t.out_off, t.out_cap, t.aux_a, t.aux_b, t.act);
}

void launch_blocks_rawcopy(hipStream_t st, uint32_t nbmax, uint32_t shift, const uint8_t* packed, uint8_t* out, const BlocksTab& t, uint32_t blocks)
{
	if (nbmax == 0) { return; }
	const uint32_t ppu_shift = shift > BK_PIECE_SHIFT ? shift - BK_PIECE_SHIFT : 0u;
	const u64 items = (u64)nbmax << ppu_shift;
	hipLaunchKernelGGL(bk_rawcopy_kernel, dim3((uint32_t)(items < blocks ? items : blocks)), dim3(CPD_THREADS), 0, st, nbmax, ppu_shift, packed, out, t.aux_a, t.aux_b, t.act);
}

void launch_blocks_dfold(hipStream_t st, uint32_t n_res, const BlocksTab& t, u64* d_out_len, int32_t* d_status)
{
	if (n_res == 0) { return; }
	hipLaunchKernelGGL(bk_dfold_kernel, dim3((n_res + 3u) / 4u), dim3(256), 0, st, n_res, t.unit_first, t.act, t.ulen, t.ustat, t.rstat, t.res_a, d_out_len, d_status);
}

void launch_blocks_sunits(hipStream_t st, uint32_t n_res, uint32_t nbmax, uint32_t shift, const u64* block_first, const u64* d_out_off, const BlocksTab& t,
                          uint32_t* verdict, u64* count)
{
	hipLaunchKernelGGL(bk_sunits_kernel, dim3((nbmax + 255u) / 256u), dim3(256), 0, st, n_res, nbmax, shift, block_first, d_out_off, t.unit_first, t.act, t.ulen, t.ustat,
	                   t.in_off, t.in_len, t.out_off, verdict, count);
}

void launch_blocks_sverdict(hipStream_t st, uint32_t n_res, uint32_t nbmax, const uint32_t* block_crc, const BlocksTab& t, uint32_t* verdict)
{
	hipLaunchKernelGGL(bk_sverdict_kernel, dim3((nbmax + 255u) / 256u), dim3(256), 0, st, n_res, nbmax, t.unit_first, t.act, t.ulen, t.ustat, t.out_off, block_crc, t.ucrc, verdict);
}

void launch_blocks_szero(hipStream_t st, uint32_t nbmax, uint32_t shift, uint8_t* out, const BlocksTab& t, uint32_t blocks)
{
	const uint32_t ppu_shift = shift > BK_PIECE_SHIFT ? shift - BK_PIECE_SHIFT : 0u;
	const u64 items = (u64)nbmax << ppu_shift;
	hipLaunchKernelGGL(bk_szero_kernel, dim3((uint32_t)(items < blocks ? items : blocks)), dim3(CPD_THREADS), 0, st, nbmax, ppu_shift, out, t.in_off, t.act, t.ucrc);
}

void launch_blocks_sfold(hipStream_t st, uint32_t n_res, const BlocksTab& t, u64* d_out_len, uint32_t* d_bad, int32_t* d_status, u64* count)
{
	hipLaunchKernelGGL(bk_sfold_kernel, dim3((n_res + 3u) / 4u), dim3(256), 0, st, n_res, t.unit_first, t.act, t.ucrc, t.rstat, t.res_a, d_out_len, d_bad, d_status, count);
}

void launch_blocks_crcgroups(hipStream_t st, uint32_t n_res, uint32_t nbmax, uint32_t shift, const u64* res_len, const u64* block_first, const BlocksTab& t)
{
	if (nbmax == 0) { return; }
	hipLaunchKernelGGL(bk_crcgroups_kernel, dim3((nbmax + 255u) / 256u), dim3(256), 0, st, n_res, nbmax, shift, res_len, block_first, t.in_len, t.act, t.ulen);
}

void launch_blocks_ktables(hipStream_t st, uint32_t n_res, uint32_t nbmax, uint32_t shift, u64 in_max, const u64* res_len, const u64* block_first,
                           const u64* range, const u64* d_out_off, const int32_t* d_status, const BlocksTab& t)
{
	hipLaunchKernelGGL(bk_kres_kernel, dim3(1), dim3(DV_THREADS), 0, st, n_res, nbmax, shift, in_max, res_len, block_first, range, d_status, t.unit_first, t.res_b, t.rstat);
	if (nbmax == 0) { return; }
	hipLaunchKernelGGL(bk_kunits_kernel, dim3((nbmax + 255u) / 256u), dim3(256), 0, st, n_res, nbmax, shift, res_len, block_first, d_out_off, t.unit_first, t.res_b,
	                   t.in_off, t.in_len, t.ulen);
}

void launch_blocks_kfold(hipStream_t st, uint32_t n_res, const uint32_t* read, const uint32_t* given, uint32_t words, const BlocksTab& t, u64* d_out_len, int32_t* d_status)
{
	if (n_res == 0) { return; }
	hipLaunchKernelGGL(words == 4u ? bk_kfold_kernel<4u> : bk_kfold_kernel<1u>, dim3((n_res + 3u) / 4u), dim3(256), 0, st, n_res, t.unit_first, t.ulen, read, given, t.rstat,
	                   d_out_len, d_status);
}

} // namespace msc
