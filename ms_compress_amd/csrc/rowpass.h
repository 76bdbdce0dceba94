// rowpass.h -- what the passes of the four deduper calls and of sync share (dedup.hip, diff.hip, match.hip, repair.hip, sync.hip): the
// table rules of a resource, the dense row numbering of the seed, the key table's clear, claim and find, the slices of the confirm passes,
// the settle of the refuted list, and the three run passes' frame -- a tile pass, the tile scan, a runs pass -- with the counts behind
// them. Device code only, inlined into each caller's kernels; a file keeps what is its own: what a row IS in that call, its class, and
// what a finished run writes.
#pragma once
#include "kernels.h"

namespace msc {

// ---- the key table (kernels.h KeyTable; DESIGN.md 4.13, "The key table") ----
// The walk for a key begins at the slot `at` its caller's start-slot function names (< t.slots) and goes on slot by slot, around the
// table's end; it takes t.slots steps at most, so it ends on any table, whatever a damaged one holds. A caller does its own atomicMin on
// t.min[slot], and what else follows a claim.
__device__ __forceinline__ u64 kt_key(u64 key) { return key ? key : 1u; }   // (0 is the empty slot: key 0 is kept as key 1)
// the body of a fixed grid of 256 threads a block over the slots: every slot empty, no item yet
__device__ __forceinline__ void kt_clear(const KeyTable& t)
{
	for (u64 i = (u64)blockIdx.x * 256u + threadIdx.x; i < t.slots; i += (u64)gridDim.x * 256u) { t.key[i] = 0; t.min[i] = KT_NONE; }
}
// The slot of `key`, claimed where no walk came with the key before: a 64-bit compare-and-swap on an empty slot, past the slots of other
// keys. A slot holds one key, so two items share a slot exactly when they share their key. KT_NONE: no slot in t.slots steps.
__device__ __forceinline__ uint32_t kt_claim(const KeyTable& t, u64 key, u64 at)
{
	const u64 kk = kt_key(key);
	for (u64 probe = 0; probe < t.slots; ++probe) {
		const u64 was = atomicCAS(reinterpret_cast<unsigned long long*>(&t.key[at]), 0ull, (unsigned long long)kk);
		if (was == 0 || was == kk) { return (uint32_t)at; }
		at = at + 1u == t.slots ? 0 : at + 1u;
	}
	return KT_NONE;
}
// The same walk without a write, behind the claims: the slot that holds `key`, KT_NONE when the walk meets an empty slot first -- where a
// claim of the key would have ended -- or finds none.
__device__ __forceinline__ uint32_t kt_find(const KeyTable& t, u64 key, u64 at)
{
	const u64 kk = kt_key(key);
	u64 k = 0;
	for (u64 probe = 0; probe < t.slots; ++probe) {
		k = t.key[at];
		if (k == kk || k == 0) { break; }
		at = at + 1u == t.slots ? 0 : at + 1u;
	}
	return k == kk ? (uint32_t)at : KT_NONE;                             // (a walk that ran out stands behind a slot of another key)
}

// Rules 1 and 2 for resource r of one view: 0, or the status that refuses it; f0 = its first row, n = its rows (0 when refused), L = its
// length (0 when rule 1 refuses it)
__device__ __forceinline__ int32_t view_rows(const SpliceView& v, u64 r, uint32_t shift, u64& f0, u64& n, u64& L)
{
	const u64 B = (u64)1 << shift, f1 = v.first[r + 1u], len = v.res_len[r];   // (r < n_res: the length is there whatever rule 1 says, and read with the
	f0 = v.first[r]; n = 0; L = 0;                                           // two table entries it costs no second trip to memory)
	if (f0 > f1 || f1 > v.nbt) { return -2; }                                // rule 1: MSCOMP_ARG_ERROR
	L = len;
	if (f1 - f0 != (L >> shift) + ((L & (B - 1u)) ? 1u : 0u)) { return -3; }   // rule 2: MSCOMP_DATA_ERROR
	n = f1 - f0;
	return 0;
}

// The numbering seed, one workgroup of DV_THREADS: item(i, rows, second) gives the status of item i (< n) by the caller's table rules and
// its rows, 0 for one it refuses. BOUNDS = 1: an item whose running total of rows crosses `room` is refused with MSCOMP_ARG_ERROR -- the
// total includes this item and the ones refused here; BOUNDS = 2: the items that say `second` are also held against room2, by a running
// total of their own; BOUNDS = 0: nothing is. Then status (n) and ufirst (n + 1): the rows of the items that passed, numbered densely in
// item order -- this pass's own running sum, so that a damaged block_first cannot send the row passes' search astray (bk_dres_kernel).
template <int BOUNDS, class Item>
__device__ __forceinline__ void seed_numbering(uint32_t n, u64 room, u64 room2, u64* __restrict__ ufirst, int32_t* __restrict__ status, Item item)
{
	constexpr int NB = BOUNDS > 1 ? BOUNDS : 1;
	__shared__ u64 s_w[NB][DV_WAVES];
	const uint32_t tid = threadIdx.x;
	u64 run[NB] = {}, kept[1] = {0};
	if (tid == 0) { ufirst[0] = 0; }
	for (uint32_t base = 0; base < n; base += DV_THREADS) {
		const uint32_t i = base + tid;
		const bool live = i < n;
		u64 rows = 0;
		bool second = false;
		int32_t st = 0;
		if (live) { st = item(i, rows, second); }
		if (BOUNDS > 0) {
			u64 t[NB];
			t[0] = rows;
			if (BOUNDS > 1) { t[NB - 1] = second ? rows : 0; }
			dv_block_scan<NB>(t, run, s_w);
			if (rows && (t[0] > room || (BOUNDS > 1 && second && t[NB - 1] > room2))) { st = -2; rows = 0; }
		}
		u64 a[1] = {rows};
		dv_block_scan<1>(a, kept, s_w);
		if (live) { ufirst[i + 1u] = a[0]; status[i] = st; }
	}
}

// The slices of a confirm pass: the (row, piece of 16 KiB) items of a numbering of `units` rows, cut into equal slices, one per workgroup
// of a fixed grid; a workgroup walks the rows of its slice and calls row(u, at, upto) for row u's stored bytes [at, upto) -- the pieces of
// the row in this slice as one stretch. What a caller has to look up per owner it keeps in its functor, until u passes the owner's end.
template <class Row>
__device__ __forceinline__ void confirm_slices(u64 units, uint32_t ppu_shift, Row row)
{
	const u64 items = units << ppu_shift;
	u64 per = (items + gridDim.x - 1u) / gridDim.x;
	per = per < DD_SLICE_MIN ? DD_SLICE_MIN : per;
	const u64 lo = (u64)blockIdx.x * per;
	if (lo >= items) { return; }
	const u64 hi = items - lo < per ? items : lo + per;
	for (u64 i = lo; i < hi; ) {
		const u64 u = i >> ppu_shift, next = (u + 1u) << ppu_shift, end = next < hi ? next : hi;   // the row's items in this slice: [i, end)
		// (a row's last piece runs to the end of the row: nothing bounds a stored length but packed_len, so a row of a damaged table that passes
		// the row rule may be longer than its pieces -- one workgroup then takes the rest)
		const u64 at = (i - (u << ppu_shift)) << DD_PIECE_SHIFT, upto = end == next ? ~(u64)0 : (end - (u << ppu_shift)) << DD_PIECE_SHIFT;
		i = end;
		row(u, at, upto);
	}
}

// The settle of a refuted list (one workgroup; rlist: nref entries, ascending, each its own representative to begin with). The refuted are
// answered exactly, one after the other: equal ones share their key, so the only ones a refuted one can still be equal to are the earlier
// refuted ones of its slot that stayed their own representative. equal(g, c): by the whole block, the same answer in every thread.
template <class R, class Equal>
__device__ __forceinline__ void settle_refuted(const uint32_t* rlist, u64 nref, const uint32_t* __restrict__ slot_of, R* rep, Equal equal)
{
	const uint32_t tid = threadIdx.x;
	__syncthreads();                                                     // rlist and rep are read back below, by other threads of this block
	for (u64 i = 0; i < nref; ++i) {
		const uint32_t g = rlist[i];
		uint32_t to = g;
		for (u64 j = 0; j < i; ++j) {
			const uint32_t c = rlist[j];
			if (slot_of[c] == slot_of[g] && rep[c] == c && equal(g, c)) { to = c; break; }
		}
		__syncthreads();                                                   // (every thread has read rep before one of them writes it)
		if (tid == 0) { rep[g] = to; }
		__syncthreads();
	}
}

// The run passes, tiled: tile b of ROW_TILE rows has eight words in tsum -- NS sums, then 8 - NS maxima, the first of them the last row of
// the tile that starts a run, + 1 (0: the tile has none). A tile pass leaves them per tile, rows_tilescan_kernel<NS, ..> turns them into
// their running values, and a runs pass goes over the rows again with the values in front of its tile: the row that ENDS a run writes the
// run, whole -- its first row is the running maximum of the rows that start one, so its length and first block need no second look at the
// rows between. K: the sums a pass scans itself.
template <int K>
struct RunScan {
	// The tile pass's tail, behind the caller's scan: the block's maxima of m[] and the tile's words -- sum[] (the totals the scan left), zeros
	// up to NS, the maxima, zeros up to 8. s_m: DV_WAVES words of LDS.
	template <int NS, int M>
	static __device__ __forceinline__ void tile(u64* __restrict__ tsum, const u64 (&sum)[K], u64 (&m)[M], u64* s_m)
	{
		static_assert(K <= NS && NS + M <= 8, "eight words per tile");
		u64 c[M] = {};
		#pragma unroll
		for (int j = 0; j < M; ++j) { dv_block_max(m[j], c[j], s_m); }
		if (threadIdx.x == 0) {
			u64* t = tsum + 8u * (u64)blockIdx.x;
			#pragma unroll
			for (int i = 0; i < K; ++i) { t[i] = sum[i]; }
			#pragma unroll
			for (int i = K; i < NS; ++i) { t[i] = 0; }
			#pragma unroll
			for (int j = 0; j < M; ++j) { t[NS + j] = c[j]; }
			#pragma unroll
			for (int i = NS + M; i < 8; ++i) { t[i] = 0; }
		}
	}

	// The runs pass's head: own[] -- what row `row` adds to the K counts, own[0] = 1 when it starts a run -- scanned behind the counts in front
	// of the tile. Returns the last row at or in front of `row` that starts a run, + 1; a[]: the counts up to and including the row.
	template <int NS>
	static __device__ __forceinline__ u64 head(const u64* __restrict__ tsum, u64 row, const u64 (&own)[K], u64 (&a)[K], u64 (*s_w)[DV_WAVES])
	{
		const u64* before = tsum + 8u * (u64)(blockIdx.x ? blockIdx.x - 1u : 0u);
		u64 sum[K] = {}, c0 = 0;
		#pragma unroll
		for (int i = 0; i < K; ++i) { a[i] = own[i]; }
		if (blockIdx.x) {
			#pragma unroll
			for (int i = 0; i < K; ++i) { sum[i] = before[i]; }
			c0 = before[NS];
		}
		dv_block_scan<K>(a, sum, s_w);
		u64 m0 = own[0] ? row + 1u : 0;
		dv_block_max(m0, c0, s_w[0]);
		return m0;
	}
	// behind it, the first row of an owner: the counts in front of it into the owner's K words of pfirst, for the counts pass
	static __device__ __forceinline__ void front(u64* __restrict__ pf, const u64 (&a)[K], const u64 (&own)[K])
	{
		#pragma unroll
		for (int i = 0; i < K; ++i) { pf[i] = a[i] - own[i]; }
	}
};

// The running sums and maxima of the tiles' words, in place (one workgroup): words [0, NS) are sums, [NS, 8) maxima, one or two. CARRY >= 0:
// the last maximum is a count within its tile of sum CARRY, + 1 (0: the tile has none), and becomes a count over the whole numbering --
// what lies in front of the tile is added (diff: the changed blocks in front of a pair's first row). CARRY < 0: a plain maximum.
// (The maxima are two scalars, not an array: as an array the compiler keeps the six-sum instance in 151 spilled scalar registers.)
template <int NS, int CARRY>
__global__ __launch_bounds__(DV_THREADS) void rows_tilescan_kernel(uint32_t tiles, u64* tsum)
{
	constexpr int NM = 8 - NS, CW = CARRY >= 0 ? CARRY : 0;
	static_assert((NM == 1 || NM == 2) && CARRY < NS, "seven sums and a maximum, or six and two");
	__shared__ u64 s_w[NS][DV_WAVES];
	u64 run[NS] = {}, c0 = 0, c1 = 0;
	for (uint32_t at = 0; at < tiles; at += DV_THREADS) {
		const uint32_t g = at + threadIdx.x;
		const bool live = g < tiles;
		u64 a[NS], m0 = 0, m1 = 0;
		#pragma unroll
		for (uint32_t i = 0; i < (uint32_t)NS; ++i) { a[i] = live ? tsum[8u * g + i] : 0; }
		const u64 own = a[CW];
		if (live) { m0 = tsum[8u * g + NS]; if (NM > 1) { m1 = tsum[8u * g + 7u]; } }
		dv_block_scan<NS>(a, run, s_w);
		if (CARRY >= 0 && m1) { m1 += a[CW] - own; }                       // what lies in front of the tile
		dv_block_max(m0, c0, s_w[0]);
		if (NM > 1) { dv_block_max(m1, c1, s_w[0]); }
		if (live) {
			#pragma unroll
			for (uint32_t i = 0; i < (uint32_t)NS; ++i) { tsum[8u * g + i] = a[i]; }
			tsum[8u * g + NS] = m0; if (NM > 1) { tsum[8u * g + 7u] = m1; }
		}
	}
}

// The counts pass: what is in front of the owner whose first row is `row` -- K counts -- is what that row left in pfirst; `row` being the
// first row of the next owner that has rows, for an owner without; or the totals tot[] behind the last row (row >= units).
template <int K, int T>
__device__ __forceinline__ void counts_in_front(const u64* __restrict__ ufirst, uint32_t n, u64 units, const u64* __restrict__ pfirst, const u64 (&tot)[T], u64 row, u64 (&out)[K])
{
	static_assert(K <= T, "the totals begin with the K counts");
	const bool behind = row >= units;                                       // (chosen by value: a pointer chosen between tot and pfirst puts tot into scratch memory)
	const u64* f = pfirst + (u64)K * (behind ? 0u : res_of_block(ufirst, n, row));
	#pragma unroll
	for (int j = 0; j < K; ++j) { const u64 t = tot[j]; out[j] = behind ? t : f[j]; }
}

} // namespace msc
