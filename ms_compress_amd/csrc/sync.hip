// sync.hip -- the passes of a block syncer (mscomp_amd_syncer_*, include/mscomp_amd.h): raw new data in HBM against the block checksums of
// ONE store container, at every byte offset. d_block_crc is the signature rsync would send; the CRC-32 of the B-byte window at position p
// of a unit M is, by the algebra of crcmath.h,
//   crc32(M[p : p + B]) = W(p) ^ crc_seed(B),   W(p) = raw(M[p : p + B]) = raw(M[: p + B]) ^ raw(M[: p]) x^(8B)
// and W rolls: W(p + 1) = W(p) x^8 ^ raw(M[p + B]) ^ raw(M[p]) x^(8B) -- two table lookups per position, t0[(W ^ hi) & 255] and tb[lo].
// The boundary passes leave raw(M[: q]) at every 64th byte, so every lane of the scan starts a run of 64 positions from two words; the
// scan walks the positions twice (a tile pass that counts, a runs pass that writes), with a tile scan between them, and stores nothing
// per position. The store's words lie in the key table dedup and match use (rowpass.h kt_*). Candidates are confirmed against the rows the reader core decodes (reader.hip, unchanged) -- or, by a digest syncer,
// by the BLAKE2s digest of their window against the store's digest column (digest.hip), without a stored byte. DESIGN.md 4.20, 4.21.
#include "rowpass.h"
#include "crcmath.h"

namespace msc {

#define SY_THREADS 256u                                   // four waves, a tile each
#define SY_NONE    0xFFFFFFFFu                            // a lane of the scan: no position of it starts a segment
#define SY_X       0xFFFFFFFEu                            // the state in front of a lane's first position: no state (a state is 0, or a row + 1)
#define SY_BMASK   ((1u << SYNC_BITS_LOG) - 1u)            // a word's two bits of the bitmap: at its low and at its high SYNC_BITS_LOG bits
#define SY_BHIGH   (32u - SYNC_BITS_LOG)
// the words of a tile (t.tword, eight per tile). From the tile pass:
#define SW_RAW   0u                                       // raw candidates
#define SW_LOCAL 1u                                       // thinned candidates of the runs that start inside the tile, behind its first position
#define SW_MAX   2u                                       // the last position behind the tile's first that starts a segment, as a tile coordinate + 1 (0: none)
#define SW_EDGE  3u                                       // state of the first position | state of the last one << 32
#define SW_EXT   4u                                       // positions of the tile's first segment
// ... and from the tile scan:
#define SW_BASE  5u                                       // thinned candidates in front of the tile
#define SW_ENTER 6u                                       // where the segment of the tile's first position starts, as a tile coordinate + 1

// ---- the store: key table and bitmap ----
// the key of word w (never 0), and where its walk begins: the table has a power of two of slots, 2^(32 - slot_shift)
__device__ __forceinline__ u64 sy_key(uint32_t w) { return (u64)w | (u64)1 << 32; }
__device__ __forceinline__ u64 sy_slot(uint32_t w, uint32_t slot_shift) { return slot_shift >= 32u ? 0u : (u64)((w * 0x9E3779B1u) >> slot_shift); }
// whether the bitmap may hold word w: two bits, at the word's low and at its high bits (the second is read only behind a set first)
__device__ __forceinline__ bool sy_maybe(const uint32_t* s_bits, uint32_t w)
{
	if (!((s_bits[(w & SY_BMASK) >> 5] >> (w & 31u)) & 1u)) { return false; }
	return (s_bits[(w >> SY_BHIGH) >> 5] >> ((w >> SY_BHIGH) & 31u)) & 1u;
}
__global__ __launch_bounds__(256) void sy_clear_kernel(SyncTab t)
{
	kt_clear(t.kt);
	for (u64 i = (u64)blockIdx.x * 256u + threadIdx.x; i < SYNC_BIT_WORDS; i += (u64)gridDim.x * 256u) { t.bits[i] = 0; }
}

// Seed, one block: view_rows' rules 1 and 2 per resource, the status, and ufirst (n + 1). No room rule: nothing of the syncer is sized
// per row but the key table, and the walk along it is bounded by its slots.
__global__ __launch_bounds__(DV_THREADS) void sy_seed_kernel(SpliceView v, uint32_t n, uint32_t shift, u64* __restrict__ ufirst, int32_t* __restrict__ status)
{
	seed_numbering<0>(n, 0, 0, ufirst, status, [&](uint32_t g, u64& rows, bool&) {
		u64 f0, L;
		return view_rows(v, g, shift, f0, rows, L);
	});
}

// Keys, a fixed grid dealt over the rows (mt_keys_kernel's scheme): an eligible row -- B bytes of data -- of an accepted resource claims
// its word's slot of the key table, puts its number into the slot's minimum and sets the word's two bits. The word is the CRC word with
// the seed of a B-byte message taken off: what the scan rolls.
__global__ __launch_bounds__(256) void sy_keys_kernel(SpliceView v, uint32_t n, uint32_t shift, SyncTab t, const int32_t* __restrict__ status)
{
	const u64 units = t.ufirst[n];
	const uint32_t seed = t.consts[5u * 256u];
	for (u64 u = (u64)blockIdx.x * 256u + threadIdx.x; u < units; u += (u64)gridDim.x * 256u) {
		const uint32_t x = res_of_block(t.ufirst, n, u);
		if (status[x] != 0) { continue; }
		const u64 k = u - t.ufirst[x];
		if (((k + 1u) << shift) > v.res_len[x]) { continue; }                // the short last block never takes part
		const uint32_t w = v.crc[v.first[x] + k] ^ seed;                     // (first[x] + k < first[x + 1] <= v.nbt: rule 1)
		const uint32_t slot = kt_claim(t.kt, sy_key(w), sy_slot(w, t.slot_shift));
		if (slot == KT_NONE) { continue; }
		atomicMin(&t.kt.min[slot], (uint32_t)u);
		atomicOr(&t.bits[(w & SY_BMASK) >> 5], 1u << (w & 31u)); atomicOr(&t.bits[(w >> SY_BHIGH) >> 5], 1u << ((w >> SY_BHIGH) & 31u));
	}
}

// the row + 1 the table holds for word w, 0 when it holds none (the rare path of the scan: only behind a set bit; a function of its own,
// called: inlined, its walk would take its registers from the sweep's)
__device__ __noinline__ uint32_t sy_probe(KeyTable kt, uint32_t slot_shift, uint32_t w)
{
	const uint32_t slot = kt_find(kt, sy_key(w), sy_slot(w, slot_shift));
	if (slot == KT_NONE) { return 0; }
	const uint32_t r = kt.min[slot];
	return r >= 0x7FFFFFF0u ? 0u : r + 1u;
}

// ---- the units ----
// One block: the dev plans' bounds rule (a unit whose running total of in_len exceeds in_max is refused, an empty unit from there on), and
// the numberings: cum, pfirst, tfirst (n + 1 each). A unit shorter than B has no piece and no tile: no window fits into it.
__global__ __launch_bounds__(DV_THREADS) void sy_units_kernel(uint32_t n, uint32_t shift, u64 in_max, const u64* __restrict__ in_off, const u64* __restrict__ in_len,
                                                             SyncTab t, int32_t* __restrict__ status)
{
	__shared__ u64 s_w[3][DV_WAVES];
	const uint32_t tid = threadIdx.x;
	const u64 B = (u64)1 << shift;
	u64 run[1] = {0}, acc[3] = {0, 0, 0};
	if (tid == 0) { t.cum[0] = 0; t.pfirst[0] = 0; t.tfirst[0] = 0; }
	for (uint32_t base = 0; base < n; base += DV_THREADS) {
		const uint32_t i = base + tid;
		const bool live = i < n;
		const u64 len = live ? in_len[i] : 0;
		u64 r[1] = {len};
		dv_block_scan<1>(r, run, s_w);
		const bool rej = live && r[0] > in_max;
		const u64 L = rej ? 0 : len;
		const bool big = L >= B;
		u64 a[3] = {L, big ? L / SYNC_RUN + 1u : 0u, big ? L / SYNC_TILE + 1u : 0u};
		dv_block_scan<3>(a, acc, s_w);
		if (live) {
			t.cum[i + 1u] = a[0]; t.pfirst[i + 1u] = a[1]; t.tfirst[i + 1u] = a[2];
			t.uoff[i] = rej ? 0 : in_off[i]; t.ulen[i] = L; status[i] = rej ? -2 : 0;   // MSCOMP_ARG_ERROR
		}
	}
}

// ---- the boundaries ----
// A wave per tile, crc_part's layout: lane l takes the piece at 64 l -- four 16-byte loads of any alignment, the last piece of a unit byte
// by byte --, the lanes combine by constant multiplications (a running value over the lanes, the factor of distance 2^s being
// x^(512 2^s)). pabs gets raw(tile[: 64 l]), traw raw(tile) -- of a whole tile; no other one's is read.
__global__ __launch_bounds__(SY_THREADS) void sy_piece_kernel(uint32_t n, const uint8_t* __restrict__ in, SyncTab t)
{
	__shared__ uint32_t s_t[16][256];
	const uint32_t tid = threadIdx.x, lane = tid & 63u;
	for (uint32_t i = tid; i < 16u * 256u; i += SY_THREADS) { (&s_t[0][0])[i] = (&g_crc_tab.t[0][0])[i]; }
	__syncthreads();
	const u64 ntiles = t.tfirst[n];
	for (u64 i = (u64)blockIdx.x * 4u + (tid >> 6); i < ntiles; i += (u64)gridDim.x * 4u) {
		const uint32_t u = res_of_block(t.tfirst, n, i);
		const u64 k = i - t.tfirst[u], L = t.ulen[u], start = (k * 64u + lane) * SYNC_RUN;
		const bool exists = start <= L;
		uint32_t r = 0;
		if (exists) {
			const uint8_t* __restrict__ p = in + t.uoff[u] + start;
			if (L - start >= SYNC_RUN) {
				const cpd_u16* __restrict__ q = reinterpret_cast<const cpd_u16*>(p);
				const cpd_u16 v0 = q[0], v1 = q[1], v2 = q[2], v3 = q[3];
				r = crc_step16(s_t, r, make_uint4(v0.w[0], v0.w[1], v0.w[2], v0.w[3])); r = crc_step16(s_t, r, make_uint4(v1.w[0], v1.w[1], v1.w[2], v1.w[3]));
				r = crc_step16(s_t, r, make_uint4(v2.w[0], v2.w[1], v2.w[2], v2.w[3])); r = crc_step16(s_t, r, make_uint4(v3.w[0], v3.w[1], v3.w[2], v3.w[3]));
			} else {
				for (uint32_t j = 0; j < (uint32_t)(L - start); ++j) { r = (r >> 8) ^ s_t[0][(r ^ p[j]) & 255u]; }
			}
		}
		uint32_t v = r;
		#pragma unroll
		for (uint32_t s = 0; s < 6u; ++s) {
			const uint32_t o = __shfl_up(v, 1u << s, 64);
			if (lane >= (1u << s) && o != 0) { v ^= crc_mul(o, g_crc_tab.x2n[9u + s]); }
		}
		uint32_t ex = __shfl_up(v, 1u, 64);
		if (lane == 0) { ex = 0; }
		if (exists) { t.pabs[t.pfirst[u] + k * 64u + lane] = ex; }             // (piece 64 k + lane <= L / 64: inside the unit's L / 64 + 1)
		if (lane == 63u) { t.traw[i] = v; }
	}
}

// One block: traw[i] = raw(unit[: tile i]), the running value of the tiles' raw() along every unit (factor of distance 2^s: x^(8 T 2^s)).
// 1023 tiles per step; slot 0 carries the tile in front of them.
__global__ __launch_bounds__(DV_THREADS) void sy_pre_kernel(uint32_t n, SyncTab t)
{
	__shared__ uint32_t s_v[DV_THREADS];
	const uint32_t tid = threadIdx.x;
	const u64 ntiles = t.tfirst[n];
	uint32_t carry = 0;
	for (u64 c0 = 0; c0 < ntiles; c0 += DV_THREADS - 1u) {
		const long long i = (long long)c0 + (long long)tid - 1;               // slot tid holds tile i
		const bool live = tid >= 1u && (u64)i < ntiles;
		long long seg = 0;
		uint32_t v = tid == 0 ? carry : 0u;
		if (live) { seg = (long long)t.tfirst[res_of_block(t.tfirst, n, (u64)i)]; v = t.traw[i]; }
		s_v[tid] = v;
		__syncthreads();
		for (uint32_t s = 0; s < 10u; ++s) {
			const uint32_t d = 1u << s;
			const uint32_t o = live && tid >= d && i - (long long)d >= seg ? s_v[tid - d] : 0u;
			__syncthreads();
			if (o != 0) { v ^= crc_mul(o, g_crc_tab.x2n[15u + s]); }
			s_v[tid] = v;
			__syncthreads();
		}
		if (live) { t.traw[i] = i == seg ? 0u : s_v[tid - 1u]; }
		if (tid == 0) { carry = s_v[DV_THREADS - 1u]; }
		__syncthreads();
	}
}

// pabs[piece] = raw(unit[: piece]): what lies in front of the tile, carried over the tile's pieces in front of this one
__global__ __launch_bounds__(SY_THREADS) void sy_abs_kernel(uint32_t n, SyncTab t)
{
	__shared__ uint32_t s_c[64];
	const uint32_t tid = threadIdx.x, lane = tid & 63u;
	if (tid < 64u) { s_c[tid] = crc_xpow((u64)(8u * SYNC_RUN) * tid); }
	__syncthreads();
	const u64 ntiles = t.tfirst[n];
	for (u64 i = (u64)blockIdx.x * 4u + (tid >> 6); i < ntiles; i += (u64)gridDim.x * 4u) {
		const uint32_t pre = t.traw[i];
		if (pre == 0) { continue; }
		const uint32_t u = res_of_block(t.tfirst, n, i);
		const u64 k = i - t.tfirst[u];
		if ((k * 64u + lane) * SYNC_RUN <= t.ulen[u]) { t.pabs[t.pfirst[u] + k * 64u + lane] ^= crc_mul(pre, s_c[lane]); }
	}
}

// ---- the scan ----
// What a lane knows of its run of positions behind a sweep. A STATE is 0 (no raw candidate) or the candidate's row + 1; a SEGMENT is a
// maximal stretch of positions of one state.
struct SyLane {
	uint32_t f, l;                                         // state of the first and of the last position
	uint32_t lead, last;                                   // positions of the first segment; the last position behind the first that starts a segment (SY_NONE: none)
	uint32_t nraw, nint;                                   // raw candidates; candidate segments that start behind the first position
	uint32_t q0, q1, r0, r1;                               // the first two of those: position in the run, state
};
struct SyEmit { u64 rank, g0, ncand, unit0; uint32_t unit; };   // MODE 2: where the lane's candidate segments go

__device__ __forceinline__ void sy_put(const SyncTab& t, const SyEmit& e, u64 rank, u64 g, uint32_t row)
{
	if (rank < e.ncand) { t.cunit[rank] = e.unit; t.cpos[rank] = g - e.unit0; t.crow[rank] = row; }
}

// One lane's sweep over nvalid <= 64 positions from the window register W of the first one; lo = the first position's byte, the windows'
// last bytes lie B further on. Sixteen positions per step of loads: of the bytes only those in front of the last position are needed,
// and only they are read. MODE 0: count. MODE 1: also remember the first two candidate segments that start behind the first position.
// MODE 2: write them all, from rank e.rank on.
template <int MODE>
__device__ __forceinline__ void sy_sweep(const uint32_t* s_t0, const uint32_t* s_tb, const uint32_t* s_bits, const SyncTab& t, const uint8_t* __restrict__ lo,
                                         u64 B, uint32_t nvalid, uint32_t W, SyLane& z, const SyEmit& e)
{
	z.f = 0; z.l = 0; z.lead = nvalid; z.last = SY_NONE; z.nraw = 0; z.nint = 0; z.q0 = z.q1 = z.r0 = z.r1 = 0;
	const uint8_t* __restrict__ hi = lo + B;
	const uint32_t steps = nvalid ? nvalid - 1u : 0u;
	uint32_t prev = SY_X;
	#pragma unroll 1
	for (uint32_t i0 = 0; i0 < nvalid; i0 += 16u) {
		uint32_t a[4] = {0, 0, 0, 0}, b[4] = {0, 0, 0, 0};
		if (i0 + 16u <= steps) {
			const cpd_u16 x = *reinterpret_cast<const cpd_u16*>(lo + i0), y = *reinterpret_cast<const cpd_u16*>(hi + i0);
			a[0] = x.w[0]; a[1] = x.w[1]; a[2] = x.w[2]; a[3] = x.w[3]; b[0] = y.w[0]; b[1] = y.w[1]; b[2] = y.w[2]; b[3] = y.w[3];
		} else {
			for (uint32_t j = 0; i0 + j < steps; ++j) { a[j >> 2] |= (uint32_t)lo[i0 + j] << (8u * (j & 3u)); b[j >> 2] |= (uint32_t)hi[i0 + j] << (8u * (j & 3u)); }
		}
		#pragma unroll
		for (uint32_t j = 0; j < 16u; ++j) {
			const uint32_t i = i0 + j;
			const bool live = i < nvalid;
			uint32_t st = 0;
			if (live && sy_maybe(s_bits, W)) {
				st = sy_probe(t.kt, t.slot_shift, W);
				if (st) { ++z.nraw; }
			}
			if (live && st != prev) {
				if (i == 0) { z.f = st; }
				else {
					if (z.last == SY_NONE) { z.lead = i; }
					z.last = i;
					if (st) {
						if (MODE == 2) { sy_put(t, e, e.rank + z.nint, e.g0 + i, st - 1u); }
						else if (MODE == 1) { if (z.nint == 0) { z.q0 = i; z.r0 = st; } else if (z.nint == 1u) { z.q1 = i; z.r1 = st; } }
						++z.nint;
					}
				}
				prev = st;
			}
			const uint32_t lb = (a[j >> 2] >> (8u * (j & 3u))) & 255u, hb = (b[j >> 2] >> (8u * (j & 3u))) & 255u;
			W = (W >> 8) ^ s_t0[(W ^ hb) & 255u] ^ s_tb[lb];
		}
	}
	z.l = prev == SY_X ? 0u : prev;
}

// Both passes over the positions (RunScan's tile pass and runs pass, a wave per tile). The tile pass leaves the tile's words. The runs
// pass, with what the tile scan added -- the thinned candidates in front of the tile and where the segment of its first position starts
// --, ranks the thinned candidates and writes those below n_cand_max: of a run of one row that starts at p0 the positions p0 + i B. A
// lane's positions are fewer than B, so of the segment that reaches into the lane at most one position survives, and of every segment
// that starts in the lane exactly its first. A lane remembers two such starts; a wave in which a lane has more (periodic data) sweeps
// again and writes them as it meets them.
template <bool WRITE>
__global__ __launch_bounds__(SY_THREADS) void sy_scan_kernel(uint32_t n, uint32_t ncand, uint32_t shift, const uint8_t* __restrict__ in, SyncTab t)
{
	__shared__ uint32_t s_t0[256];
	__shared__ uint32_t s_c[5u * 256u];                                   // tb, then mb[4]
	__shared__ uint32_t s_bits[SYNC_BIT_WORDS];
	const uint32_t tid = threadIdx.x, lane = tid & 63u;
	for (uint32_t i = tid; i < 256u; i += SY_THREADS) { s_t0[i] = g_crc_tab.t[0][i]; }
	for (uint32_t i = tid; i < 5u * 256u; i += SY_THREADS) { s_c[i] = t.consts[i]; }
	for (uint32_t i = tid; i < SYNC_BIT_WORDS; i += SY_THREADS) { s_bits[i] = t.bits[i]; }
	__syncthreads();
	const uint32_t* s_tb = s_c;
	const uint32_t* s_mb = s_c + 256u;
	const u64 B = (u64)1 << shift, ntiles = t.tfirst[n];
	for (u64 i = (u64)blockIdx.x * 4u + (tid >> 6); i < ntiles; i += (u64)gridDim.x * 4u) {
		const uint32_t u = res_of_block(t.tfirst, n, i);
		const u64 k = i - t.tfirst[u], L = t.ulen[u];
		const uint32_t a_off = lane * SYNC_RUN;
		const u64 p = k * SYNC_TILE + a_off, G = i * SYNC_TILE + a_off;
		uint32_t nvalid = 0, W0 = 0;
		if (p + B <= L) {                                                    // (L >= B: the unit has tiles)
			const u64 avail = L - B - p, q = t.pfirst[u] + k * 64u + lane;
			nvalid = avail + 1u < SYNC_RUN ? (uint32_t)avail + 1u : SYNC_RUN;
			const uint32_t A = t.pabs[q];                                      // (p <= p + B <= L: both boundaries are the unit's)
			W0 = t.pabs[q + (B >> 6)] ^ s_mb[A & 255u] ^ s_mb[256u + ((A >> 8) & 255u)] ^ s_mb[512u + ((A >> 16) & 255u)] ^ s_mb[768u + (A >> 24)];
		}
		const uint8_t* lo = in + t.uoff[u] + p;
		SyEmit e = { 0, G, ncand, t.tfirst[u] * SYNC_TILE, u };
		SyLane z;
		sy_sweep<WRITE ? 1 : 0>(s_t0, s_tb, s_bits, t, lo, B, nvalid, W0, z, e);
		const bool valid = nvalid != 0;
		const uint32_t prev_l = __shfl_up(z.l, 1u, 64);
		const bool sf = lane > 0 && valid && z.f != prev_l;                   // the lane's first position starts a segment (lane 0: the tile scan's to say)
		u64 m = z.last != SY_NONE ? G + z.last + 1u : sf ? G + 1u : 0u;
		if (!WRITE) {
			const auto sum = [](uint32_t a, uint32_t b) { return a + b; };
			const uint32_t raw = wave_all(z.nraw, sum), loc = wave_all(z.nint + (sf && z.f ? 1u : 0u), sum), nvt = wave_all(nvalid, sum);
			const uint32_t nvl = (uint32_t)__popcll(__ballot(valid));
			const u64 mx = wave_all(m, [](u64 a, u64 b) { return b > a ? b : a; });
			uint32_t ext = wave_all(!valid ? SY_NONE : sf ? a_off : z.last != SY_NONE ? a_off + z.lead : SY_NONE, [](uint32_t a, uint32_t b) { return b < a ? b : a; });
			ext = ext < nvt ? ext : nvt;
			const uint32_t F = __shfl(z.f, 0, 64), Lst = __shfl(z.l, nvl ? (int)nvl - 1 : 0, 64);
			if (lane == 0) {
				u64* w = t.tword + 8u * i;
				w[SW_RAW] = raw; w[SW_LOCAL] = loc; w[SW_MAX] = mx; w[SW_EDGE] = (u64)F | (u64)Lst << 32; w[SW_EXT] = ext; w[SW_BASE] = 0; w[SW_ENTER] = 0; w[7] = 0;
			}
		} else {
			const u64 enter = t.tword[8u * i + SW_ENTER], base = t.tword[8u * i + SW_BASE];
			if (lane == 0 && enter > m) { m = enter; }
			u64 inc = m;
			#pragma unroll
			for (uint32_t d = 1; d < 64u; d <<= 1) { const u64 o = __shfl_up(inc, d, 64); if (lane >= d && o > inc) { inc = o; } }
			u64 exc = __shfl_up(inc, 1u, 64);
			if (lane == 0) { exc = enter; }
			uint32_t lk = 0;
			u64 first = 0;
			if (valid && z.f != 0 && (sf || exc != 0)) {
				const u64 p0 = sf ? G : exc - 1u;                                // where the run of the lane's first position starts
				first = p0 + (((G - p0) + B - 1u) >> shift << shift);
				lk = first < G + z.lead ? 1u : 0u;
			}
			const uint32_t kept = lk + z.nint;
			uint32_t ex = kept;
			#pragma unroll
			for (uint32_t d = 1; d < 64u; d <<= 1) { const uint32_t o = __shfl_up(ex, d, 64); if (lane >= d) { ex += o; } }
			e.rank = base + (ex - kept);
			if (lk) { sy_put(t, e, e.rank, first, z.f - 1u); }
			e.rank += lk;
			if (__ballot(z.nint > 2u) == 0) {
				if (z.nint >= 1u) { sy_put(t, e, e.rank, G + z.q0, z.r0 - 1u); }
				if (z.nint >= 2u) { sy_put(t, e, e.rank + 1u, G + z.q1, z.r1 - 1u); }
			} else {
				SyLane z2;
				sy_sweep<2>(s_t0, s_tb, s_bits, t, lo, B, nvalid, W0, z2, e);
			}
		}
	}
}

// The tile scan, one block, between the two passes: whether a tile's first position starts a segment (its state against the last state of
// the tile in front, within a unit), the running maximum of the segment starts, the thinned candidates of the tile's first segment --
// which need the start of its run --, and the running sums. count[0 .. 2]: raw, thinned, kept.
__global__ __launch_bounds__(DV_THREADS) void sy_tilescan_kernel(uint32_t n, uint32_t ncand, uint32_t shift, SyncTab t)
{
	__shared__ u64 s_w[2][DV_WAVES];
	__shared__ u64 s_inc[DV_THREADS];
	const uint32_t tid = threadIdx.x;
	const u64 B = (u64)1 << shift, ntiles = t.tfirst[n];
	u64 carry = 0, sums[2] = {0, 0};
	for (u64 base = 0; base < ntiles; base += DV_THREADS) {
		const u64 i = base + tid, g0 = i * SYNC_TILE;
		const bool live = i < ntiles;
		u64 raw = 0, loc = 0, mx = 0, ext = 0;
		uint32_t F = 0;
		bool s0 = true;
		if (live) {
			const u64* w = t.tword + 8u * i;
			raw = w[SW_RAW]; loc = w[SW_LOCAL]; mx = w[SW_MAX]; ext = w[SW_EXT]; F = (uint32_t)w[SW_EDGE];
			const uint32_t u = res_of_block(t.tfirst, n, i);
			if (i != t.tfirst[u]) { s0 = F != (uint32_t)(t.tword[8u * (i - 1u) + SW_EDGE] >> 32); }
			if (s0 && g0 + 1u > mx) { mx = g0 + 1u; }
		}
		const u64 before = carry;
		u64 v = mx;
		dv_block_max(v, carry, s_w[0]);
		s_inc[tid] = v;
		__syncthreads();
		const u64 enter = s0 ? g0 + 1u : tid ? s_inc[tid - 1u] : before;
		__syncthreads();
		u64 c0 = 0;
		if (live && F != 0 && enter != 0) {
			const u64 p0 = enter - 1u, first = p0 + (((g0 - p0) + B - 1u) >> shift << shift);
			if (first < g0 + ext) { c0 = 1u + ((g0 + ext - 1u - first) >> shift); }
		}
		const u64 thin = loc + c0;
		u64 a[2] = {raw, thin};
		dv_block_scan<2>(a, sums, s_w);
		if (live) { t.tword[8u * i + SW_BASE] = a[1] - thin; t.tword[8u * i + SW_ENTER] = enter; }
	}
	if (tid == 0) { t.count[0] = sums[0]; t.count[1] = sums[1]; t.count[2] = sums[1] < ncand ? sums[1] : ncand; }
}

// ---- confirm ----
// One thread per slot of the kept list: the request (r, k B, B) of a kept candidate's row for the reader core, which decodes every
// distinct row once; a slot behind the kept ones asks for a resource that does not exist and so for nothing. The flags cleared.
__global__ __launch_bounds__(256) void sy_req_kernel(uint32_t n, uint32_t ncand, uint32_t shift, SyncTab t)
{
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= ncand) { return; }
	u64 r = ~(u64)0, o = 0, l = 0;
	if (i < t.count[2]) {
		const u64 row = t.crow[i];
		if (row < t.ufirst[n]) { const uint32_t x = res_of_block(t.ufirst, n, row); r = x; o = (row - t.ufirst[x]) << shift; l = (u64)1 << shift; }
	}
	t.req[3u * (u64)i] = r; t.req[3u * (u64)i + 1u] = o; t.req[3u * (u64)i + 2u] = l; t.flag[i] = 0;
}

// The compare (confirm_slices over the kept candidates, pieces of 16 KiB): the B bytes of the unit at a candidate whose row the reader
// core judged MSCOMP_OK against that row's bytes -- its owner's cache slot, or its place in d_packed when stored raw. A mismatch sets the
// candidate's flag; every writer stores the same value.
__global__ __launch_bounds__(CPD_THREADS) void sy_confirm_kernel(uint32_t shift, uint32_t ppu_shift, const uint8_t* __restrict__ in, SyncTab t, ReaderTab r)
{
	const u64 B = (u64)1 << shift;
	confirm_slices(t.count[2], ppu_shift, [&](u64 i, u64 at, u64 upto) {
		if (t.qstat[i] != 0 || t.flag[i] != 0 || at >= B) { return; }
		const uint8_t* a = in + t.uoff[t.cunit[i]] + t.cpos[i] + at;
		const uint8_t* b = reinterpret_cast<const uint8_t*>((uintptr_t)r.src[r.owner[r.unit_first[i]]]) + at;   // (an MSCOMP_OK request of B bytes at k B has exactly one unit)
		if (cpd_differs<CPD_THREADS>(a, b, (upto < B ? upto : B) - at, threadIdx.x)) { t.flag[i] = 1u; }
	});
}

// ---- confirm by digest (mscomp_amd_syncer_sync_digest; the digest kernels: digest.hip) ----
// Behind sy_req_kernel, one thread per slot of the kept list: the window of a kept candidate as a unit of the digest passes, and the
// status the reader core would have written -- MSCOMP_OK, since nothing is decoded; a row outside the numbering is refuted.
__global__ __launch_bounds__(256) void sy_dunits_kernel(uint32_t n, uint32_t ncand, uint32_t shift, SyncTab t, u64* __restrict__ off, u64* __restrict__ len)
{
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= ncand) { return; }
	u64 o = 0, l = 0;
	int32_t st = 0;
	if (i < t.count[2]) {
		o = t.uoff[t.cunit[i]] + t.cpos[i]; l = (u64)1 << shift;               // (cpos + B <= ulen: rule 3)
		if (t.crow[i] >= t.ufirst[n]) { st = -3; }                             // MSCOMP_DATA_ERROR
	}
	off[i] = o; len[i] = l; t.qstat[i] = st;
}

// Behind the root pass, one thread per kept candidate: its window's digest against the four words at its row of the store's table
__global__ __launch_bounds__(256) void sy_dcompare_kernel(SpliceView v, uint32_t n, uint32_t ncand, const uint32_t* __restrict__ block_digest, SyncTab t,
                                                         const uint32_t* __restrict__ wdig)
{
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= ncand || i >= t.count[2] || t.qstat[i] != 0) { return; }
	const u64 row = t.crow[i];
	const uint32_t x = res_of_block(t.ufirst, n, row);
	const uint32_t* a = wdig + 4u * (u64)i;
	const uint32_t* b = block_digest + 4u * (v.first[x] + (row - t.ufirst[x]));   // (first[x] + k < first[x + 1] <= v.nbt: rule 1)
	if (a[0] != b[0] || a[1] != b[1] || a[2] != b[2] || a[3] != b[3]) { t.flag[i] = 1u; }
}

// ---- select and emit ----
// the first slot of the kept list (sorted by unit, then position) that belongs to unit u or a later one
__device__ __forceinline__ u64 sy_lower(const uint32_t* __restrict__ cunit, u64 kept, uint32_t u)
{
	u64 lo = 0, hi = kept;
	while (lo < hi) { const u64 mid = lo + (hi - lo) / 2u; if (cunit[mid] < u) { lo = mid + 1u; } else { hi = mid; } }
	return lo;
}

// One wave's greedy walk over the kept candidates of unit u -- a confirmed one at or behind `end` is a hit, and end = p + B --, sixty-four
// candidates per step: the lanes load them, the wave decides the hits among the confirmed ones with scalar reads of the lanes (the walk
// is serial by nature; a step is a few scalar instructions and touches no memory), and the lanes that hold a hit finish it side by side:
// its rank from the hit mask, the gap in front of it from the hit below it. WRITE: the hits as the reader's requests and offsets from
// slot h on, the gaps as literal runs from slot q on. Counts: hits, runs, confirmed.
template <bool WRITE>
__device__ __forceinline__ void sy_walk(const SyncTab& t, uint32_t u, u64 B, u64 kept, const int32_t* __restrict__ status, uint32_t lane, u64 h, u64 q,
                                        u64* __restrict__ req, u64* __restrict__ req_off, u64* __restrict__ lit, u64 (&cnt)[3])
{
	const u64 lo = sy_lower(t.cunit, kept, u), hi = sy_lower(t.cunit, kept, u + 1u), L = status[u] == 0 ? t.ulen[u] : 0, off = t.uoff[u];
	u64 end = 0;
	for (u64 base = lo; base < hi; base += 64u) {
		const u64 i = base + lane, end0 = end;
		const bool live = i < hi;
		const u64 p = live ? t.cpos[i] : 0;
		const u64 mask = __ballot(live && t.qstat[i] == 0 && t.flag[i] == 0);
		u64 hm = 0;
		#pragma unroll
		for (int j = 0; j < 64; ++j) {
			if (!((mask >> j) & 1u)) { continue; }
			const u64 pj = (u64)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)p, j) | (u64)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(p >> 32), j) << 32;
			if (pj >= end) { hm |= (u64)1 << j; end = pj + B; }
		}
		const u64 below = hm & (((u64)1 << lane) - 1u);
		const u64 pp = __shfl(p, below ? 63 - __clzll((long long)below) : 0, 64);
		const u64 pe = below ? pp + B : end0;                                // where the hit below this lane's ends
		const bool hit = (hm >> lane) & 1u, gap = hit && p > pe;
		const u64 gm = __ballot(gap);
		if (WRITE && hit) {
			const u64 x = h + (u64)__popcll(below);
			req[3u * x] = t.req[3u * i]; req[3u * x + 1u] = t.req[3u * i + 1u]; req[3u * x + 2u] = t.req[3u * i + 2u]; req_off[x] = off + p;
			if (gap) { const u64 y = q + (u64)__popcll(gm & (((u64)1 << lane) - 1u)); lit[2u * y] = off + pe; lit[2u * y + 1u] = p - pe; }
		}
		h += (u64)__popcll(hm); q += (u64)__popcll(gm);
		cnt[0] += (u64)__popcll(hm); cnt[1] += (u64)__popcll(gm); cnt[2] += (u64)__popcll(mask);
	}
	if (L > end) {
		if (WRITE && lane == 0) { lit[2u * q] = off + end; lit[2u * q + 1u] = L - end; }
		++cnt[1];
	}
}

// Select and emit, one block, a wave per unit in turn: the walk once to count, the scan of the counts over the units, the walk again to
// write. Then the counts.
__global__ __launch_bounds__(DV_THREADS) void sy_select_kernel(uint32_t n, uint32_t shift, SyncTab t, const int32_t* __restrict__ status, const uint32_t* __restrict__ distinct,
                                                              u64* hit_first, u64* __restrict__ req, u64* __restrict__ req_off, u64* lit_first,
                                                              u64* __restrict__ lit, u64* __restrict__ count)
{
	__shared__ u64 s_w[2][DV_WAVES];
	__shared__ u64 s_tot[2][DV_WAVES];
	const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
	const u64 B = (u64)1 << shift, kept = t.count[2];
	u64 bytes = 0, conf = 0;
	for (uint32_t u = wave; u < n; u += DV_WAVES) {
		u64 c[3] = {0, 0, 0};
		sy_walk<false>(t, u, B, kept, status, lane, 0, 0, req, req_off, lit, c);
		if (lane == 0) { hit_first[u + 1u] = c[0]; lit_first[u + 1u] = c[1]; }
		bytes += (status[u] == 0 ? t.ulen[u] : 0) - (c[0] << shift); conf += c[2];      // what no hit covers
	}
	if (lane == 0) { s_tot[0][wave] = bytes; s_tot[1][wave] = conf; }
	if (tid == 0) { hit_first[0] = 0; lit_first[0] = 0; }
	__syncthreads();
	u64 carry[2] = {0, 0};
	for (uint32_t base = 0; base < n; base += DV_THREADS) {
		const uint32_t u = base + tid;
		u64 a[2] = {u < n ? hit_first[u + 1u] : 0, u < n ? lit_first[u + 1u] : 0};
		dv_block_scan<2>(a, carry, s_w);
		if (u < n) { hit_first[u + 1u] = a[0]; lit_first[u + 1u] = a[1]; }
	}
	__syncthreads();
	for (uint32_t u = wave; u < n; u += DV_WAVES) {
		u64 c[3] = {0, 0, 0};
		sy_walk<true>(t, u, B, kept, status, lane, hit_first[u], lit_first[u], req, req_off, lit, c);
	}
	if (tid == 0) {
		u64 lb = 0, nc = 0;
		for (uint32_t w = 0; w < DV_WAVES; ++w) { lb += s_tot[0][w]; nc += s_tot[1][w]; }
		const u64 c[8] = { t.count[0], t.count[1], kept, nc, carry[0], carry[1], lb, distinct ? (u64)distinct[0] : 0u };
		for (uint32_t i = 0; i < 8u; ++i) { count[i] = c[i]; t.count[i] = c[i]; }
	}
}

// ---- host ----
void sync_host_consts(uint32_t shift, uint32_t* out)
{
	uint32_t xb = CRC_ONE >> 1;                                            // x^1, squared up to x^(8B) = x^(2^(shift + 3))
	for (uint32_t k = 0; k < shift + 3u; ++k) { xb = crc_mul(xb, xb); }
	for (uint32_t b = 0; b < 256u; ++b) {
		uint32_t v = b;
		for (int i = 0; i < 8; ++i) { v = (v >> 1) ^ (CRC_POLY & (0u - (v & 1u))); }
		out[b] = crc_mul(v, xb);
		for (uint32_t k = 0; k < 4u; ++k) { out[256u + 256u * k + b] = crc_mul(b << (8u * k), xb); }
	}
	out[5u * 256u] = crc_mul(0xFFFFFFFFu, xb) ^ 0xFFFFFFFFu;               // crc_seed(B)
	out[5u * 256u + 1u] = out[5u * 256u + 2u] = out[5u * 256u + 3u] = 0;
}

void launch_sync_clear(hipStream_t st, const SyncTab& t, uint32_t blocks)
{
	hipLaunchKernelGGL(sy_clear_kernel, fixed_grid(t.kt.slots > SYNC_BIT_WORDS ? t.kt.slots : SYNC_BIT_WORDS, 256u, blocks), dim3(256), 0, st, t);
}

void launch_sync_seed(hipStream_t st, const SpliceView& v, uint32_t n, uint32_t shift, const SyncTab& t, int32_t* status)
{
	hipLaunchKernelGGL(sy_seed_kernel, dim3(1), dim3(DV_THREADS), 0, st, v, n, shift, t.ufirst, status);
}

void launch_sync_keys(hipStream_t st, const SpliceView& v, uint32_t n, uint32_t nbt, uint32_t shift, const SyncTab& t, const int32_t* status, uint32_t blocks)
{
	if (nbt == 0) { return; }
	hipLaunchKernelGGL(sy_keys_kernel, fixed_grid(nbt, 256u, blocks), dim3(256), 0, st, v, n, shift, t, status);
}

void launch_sync_units(hipStream_t st, uint32_t n_units, uint32_t shift, u64 in_total_max, const u64* in_off, const u64* in_len, const SyncTab& t, int32_t* status)
{
	hipLaunchKernelGGL(sy_units_kernel, dim3(1), dim3(DV_THREADS), 0, st, n_units, shift, in_total_max, in_off, in_len, t, status);
}

void launch_sync_bounds(hipStream_t st, uint32_t n_units, const uint8_t* in, const SyncTab& t, uint32_t blocks)
{
	if (t.tiles_max == 0) { return; }
	hipLaunchKernelGGL(sy_piece_kernel, fixed_grid(t.tiles_max, 4u, blocks), dim3(SY_THREADS), 0, st, n_units, in, t);
	hipLaunchKernelGGL(sy_pre_kernel, dim3(1), dim3(DV_THREADS), 0, st, n_units, t);
	hipLaunchKernelGGL(sy_abs_kernel, fixed_grid(t.tiles_max, 4u, blocks), dim3(SY_THREADS), 0, st, n_units, t);
}

void launch_sync_scan(hipStream_t st, uint32_t n_units, uint32_t n_cand, uint32_t shift, const uint8_t* in, const SyncTab& t, uint32_t blocks)
{
	if (t.tiles_max) { hipLaunchKernelGGL(sy_scan_kernel<false>, fixed_grid(t.tiles_max, 4u, blocks), dim3(SY_THREADS), 0, st, n_units, n_cand, shift, in, t); }
	hipLaunchKernelGGL(sy_tilescan_kernel, dim3(1), dim3(DV_THREADS), 0, st, n_units, n_cand, shift, t);
	if (t.tiles_max && n_cand) { hipLaunchKernelGGL(sy_scan_kernel<true>, fixed_grid(t.tiles_max, 4u, blocks), dim3(SY_THREADS), 0, st, n_units, n_cand, shift, in, t); }
}

void launch_sync_requests(hipStream_t st, uint32_t n, uint32_t n_cand, uint32_t shift, const SyncTab& t)
{
	if (n_cand == 0) { return; }
	hipLaunchKernelGGL(sy_req_kernel, dim3((n_cand + 255u) / 256u), dim3(256), 0, st, n, n_cand, shift, t);
}

void launch_sync_confirm(hipStream_t st, uint32_t n_cand, uint32_t shift, const uint8_t* in, const SyncTab& t, const ReaderTab& r, uint32_t blocks)
{
	if (n_cand == 0) { return; }
	const uint32_t ppu_shift = shift > DD_PIECE_SHIFT ? shift - DD_PIECE_SHIFT : 0u;
	hipLaunchKernelGGL(sy_confirm_kernel, fixed_grid((u64)n_cand << ppu_shift, DD_SLICE_MIN, blocks), dim3(CPD_THREADS), 0, st, shift, ppu_shift, in, t, r);
}

void launch_sync_digest_units(hipStream_t st, uint32_t n, uint32_t n_cand, uint32_t shift, const SyncTab& t, u64* off, u64* len)
{
	if (n_cand == 0) { return; }
	hipLaunchKernelGGL(sy_dunits_kernel, dim3((n_cand + 255u) / 256u), dim3(256), 0, st, n, n_cand, shift, t, off, len);
}

void launch_sync_digest_compare(hipStream_t st, const SpliceView& v, uint32_t n, uint32_t n_cand, const uint32_t* block_digest, const SyncTab& t, const uint32_t* wdig)
{
	if (n_cand == 0) { return; }
	hipLaunchKernelGGL(sy_dcompare_kernel, dim3((n_cand + 255u) / 256u), dim3(256), 0, st, v, n, n_cand, block_digest, t, wdig);
}

void launch_sync_select(hipStream_t st, uint32_t n_units, uint32_t shift, const SyncTab& t, const int32_t* status, const uint32_t* distinct, u64* hit_first, u64* req, u64* req_off,
                        u64* lit_first, u64* lit, u64* count)
{
	hipLaunchKernelGGL(sy_select_kernel, dim3(1), dim3(DV_THREADS), 0, st, n_units, shift, t, status, distinct, hit_first, req, req_off, lit_first, lit, count);
}

} // namespace msc
