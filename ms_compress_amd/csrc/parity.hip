// parity.hip -- Reed-Solomon parity rows of a block container (mscomp_amd_parity_*, include/mscomp_amd.h): m <= 3 parity rows for every k
// stored rows, and from them up to m lost rows per group back, without a mirror. The code is the Vandermonde one of RAID-6 over GF(2^8)
// (gfmath.h): P_p[x] = XOR_i alpha^(p i) D_i[x], D_i[x] = stored byte x of member i and 0 at and behind its stored length. By Horner from
// the last member down, acc_p = alpha^p acc_p ^ d: the build pass is loads, p shifts-and-masks per dword and stores -- no table, no LDS, no
// atomic. Groups are interleaved: row j of nb is member j / G of group j % G, G = ceil(nb / k), so a burst of G rows costs every group one
// member. Kernels only, vector stores only; the CRC-32 of the parity rows is the CRC unit kernels' (crc32.hip). DESIGN.md 4.22.
#include "../../include/mscomp_amd.h"
#include "rowpass.h"
#include "gfmath.h"

namespace msc {

#define PA_THREADS 256u                                  // lanes of a parity or solve workgroup: 16 bytes of the column each
#define PA_DEPTH   4u                                    // members whose loads are in flight at once
#define PA_SCAN_PER 8u                                   // entries a lane of the running sum takes: a tile is 8192 of them
static_assert(PA_THREADS * 16u == 1u << PA_TILE_SHIFT, "a column tile is a workgroup's lanes");

// Rule 0 of both calls, which every pass works out for itself from the view and the header (two scalar loads, five in rebuild): the rows nb
// the container has, its groups G, and the status that refuses the call -- then with nb = G = 0, so that a pass finds nothing to do.
struct PaHead { u64 nb, G; int32_t st; };
__device__ __forceinline__ PaHead pa_head(const SpliceView& v, const ParityTab& t, uint32_t mis, const u64* __restrict__ head)
{
	PaHead h = {0, 0, MSCOMP_ARG_ERROR};
	if (mis) { return h; }
	const u64 nb = v.n_res ? v.first[v.n_res] : 0;
	if (nb > t.nbt) { return h; }
	const u64 G = (nb + t.k - 1u) / t.k;
	h.st = MSCOMP_DATA_ERROR;
	if (head && (head[0] != nb || head[1] != G || head[2] != t.k || head[3] != t.m)) { return h; }   // parity of another container, or of another shape
	h.nb = nb; h.G = G; h.st = MSCOMP_OK;
	return h;
}
// the members group g (< G) has: the i with i G + g < nb
__device__ __forceinline__ uint32_t pa_members(const PaHead& h, u64 g) { return (uint32_t)((h.nb - g + h.G - 1u) / h.G); }

// The 16 bytes at column col of a stored row of len bytes, zeros at and behind len, in two steps -- so that the loads of a batch of members
// are all issued before the first of them is waited for: a load inside a lane's own branch is waited for where the branch ends, and a
// group's members then cost a round trip to memory each. pa_fetch: for a row of 16 bytes or more ONE 16-byte load at any alignment in
// every lane, from inside the row -- a lane on or behind the row's end loads the row's last 16 bytes --; a shorter row (len is the same
// in every lane: a scalar branch) is read byte by byte by its first lane. Never a byte in front of row or behind row + len.
__device__ __forceinline__ uint32_t pa_at(uint32_t len, uint32_t col) { return len < 16u || col + 16u <= len ? col : len - 16u; }
__device__ __forceinline__ uint4 pa_fetch(const uint8_t* __restrict__ row, uint32_t len, uint32_t col)
{
	uint32_t w[4] = {0, 0, 0, 0};
	if (len >= 16u) {
		const cpd_u16 x = *reinterpret_cast<const cpd_u16*>(row + pa_at(len, col));
		w[0] = x.w[0]; w[1] = x.w[1]; w[2] = x.w[2]; w[3] = x.w[3];
	} else if (col < len) {
		#pragma unroll
		for (uint32_t b = 0; b < 16u; ++b) { if (col + b < len) { w[b >> 2] |= (uint32_t)row[col + b] << (8u * (b & 3u)); } }
	}
	return make_uint4(w[0], w[1], w[2], w[3]);
}
// pa_bytes: what pa_fetch loaded moved down to the lane's column -- by col - pa_at bytes: none for a whole 16, all for a lane behind the row
__device__ __forceinline__ uint4 pa_bytes(uint4 x, uint32_t len, uint32_t col)
{
	const uint32_t sh = col - pa_at(len, col), s8 = (sh & 7u) * 8u;
	const u64 lo = x.x | (u64)x.y << 32, hi = x.z | (u64)x.w << 32;
	const u64 l1 = sh & 8u ? hi : lo, h1 = sh & 8u ? 0 : hi;                 // by eight bytes, then by the rest
	const u64 l2 = (l1 >> s8) | ((h1 << 1) << (63u - s8)), h2 = h1 >> s8;
	const bool none = sh >= 16u;
	return make_uint4(none ? 0u : (uint32_t)l2, none ? 0u : (uint32_t)(l2 >> 32), none ? 0u : (uint32_t)h2, none ? 0u : (uint32_t)(h2 >> 32));
}
__device__ __forceinline__ uint4 pa_x2(uint4 a) { return make_uint4(gf_x2(a.x), gf_x2(a.y), gf_x2(a.z), gf_x2(a.w)); }
__device__ __forceinline__ uint4 pa_xor(uint4 a, uint4 b) { return make_uint4(a.x ^ b.x, a.y ^ b.y, a.z ^ b.z, a.w ^ b.w); }
// alpha^p a, p <= 2 and the same in every lane
__device__ __forceinline__ uint4 pa_xp(uint4 a, uint32_t p)
{
	if (p >= 1u) { a = pa_x2(a); }
	if (p >= 2u) { a = pa_x2(a); }
	return a;
}

// ---- build ----
// Rule 1, a fixed grid over the table's rows: a row's stored length where its two table entries are in order, within packed_len and at
// most B apart; 0 otherwise and at and behind nb.
__global__ __launch_bounds__(256) void pa_rows_kernel(SpliceView v, ParityTab t, uint32_t mis, uint32_t* __restrict__ row_len)
{
	const PaHead h = pa_head(v, t, mis, nullptr);
	if (h.st != MSCOMP_OK) { return; }                                       // (rule 0: nothing but the header, the offsets and the status is written)
	for (u64 j = (u64)blockIdx.x * 256u + threadIdx.x; j < t.nbt; j += (u64)gridDim.x * 256u) {
		uint32_t len = 0;
		if (j < h.nb) {
			const u64 a = v.off[j], b = v.off[j + 1u];
			if (a <= b && b <= v.packed_len && b - a <= (u64)1 << t.shift) { len = (uint32_t)(b - a); }
		}
		row_len[j] = len;
	}
}

// The groups' maxima, a lane per possible group: t.plen[g m + p] = the largest row_len of group g rounded up to 16, 0 at and behind G.
// Adjacent lanes read adjacent rows. head: rebuild's (null in build).
__global__ __launch_bounds__(256) void pa_groups_kernel(SpliceView v, ParityTab t, uint32_t mis, const uint32_t* __restrict__ row_len, const u64* __restrict__ head)
{
	const PaHead h = pa_head(v, t, mis, head);
	for (u64 g = (u64)blockIdx.x * 256u + threadIdx.x; g < t.gmax; g += (u64)gridDim.x * 256u) {
		uint32_t mx = 0;
		if (g < h.G) {
			const uint32_t n = pa_members(h, g);
			for (uint32_t i = 0; i < n; ++i) { const uint32_t len = row_len[(u64)i * h.G + g]; mx = len > mx ? len : mx; }
		}
		const u64 plen = ((u64)mx + 15u) & ~(u64)15u;
		for (uint32_t p = 0; p < t.m; ++p) { t.plen[g * t.m + p] = plen; }
	}
}

// The running sum of n lengths (one workgroup, in tiles): out[0] = 0, out[i + 1] = len[0] + .. + len[i] -- the parity rows' offsets in
// build, the fix view's offset table in rebuild. A lane takes PA_SCAN_PER consecutive entries, loaded before anything waits for them, so
// the workgroup's serial steps -- a block scan each, which is latency and nothing else -- are an eighth of a scan with a lane per entry.
// (No sum here comes near 2^64: at most 2^31 lengths below 2^32.)
__global__ __launch_bounds__(DV_THREADS) void pa_scan_kernel(u64 n, const u64* __restrict__ len, u64* __restrict__ out)
{
	__shared__ u64 s_w[1][DV_WAVES];
	u64 run[1] = {0};
	if (threadIdx.x == 0) { out[0] = 0; }
	for (u64 base = 0; base < n; base += (u64)DV_THREADS * PA_SCAN_PER) {
		const u64 at = base + (u64)threadIdx.x * PA_SCAN_PER;
		const bool all = at + PA_SCAN_PER <= n;                                 // (a lane whose entries all exist: no test per entry, no eight masks kept across the scan)
		u64 v[PA_SCAN_PER];
		if (all) {
			#pragma unroll
			for (uint32_t j = 0; j < PA_SCAN_PER; ++j) { v[j] = len[at + j]; }
		} else {
			#pragma unroll
			for (uint32_t j = 0; j < PA_SCAN_PER; ++j) { v[j] = at + j < n ? len[at + j] : 0; }
		}
		#pragma unroll
		for (uint32_t j = 1; j < PA_SCAN_PER; ++j) { v[j] += v[j - 1u]; }
		u64 tot[1] = {v[PA_SCAN_PER - 1u]};
		dv_block_scan<1>(tot, run, s_w);                                     // up to and including this lane's entries
		const u64 before = tot[0] - v[PA_SCAN_PER - 1u];
		if (all) {
			#pragma unroll
			for (uint32_t j = 0; j < PA_SCAN_PER; ++j) { out[at + j + 1u] = before + v[j]; }
		} else {
			#pragma unroll
			for (uint32_t j = 0; j < PA_SCAN_PER; ++j) { if (at + j < n) { out[at + j + 1u] = before + v[j]; } }
		}
	}
}

// Rule 4 for the CRC pass: a parity row that ends beyond par_cap is not written, and read as an empty unit
__global__ __launch_bounds__(256) void pa_units_kernel(ParityTab t, const u64* __restrict__ par_off, u64 par_cap)
{
	const u64 Q = (u64)t.gmax * t.m;
	for (u64 q = (u64)blockIdx.x * 256u + threadIdx.x; q < Q; q += (u64)gridDim.x * 256u) { t.clen[q] = par_off[q + 1u] <= par_cap ? t.plen[q] : 0; }
}

// The parity pass, a fixed grid dealt over (group, column tile) items: a lane owns 16 bytes of the group's column, walks the members from
// the last one down with PA_DEPTH independent loads in flight, and writes M aligned 16-byte stores. The members' table entries are the same
// in every lane: scalar loads.
template <uint32_t M>
__global__ __launch_bounds__(PA_THREADS) void pa_build_kernel(SpliceView v, ParityTab t, uint32_t mis, const uint32_t* __restrict__ row_len, uint8_t* __restrict__ par,
                                                             u64 par_cap, const u64* __restrict__ par_off)
{
	const PaHead h = pa_head(v, t, mis, nullptr);
	const uint32_t ts = t.shift - PA_TILE_SHIFT;
	const u64 items = h.G << ts;
	for (u64 it = blockIdx.x; it < items; it += gridDim.x) {
		const u64 g = it >> ts, q0 = g * M;
		const uint32_t base = (uint32_t)(it & (((u64)1 << ts) - 1u)) << PA_TILE_SHIFT, col = base + threadIdx.x * 16u;
		const u64 o0 = par_off[q0], plen = par_off[q0 + 1u] - o0;
		if (base >= plen) { continue; }                                        // (the same in every lane)
		uint4 acc[M];
		#pragma unroll
		for (uint32_t p = 0; p < M; ++p) { acc[p] = make_uint4(0, 0, 0, 0); }
		// (the members in batches from the top: the places of a first batch above the last member are rows of no bytes, which leave 0 as it is)
		const uint32_t cnt = pa_members(h, g);
		for (uint32_t top = (cnt + PA_DEPTH - 1u) / PA_DEPTH * PA_DEPTH; top > 0; top -= PA_DEPTH) {
			uint4 d[PA_DEPTH];
			uint32_t len[PA_DEPTH];
			const uint8_t* row[PA_DEPTH];
			#pragma unroll
			for (uint32_t s = 0; s < PA_DEPTH; ++s) {                             // the batch's table entries first: scalar loads, none waiting for another
				const uint32_t x = top - 1u - s;
				const u64 j = x < cnt ? (u64)x * h.G + g : g;
				len[s] = x < cnt ? row_len[j] : 0;
				row[s] = v.packed + v.off[j];
			}
			#pragma unroll
			for (uint32_t s = 0; s < PA_DEPTH; ++s) { d[s] = pa_fetch(row[s], len[s], col); }
			#pragma unroll
			for (uint32_t s = 0; s < PA_DEPTH; ++s) {
				const uint4 b = pa_bytes(d[s], len[s], col);
				#pragma unroll
				for (uint32_t p = 0; p < M; ++p) { acc[p] = pa_xor(pa_xp(acc[p], p), b); }
			}
		}
		if (col >= plen) { continue; }
		#pragma unroll
		for (uint32_t p = 0; p < M; ++p) {
			if (o0 + (p + 1u) * plen <= par_cap) { *reinterpret_cast<uint4*>(par + o0 + p * plen + col) = acc[p]; }   // (par and every offset: multiples of 16)
		}
	}
}

// Behind the CRC pass: rules 5 and 6. par_crc from the scratch column (so that a refused call leaves the caller's alone), the header, the status.
__global__ __launch_bounds__(256) void pa_head_kernel(SpliceView v, ParityTab t, uint32_t mis, const u64* __restrict__ par_off, u64 par_cap, uint32_t* __restrict__ par_crc,
                                                     u64* __restrict__ par_head, int32_t* __restrict__ status)
{
	const PaHead h = pa_head(v, t, mis, nullptr);
	const u64 Q = (u64)t.gmax * t.m;
	if (blockIdx.x == 0 && threadIdx.x == 0) {
		const bool ok = h.st == MSCOMP_OK;
		par_head[0] = h.nb; par_head[1] = h.G; par_head[2] = ok ? t.k : 0; par_head[3] = ok ? t.m : 0;
		status[0] = !ok ? h.st : Q && par_off[Q] > par_cap ? MSCOMP_BUF_ERROR : MSCOMP_OK;   // (the rows lie in order: one ends beyond the capacity when the last does)
	}
	if (h.st != MSCOMP_OK) { return; }
	for (u64 q = (u64)blockIdx.x * 256u + threadIdx.x; q < Q; q += (u64)gridDim.x * 256u) { par_crc[q] = t.pcrc[q]; }
}

// ---- rebuild ----
// the table half of rule 2: parity row q lies in order, within par_len and has the length the row lengths give it
__device__ __forceinline__ bool pa_par_ok(const ParityTab& t, const u64* __restrict__ par_off, u64 par_len, u64 q)
{
	const u64 a = par_off[q], b = par_off[q + 1u];
	return a <= b && b <= par_len && b - a == t.plen[q] && !(a & 15u);              // (and where build puts one: the solve pass loads it 16 bytes at a time)
}

// In front of the CRC pass, a fixed grid over the parity rows and the table's rows: what the CRC kernels read of a parity row -- all of it, or
// nothing of one the table refuses --, and the columns and counts of this execution cleared.
__global__ __launch_bounds__(256) void pa_check_kernel(ParityTab t, const u64* __restrict__ par_off, u64 par_len)
{
	const u64 Q = (u64)t.gmax * t.m, n = Q > t.nbt ? Q : t.nbt;
	if (blockIdx.x == 0 && threadIdx.x < 8u) { t.count[threadIdx.x] = 0; }
	for (u64 i = (u64)blockIdx.x * 256u + threadIdx.x; i < n; i += (u64)gridDim.x * 256u) {
		if (i < Q) { t.clen[i] = pa_par_ok(t, par_off, par_len, i) ? t.plen[i] : 0; }
		if (i < t.nbt) { t.fixlen[i] = 0; t.rflag[i] = 0; }
	}
}

// Rules 1-3, a lane per group: the missing members, the usable parity rows, and for a group that can be recovered its record -- the e
// parities used, the e members missing, the inverse of alpha^(p_a i_b) -- in the next free slot of the list; the rows it rebuilds get their
// lengths in t.fixlen. The counts are sums: the order the lanes arrive in shows nowhere in the answer.
__global__ __launch_bounds__(256) void pa_damage_kernel(SpliceView v, ParityTab t, uint32_t mis, const uint32_t* __restrict__ verdict, const u64* __restrict__ par_off, u64 par_len,
                                                       const uint32_t* __restrict__ par_crc, const uint32_t* __restrict__ row_len, const u64* __restrict__ head)
{
	const PaHead h = pa_head(v, t, mis, head);
	unsigned long long* cnt = reinterpret_cast<unsigned long long*>(t.count);
	for (u64 g = (u64)blockIdx.x * 256u + threadIdx.x; g < h.G; g += (u64)gridDim.x * 256u) {
		const uint32_t n = pa_members(h, g);
		uint32_t e = 0, mi = 0;                                                // the first three missing members, a byte each
		for (uint32_t i = 0; i < n; ++i) {
			const u64 j = (u64)i * h.G + g, a = v.off[j], b = v.off[j + 1u];
			const bool present = verdict[j] == SV_GOOD && a <= b && b <= v.packed_len && b - a == row_len[j];
			if (!present) { if (e < GF_ROWS) { mi |= i << (8u * e); } ++e; }
		}
		uint32_t u = 0, pu = 0;                                                // the first three usable parities, four bits each
		for (uint32_t p = 0; p < t.m; ++p) {
			const u64 q = g * t.m + p;
			if (pa_par_ok(t, par_off, par_len, q) && t.pcrc[q] == par_crc[q]) { pu |= p << (4u * u); ++u; }
		}
		if (u < t.m) { atomicAdd(cnt + 4, (unsigned long long)(t.m - u)); }
		if (e == 0) { continue; }
		atomicAdd(cnt + 0, (unsigned long long)e); atomicAdd(cnt + 2, 1ull);
		if (e > u) { atomicAdd(cnt + 3, 1ull); continue; }
		uint32_t a[GF_ROWS][GF_ROWS], inv[GF_ROWS][GF_ROWS];
		#pragma unroll
		for (uint32_t r = 0; r < GF_ROWS; ++r) {
			#pragma unroll
			for (uint32_t c = 0; c < GF_ROWS; ++c) { a[r][c] = gf_exp(((pu >> (4u * r)) & 15u) * ((mi >> (8u * c)) & 255u)); }
		}
		(void)gf_invert(e, a, inv);                                            // (never singular for m <= 3: DESIGN.md 4.22)
		u64 bytes = 0;
		#pragma unroll
		for (uint32_t b = 0; b < GF_ROWS; ++b) {
			if (b < e) { const u64 j = (u64)((mi >> (8u * b)) & 255u) * h.G + g; const uint32_t len = row_len[j]; t.fixlen[j] = len; t.rflag[j] = 1u; bytes += len; }
		}
		atomicAdd(cnt + 1, (unsigned long long)e); atomicAdd(cnt + 5, (unsigned long long)bytes);
		uint32_t* rec = t.grec + 6u * (u64)atomicAdd(cnt + 6, 1ull);           // (a group is listed once: no more entries than gmax)
		rec[0] = e | pu << 8; rec[1] = mi; rec[5] = (uint32_t)g;
		#pragma unroll
		for (uint32_t r = 0; r < GF_ROWS; ++r) { rec[2u + r] = inv[r][0] | inv[r][1] << 8 | inv[r][2] << 16; }
	}
}

// sixteen bytes of a rebuilt row, the first n of them: one store at any alignment, or byte stores on the row's end
__device__ __forceinline__ void pa_store(uint8_t* __restrict__ dst, uint4 d, uint32_t n)
{
	if (n >= 16u) { cpd_u16 x; x.w[0] = d.x; x.w[1] = d.y; x.w[2] = d.z; x.w[3] = d.w; *reinterpret_cast<cpd_u16*>(dst) = x; return; }
	const uint32_t w[4] = {d.x, d.y, d.z, d.w};
	#pragma unroll
	for (uint32_t b = 0; b < 16u; ++b) { if (b < n) { dst[b] = (uint8_t)(w[b >> 2] >> (8u * (b & 3u))); } }
}
__device__ __forceinline__ uint4 pa_mulc(uint4 a, uint32_t c) { return make_uint4(gf_mulc(a.x, c), gf_mulc(a.y, c), gf_mulc(a.z, c), gf_mulc(a.w, c)); }

// The solve pass, a fixed grid dealt over (listed group, column tile) items: the syndromes -- the Horner pass over the present members, a
// missing one counting as zeros, XOR the parity rows used -- times the inverse are the missing members' bytes. A row that would end beyond
// fix_cap is not written (rule 5).
__global__ __launch_bounds__(PA_THREADS) void pa_solve_kernel(SpliceView v, ParityTab t, uint32_t mis, const uint8_t* __restrict__ par, const u64* __restrict__ par_off,
                                                             const uint32_t* __restrict__ row_len, const u64* __restrict__ head, uint8_t* __restrict__ fix, u64 fix_cap,
                                                             const u64* __restrict__ fix_off)
{
	const PaHead h = pa_head(v, t, mis, head);
	if (h.st != MSCOMP_OK) { return; }
	const uint32_t ts = t.shift - PA_TILE_SHIFT;
	const u64 items = t.count[6] << ts;
	for (u64 it = blockIdx.x; it < items; it += gridDim.x) {
		const uint32_t* __restrict__ rec = t.grec + 6u * (it >> ts);
		const uint32_t e = rec[0] & 7u, pu = rec[0] >> 8, mi = rec[1];
		const u64 g = rec[5], q0 = g * t.m;
		const uint32_t base = (uint32_t)(it & (((u64)1 << ts) - 1u)) << PA_TILE_SHIFT, col = base + threadIdx.x * 16u;
		const u64 plen = t.plen[q0];
		if (base >= plen) { continue; }
		const uint32_t m0 = mi & 255u, m1 = e > 1u ? (mi >> 8) & 255u : ~0u, m2 = e > 2u ? (mi >> 16) & 255u : ~0u;
		uint4 acc[GF_ROWS];
		#pragma unroll
		for (uint32_t a = 0; a < GF_ROWS; ++a) { acc[a] = make_uint4(0, 0, 0, 0); }
		const uint32_t cnt = pa_members(h, g);
		for (uint32_t top = (cnt + PA_DEPTH - 1u) / PA_DEPTH * PA_DEPTH; top > 0; top -= PA_DEPTH) {
			uint4 d[PA_DEPTH];
			uint32_t len[PA_DEPTH];
			const uint8_t* row[PA_DEPTH];
			#pragma unroll
			for (uint32_t s = 0; s < PA_DEPTH; ++s) {
				const uint32_t x = top - 1u - s;
				const bool present = x < cnt && x != m0 && x != m1 && x != m2;
				const u64 j = present ? (u64)x * h.G + g : g;
				len[s] = present ? row_len[j] : 0;                                 // (a missing member: a row of no bytes, and not read)
				row[s] = v.packed + v.off[j];
			}
			#pragma unroll
			for (uint32_t s = 0; s < PA_DEPTH; ++s) { d[s] = pa_fetch(row[s], len[s], col); }
			#pragma unroll
			for (uint32_t s = 0; s < PA_DEPTH; ++s) {
				const uint4 b = pa_bytes(d[s], len[s], col);
				#pragma unroll
				for (uint32_t a = 0; a < GF_ROWS; ++a) { if (a < e) { acc[a] = pa_xor(pa_xp(acc[a], (pu >> (4u * a)) & 15u), b); } }
			}
		}
		if (col >= plen) { continue; }
		#pragma unroll
		for (uint32_t a = 0; a < GF_ROWS; ++a) {
			if (a < e) { acc[a] = pa_xor(acc[a], *reinterpret_cast<const uint4*>(par + par_off[q0 + ((pu >> (4u * a)) & 15u)] + col)); }   // (a usable row: 16-byte aligned, within par_len)
		}
		#pragma unroll
		for (uint32_t b = 0; b < GF_ROWS; ++b) {
			if (b >= e) { continue; }
			const u64 j = (u64)((mi >> (8u * b)) & 255u) * h.G + g;
			const uint32_t len = row_len[j];
			if (col >= len || fix_off[j + 1u] > fix_cap) { continue; }
			uint4 d = make_uint4(0, 0, 0, 0);
			#pragma unroll
			for (uint32_t a = 0; a < GF_ROWS; ++a) { if (a < e) { d = pa_xor(d, pa_mulc(acc[a], (rec[2u + b] >> (8u * a)) & 255u)); } }
			pa_store(fix + fix_off[j] + col, d, len - col);
		}
	}
}

// Rules 6-8, a fixed grid over the table's rows: the verdicts, and from one lane the counts and the status.
__global__ __launch_bounds__(256) void pa_tail_kernel(SpliceView v, ParityTab t, uint32_t mis, const u64* __restrict__ head, u64 fix_cap, const u64* __restrict__ fix_off,
                                                     uint32_t* __restrict__ fix_verdict, u64* __restrict__ count, int32_t* __restrict__ status)
{
	const PaHead h = pa_head(v, t, mis, head);
	if (blockIdx.x == 0 && threadIdx.x == 0) {
		#pragma unroll
		for (uint32_t i = 0; i < 6u; ++i) { count[i] = t.count[i]; }
		status[0] = h.st != MSCOMP_OK ? h.st : t.nbt && fix_off[t.nbt] > fix_cap ? MSCOMP_BUF_ERROR : t.count[3] ? MSCOMP_DATA_ERROR : MSCOMP_OK;
	}
	for (u64 j = (u64)blockIdx.x * 256u + threadIdx.x; j < t.nbt; j += (u64)gridDim.x * 256u) {
		fix_verdict[j] = t.rflag[j] && fix_off[j + 1u] <= fix_cap ? SV_GOOD : SV_SKIPPED;
	}
}

void launch_parity_rows(hipStream_t st, const SpliceView& v, const ParityTab& t, bool mis, uint32_t* row_len, uint32_t blocks)
{
	hipLaunchKernelGGL(pa_rows_kernel, fixed_grid(t.nbt, 256u, blocks), dim3(256), 0, st, v, t, mis ? 1u : 0u, row_len);
}
void launch_parity_groups(hipStream_t st, const SpliceView& v, const ParityTab& t, bool mis, const uint32_t* row_len, const u64* head, uint32_t blocks)
{
	hipLaunchKernelGGL(pa_groups_kernel, fixed_grid(t.gmax, 256u, blocks), dim3(256), 0, st, v, t, mis ? 1u : 0u, row_len, head);
}
void launch_parity_scan(hipStream_t st, u64 n, const u64* len, u64* out)
{
	hipLaunchKernelGGL(pa_scan_kernel, dim3(1), dim3(DV_THREADS), 0, st, n, len, out);
}
void launch_parity_units(hipStream_t st, const ParityTab& t, const u64* par_off, u64 par_cap, uint32_t blocks)
{
	hipLaunchKernelGGL(pa_units_kernel, fixed_grid((u64)t.gmax * t.m, 256u, blocks), dim3(256), 0, st, t, par_off, par_cap);
}
void launch_parity_build(hipStream_t st, const SpliceView& v, const ParityTab& t, bool mis, const uint32_t* row_len, uint8_t* par, u64 par_cap, const u64* par_off, uint32_t blocks)
{
	const dim3 grid = fixed_grid((u64)t.gmax << (t.shift - PA_TILE_SHIFT), 1u, 2u * blocks);   // (workgroups of four waves: eight to a CU, a full one, where the CRC kernel has four)
	const uint32_t mis1 = mis ? 1u : 0u;
	if (t.m == 1u) { hipLaunchKernelGGL(pa_build_kernel<1u>, grid, dim3(PA_THREADS), 0, st, v, t, mis1, row_len, par, par_cap, par_off); }
	else if (t.m == 2u) { hipLaunchKernelGGL(pa_build_kernel<2u>, grid, dim3(PA_THREADS), 0, st, v, t, mis1, row_len, par, par_cap, par_off); }
	else { hipLaunchKernelGGL(pa_build_kernel<3u>, grid, dim3(PA_THREADS), 0, st, v, t, mis1, row_len, par, par_cap, par_off); }
}
void launch_parity_head(hipStream_t st, const SpliceView& v, const ParityTab& t, bool mis, const u64* par_off, u64 par_cap, uint32_t* par_crc, u64* par_head, int32_t* status,
                        uint32_t blocks)
{
	hipLaunchKernelGGL(pa_head_kernel, fixed_grid((u64)t.gmax * t.m + 1u, 256u, blocks), dim3(256), 0, st, v, t, mis ? 1u : 0u, par_off, par_cap, par_crc, par_head, status);
}
void launch_parity_check(hipStream_t st, const ParityTab& t, const u64* par_off, u64 par_len, uint32_t blocks)
{
	const u64 Q = (u64)t.gmax * t.m;
	hipLaunchKernelGGL(pa_check_kernel, fixed_grid((Q > t.nbt ? Q : t.nbt) + 1u, 256u, blocks), dim3(256), 0, st, t, par_off, par_len);
}
void launch_parity_damage(hipStream_t st, const SpliceView& v, const ParityTab& t, bool mis, const uint32_t* verdict, const u64* par_off, u64 par_len, const uint32_t* par_crc,
                          const uint32_t* row_len, const u64* head, uint32_t blocks)
{
	hipLaunchKernelGGL(pa_damage_kernel, fixed_grid(t.gmax, 256u, blocks), dim3(256), 0, st, v, t, mis ? 1u : 0u, verdict, par_off, par_len, par_crc, row_len, head);
}
void launch_parity_solve(hipStream_t st, const SpliceView& v, const ParityTab& t, bool mis, const uint8_t* par, const u64* par_off, const uint32_t* row_len, const u64* head,
                         uint8_t* fix, u64 fix_cap, const u64* fix_off, uint32_t blocks)
{
	hipLaunchKernelGGL(pa_solve_kernel, fixed_grid((u64)t.gmax << (t.shift - PA_TILE_SHIFT), 1u, 2u * blocks), dim3(PA_THREADS), 0, st, v, t, mis ? 1u : 0u, par, par_off, row_len,
	                   head, fix, fix_cap, fix_off);
}
void launch_parity_tail(hipStream_t st, const SpliceView& v, const ParityTab& t, bool mis, const u64* head, u64 fix_cap, const u64* fix_off, uint32_t* fix_verdict, u64* count,
                        int32_t* status, uint32_t blocks)
{
	hipLaunchKernelGGL(pa_tail_kernel, fixed_grid((u64)t.nbt + 1u, 256u, blocks), dim3(256), 0, st, v, t, mis ? 1u : 0u, head, fix_cap, fix_off, fix_verdict, count, status);
}

} // namespace msc
