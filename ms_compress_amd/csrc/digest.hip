// digest.hip -- BLAKE2s block digests (mscomp_amd_digester_*, mscomp_amd_syncer_sync_digest, include/mscomp_amd.h): the strong half of
// the signature a container keeps per block, beside the CRC-32 that rolls. digest(D) is BLAKE2s in its tree mode (RFC 7693, parameter
// block): leaves of 1024 bytes, two levels, unlimited fan-out, 16 bytes inner and final length, no key, salt or personalisation. A leaf
// is a serial chain of at most 16 compressions and a lane takes one; the root hashes the 16 n bytes of its unit's leaf digests, a lane
// per unit. Nothing here rolls and nothing is shared between lanes: the work is the compression function. DESIGN.md 4.21.
#include "kernels.h"

namespace msc {

#define DG_THREADS 256u
#define DG_ROOT_THREADS 64u                               // a root is a serial chain: a wave per workgroup spreads few units over many CUs
// the parameter block's words that are not zero (digest_length 16, key_length 0, fanout 0, depth 2 | leaf_length | node_offset | node_depth, inner_length 16)
#define DG_P0 0x02000010u
#define DG_P1 DG_LEAF
#define DG_P3(depth) (0x10000000u | ((depth) << 16))
#define DG_IV0 0x6A09E667u
#define DG_IV1 0xBB67AE85u
#define DG_IV2 0x3C6EF372u
#define DG_IV3 0xA54FF53Au
#define DG_IV4 0x510E527Fu
#define DG_IV5 0x9B05688Cu
#define DG_IV6 0x1F83D9ABu
#define DG_IV7 0x5BE0CD19u

__host__ __device__ __forceinline__ uint32_t dg_rotr(uint32_t x, uint32_t n)
{
#if defined(__HIP_DEVICE_COMPILE__)
	return __builtin_amdgcn_alignbit(x, x, n);
#else
	return (x >> n) | (x << (32u - n));
#endif
}

#define DG_G(a, b, c, d, x, y) \
	a += b + (x); d = dg_rotr(d ^ a, 16u); c += d; b = dg_rotr(b ^ c, 12u); \
	a += b + (y); d = dg_rotr(d ^ a, 8u);  c += d; b = dg_rotr(b ^ c, 7u);
// a round with its message schedule written out: every index is a constant, so m stays in registers
#define DG_ROUND(s0, s1, s2, s3, s4, s5, s6, s7, s8, s9, s10, s11, s12, s13, s14, s15) \
	DG_G(v0, v4, v8,  v12, m[s0],  m[s1])  DG_G(v1, v5, v9,  v13, m[s2],  m[s3])  DG_G(v2, v6, v10, v14, m[s4],  m[s5])  DG_G(v3, v7, v11, v15, m[s6],  m[s7]) \
	DG_G(v0, v5, v10, v15, m[s8],  m[s9])  DG_G(v1, v6, v11, v12, m[s10], m[s11]) DG_G(v2, v7, v8,  v13, m[s12], m[s13]) DG_G(v3, v4, v9,  v14, m[s14], m[s15])

// The BLAKE2s compression: h over the 64-byte message block m, t = the bytes hashed up to and including it (below 2^32 here), f0 / f1 =
// all ones on the last block / on the last block of the last node of a level.
__host__ __device__ __forceinline__ void dg_compress(uint32_t (&h)[8], const uint32_t (&m)[16], uint32_t t, uint32_t f0, uint32_t f1)
{
	uint32_t v0 = h[0], v1 = h[1], v2 = h[2], v3 = h[3], v4 = h[4], v5 = h[5], v6 = h[6], v7 = h[7];
	uint32_t v8 = DG_IV0, v9 = DG_IV1, v10 = DG_IV2, v11 = DG_IV3, v12 = DG_IV4 ^ t, v13 = DG_IV5, v14 = DG_IV6 ^ f0, v15 = DG_IV7 ^ f1;
	DG_ROUND( 0,  1,  2,  3,  4,  5,  6,  7,  8,  9, 10, 11, 12, 13, 14, 15)
	DG_ROUND(14, 10,  4,  8,  9, 15, 13,  6,  1, 12,  0,  2, 11,  7,  5,  3)
	DG_ROUND(11,  8, 12,  0,  5,  2, 15, 13, 10, 14,  3,  6,  7,  1,  9,  4)
	DG_ROUND( 7,  9,  3,  1, 13, 12, 11, 14,  2,  6,  5, 10,  4,  0, 15,  8)
	DG_ROUND( 9,  0,  5,  7,  2,  4, 10, 15, 14,  1, 11, 12,  6,  8,  3, 13)
	DG_ROUND( 2, 12,  6, 10,  0, 11,  8,  3,  4, 13,  7,  5, 15, 14,  1,  9)
	DG_ROUND(12,  5,  1, 15, 14, 13,  4, 10,  0,  7,  6,  3,  9,  2,  8, 11)
	DG_ROUND(13, 11,  7, 14, 12,  1,  3,  9,  5,  0, 15,  4,  8,  6,  2, 10)
	DG_ROUND( 6, 15, 14,  9, 11,  3,  0,  8, 12,  2, 13,  7,  1,  4, 10,  5)
	DG_ROUND(10,  2,  8,  4,  7,  6,  1,  5, 15, 11,  9, 14,  3, 12, 13,  0)
	h[0] ^= v0 ^ v8; h[1] ^= v1 ^ v9; h[2] ^= v2 ^ v10; h[3] ^= v3 ^ v11; h[4] ^= v4 ^ v12; h[5] ^= v5 ^ v13; h[6] ^= v6 ^ v14; h[7] ^= v7 ^ v15;
}

// One node of the tree: the 16-byte digest of the len >= 1 bytes at p (any alignment) as node `node` of level `depth`, `last` = the
// last node of its level. A full 64-byte message block is four 16-byte loads; the short last one is read byte by byte and padded with
// zeros, and never a byte behind p + len. A node whose length is a multiple of 64 finalises on its last full block.
__host__ __device__ __forceinline__ void dg_node(const uint8_t* __restrict__ p, uint32_t len, uint32_t node, uint32_t depth, bool last, uint32_t (&out)[4])
{
	uint32_t h[8] = { DG_IV0 ^ DG_P0, DG_IV1 ^ DG_P1, DG_IV2 ^ node, DG_IV3 ^ DG_P3(depth), DG_IV4, DG_IV5, DG_IV6, DG_IV7 };
	const uint32_t nblk = (len + 63u) >> 6;
	#pragma unroll 1
	for (uint32_t j = 0; j < nblk; ++j) {
		const uint32_t at = j << 6, left = len - at;
		const uint8_t* __restrict__ q = p + at;
		uint32_t m[16];
		if (left >= 64u) {
			const cpd_u16* __restrict__ s = reinterpret_cast<const cpd_u16*>(q);
			const cpd_u16 a = s[0], b = s[1], c = s[2], d = s[3];
			m[0] = a.w[0]; m[1] = a.w[1]; m[2] = a.w[2]; m[3] = a.w[3]; m[4] = b.w[0]; m[5] = b.w[1]; m[6] = b.w[2]; m[7] = b.w[3];
			m[8] = c.w[0]; m[9] = c.w[1]; m[10] = c.w[2]; m[11] = c.w[3]; m[12] = d.w[0]; m[13] = d.w[1]; m[14] = d.w[2]; m[15] = d.w[3];
		} else {
			#pragma unroll
			for (uint32_t w = 0; w < 16u; ++w) {
				uint32_t x = 0;
				#pragma unroll
				for (uint32_t k = 0; k < 4u; ++k) { if (4u * w + k < left) { x |= (uint32_t)q[4u * w + k] << (8u * k); } }
				m[w] = x;
			}
		}
		const bool fin = j + 1u == nblk;
		dg_compress(h, m, fin ? len : at + 64u, fin ? 0xFFFFFFFFu : 0u, fin && last ? 0xFFFFFFFFu : 0u);
	}
	out[0] = h[0]; out[1] = h[1]; out[2] = h[2]; out[3] = h[3];
}

// a unit's length as the passes take it: nothing behind the creation's block size is read whatever the table says
__device__ __forceinline__ uint32_t dg_len(const DigestTab& d, u64 u)
{
	const u64 L = d.len[u], B = (u64)1 << d.shift;
	return (uint32_t)(L < B ? L : B);
}
__device__ __forceinline__ u64 dg_units(const DigestTab& d)
{
	const u64 c = d.count[0];
	return c < d.n_max ? c : d.n_max;
}

// The leaf pass, a fixed grid dealt over the leaf slots of the units of this execution: slot i is leaf i & (B / 1024 - 1) of unit
// i >> (shift - 10). A slot behind its unit's data is skipped; only the last leaf of a unit carries the last-node flag.
__global__ __launch_bounds__(DG_THREADS) void dg_leaf_kernel(DigestTab d, const uint8_t* __restrict__ base)
{
	const uint32_t lps = d.shift - DG_LEAF_SHIFT;
	const u64 items = dg_units(d) << lps;
	for (u64 i = (u64)blockIdx.x * DG_THREADS + threadIdx.x; i < items; i += (u64)gridDim.x * DG_THREADS) {
		const u64 u = i >> lps;
		const uint32_t k = (uint32_t)(i & (((u64)1 << lps) - 1u)), len = dg_len(d, u), at = k << DG_LEAF_SHIFT;
		if (at >= len) { continue; }
		const uint32_t ll = len - at < DG_LEAF ? len - at : DG_LEAF;
		uint32_t h[4];
		dg_node(base + d.off[u] + at, ll, k, 0u, at + ll == len, h);
		reinterpret_cast<uint4*>(d.leaf)[i] = make_uint4(h[0], h[1], h[2], h[3]);      // (the leaf column is 16-byte aligned: first in its buffer)
	}
}

// The root pass, a lane per possible unit: the leaf digests of the unit, 16 bytes each and back to back in its slots, hashed as the one
// node of level 1 -- of a one-leaf unit too, whose leaf and root both carry the last-node flag. The same launch copies the resources'
// statuses when it is given them.
__global__ __launch_bounds__(DG_ROOT_THREADS) void dg_root_kernel(DigestTab d, uint32_t* __restrict__ out, uint32_t n_res, const int32_t* __restrict__ rstat,
                                                                 int32_t* __restrict__ d_status)
{
	const uint32_t u = blockIdx.x * DG_ROOT_THREADS + threadIdx.x;
	if (rstat && u < n_res) { d_status[u] = rstat[u]; }
	if (u >= d.n_max) { return; }
	uint32_t h[4] = {0, 0, 0, 0};
	if (u < dg_units(d)) {
		const uint32_t len = dg_len(d, u);
		if (len) {
			const uint32_t n = (len + DG_LEAF - 1u) >> DG_LEAF_SHIFT;
			dg_node(reinterpret_cast<const uint8_t*>(d.leaf + 4u * ((u64)u << (d.shift - DG_LEAF_SHIFT))), 16u * n, 0u, 1u, true, h);
		}
	}
	out[4u * (u64)u] = h[0]; out[4u * (u64)u + 1u] = h[1]; out[4u * (u64)u + 2u] = h[2]; out[4u * (u64)u + 3u] = h[3];
}

void launch_digest_leaves(hipStream_t st, const uint8_t* base, const DigestTab& d, uint32_t blocks)
{
	if (d.n_max == 0) { return; }
	hipLaunchKernelGGL(dg_leaf_kernel, fixed_grid((u64)d.n_max << (d.shift - DG_LEAF_SHIFT), DG_THREADS, blocks), dim3(DG_THREADS), 0, st, d, base);
}

void launch_digest_roots(hipStream_t st, const DigestTab& d, uint32_t* out, uint32_t n_res, const int32_t* rstat, int32_t* d_status)
{
	const uint32_t items = d.n_max > n_res || !rstat ? d.n_max : n_res;
	if (items == 0) { return; }
	hipLaunchKernelGGL(dg_root_kernel, dim3((items + DG_ROOT_THREADS - 1u) / DG_ROOT_THREADS), dim3(DG_ROOT_THREADS), 0, st, d, out, n_res, rstat, d_status);
}

} // namespace msc
