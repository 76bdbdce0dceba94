// gfmath.h -- GF(2^8) as the parity kernels take it (parity.hip; mscomp_amd_parity_*, include/mscomp_amd.h): polynomial x^8 + x^4 + x^3 +
// x^2 + 1 (0x11D), generator alpha = 2 -- the field of RAID-6 and PAR2. Host and device code without tables: the build pass needs "times
// alpha" alone, on four bytes packed in a dword, and everything else serves the solver, which is the rare path. DESIGN.md 4.22.
#pragma once
#include <stdint.h>
#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#endif

namespace msc {

#define GF_POLY 0x1Du                                    // the polynomial below x^8
#define GF_ROWS 3u                                       // the largest system the solver inverts (MSCOMP_AMD_PARITY_M_MAX)

// alpha times each of the four bytes of v
__host__ __device__ constexpr uint32_t gf_x2(uint32_t v) { return ((v & 0x7F7F7F7Fu) << 1) ^ (((v >> 7) & 0x01010101u) * GF_POLY); }
// c (a byte, the same in every lane that matters: no table, no divergence) times each of the four bytes of v, by shift and add
__host__ __device__ constexpr uint32_t gf_mulc(uint32_t v, uint32_t c)
{
	uint32_t r = 0;
	for (int i = 0; i < 8; ++i) { r ^= v & (0u - ((c >> i) & 1u)); v = gf_x2(v); }
	return r;
}
__host__ __device__ constexpr uint32_t gf_mul(uint32_t a, uint32_t b) { return gf_mulc(a & 255u, b & 255u) & 255u; }
// alpha^n
__host__ __device__ constexpr uint32_t gf_exp(uint32_t n)
{
	uint32_t r = 1;
	for (n %= 255u; n; --n) { r = gf_x2(r) & 255u; }
	return r;
}
// 1 / a = a^254 (a != 0): seven squarings, the last six multiplied in
__host__ __device__ constexpr uint32_t gf_inv(uint32_t a)
{
	uint32_t r = 1, s = a;
	for (int i = 1; i < 8; ++i) { s = gf_mul(s, s); r = gf_mul(r, s); }
	return r;
}
// The e x e matrix in the upper left of a (e <= GF_ROWS) inverted into inv, by cofactors: a is taken as the identity outside its e x e, so
// one 3 x 3 formula serves every e -- no pivot search, no index that depends on the data, and in characteristic 2 no signs. False: singular.
__host__ __device__ inline bool gf_invert(uint32_t e, const uint32_t (&a)[GF_ROWS][GF_ROWS], uint32_t (&inv)[GF_ROWS][GF_ROWS])
{
	uint32_t m[3][3], cof[3][3];
	for (uint32_t r = 0; r < 3u; ++r) { for (uint32_t c = 0; c < 3u; ++c) { m[r][c] = r < e && c < e ? a[r][c] & 255u : r == c ? 1u : 0u; } }
	for (uint32_t r = 0; r < 3u; ++r) {
		for (uint32_t c = 0; c < 3u; ++c) {
			const uint32_t r1 = r == 0 ? 1u : 0u, r2 = r == 2u ? 1u : 2u, c1 = c == 0 ? 1u : 0u, c2 = c == 2u ? 1u : 2u;
			cof[r][c] = gf_mul(m[r1][c1], m[r2][c2]) ^ gf_mul(m[r1][c2], m[r2][c1]);
		}
	}
	const uint32_t det = gf_mul(m[0][0], cof[0][0]) ^ gf_mul(m[0][1], cof[0][1]) ^ gf_mul(m[0][2], cof[0][2]);
	if (det == 0) { return false; }
	const uint32_t d = gf_inv(det);
	for (uint32_t r = 0; r < 3u; ++r) { for (uint32_t c = 0; c < 3u; ++c) { inv[r][c] = gf_mul(cof[c][r], d); } }
	return true;
}

} // namespace msc
