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
// Four products of bytes at once, byte j of a times byte j of b: shift and add under a mask per byte, by arithmetic alone. The solver's lane
// per group multiplies by bytes of its own; as selects (what a compiler makes of gf_mulc's form there) every step holds a mask in a scalar
// register pair, and the 44 products of gf_invert kept theirs alive side by side and spilled.
__host__ __device__ constexpr uint32_t gf_mul4(uint32_t a, uint32_t b)
{
	uint32_t r = 0;
	for (int i = 0; i < 8; ++i) { const uint32_t bit = (b >> i) & 0x01010101u; r ^= a & ((bit << 8) - bit); a = gf_x2(a); }
	return r;
}
__host__ __device__ constexpr uint32_t gf_pack(uint32_t a0, uint32_t a1, uint32_t a2, uint32_t a3) { return (a0 & 255u) | (a1 & 255u) << 8 | (a2 & 255u) << 16 | a3 << 24; }
__host__ __device__ constexpr uint32_t gf_byte(uint32_t v, uint32_t j) { return (v >> (8u * j)) & 255u; }
__host__ __device__ constexpr uint32_t gf_mul(uint32_t a, uint32_t b) { return gf_mul4(a & 255u, b & 255u); }
// alpha^n
__host__ __device__ constexpr uint32_t gf_exp(uint32_t n)
{
	uint32_t r = 1;
	for (n %= 255u; n; --n) { r = gf_x2(r) & 255u; }
	return r;
}
// 1 / a = a^254 (a != 0) = a^2 a^4 .. a^128: the seven squares, multiplied as a tree three products deep
__host__ __device__ constexpr uint32_t gf_inv(uint32_t a)
{
	uint32_t s[8] = {a & 255u, 0, 0, 0, 0, 0, 0, 0};
	for (uint32_t i = 1; i < 8u; ++i) { s[i] = gf_mul(s[i - 1u], s[i - 1u]); }
	const uint32_t p3 = gf_mul4(gf_pack(s[1], s[3], s[5], 0), gf_pack(s[2], s[4], s[6], 0));
	const uint32_t p2 = gf_mul4(gf_pack(gf_byte(p3, 0), gf_byte(p3, 2), 0, 0), gf_pack(gf_byte(p3, 1), s[7], 0, 0));
	return gf_mul(gf_byte(p2, 0), gf_byte(p2, 1));
}
// The e x e matrix in the upper left of a (e <= GF_ROWS) inverted into inv, by cofactors: a is taken as the identity outside its e x e, so
// one 3 x 3 formula serves every e -- no pivot search, no index that depends on the data, and in characteristic 2 no signs. False: singular.
__host__ __device__ inline bool gf_invert(uint32_t e, const uint32_t (&a)[GF_ROWS][GF_ROWS], uint32_t (&inv)[GF_ROWS][GF_ROWS])
{
	uint32_t m[3][3], x[20] = {}, y[20] = {}, p[5], cof[12] = {};
	#pragma unroll
	for (uint32_t r = 0; r < 3u; ++r) {
		#pragma unroll
		for (uint32_t c = 0; c < 3u; ++c) { m[r][c] = r < e && c < e ? a[r][c] & 255u : r == c ? 1u : 0u; }
	}
	#pragma unroll
	for (uint32_t r = 0; r < 3u; ++r) {                                      // the two products of cofactor (r, c) at 6 r + 2 c, packed four to a dword
		#pragma unroll
		for (uint32_t c = 0; c < 3u; ++c) {
			const uint32_t r1 = r == 0 ? 1u : 0u, r2 = r == 2u ? 1u : 2u, c1 = c == 0 ? 1u : 0u, c2 = c == 2u ? 1u : 2u, at = 6u * r + 2u * c;
			x[at] = m[r1][c1]; y[at] = m[r2][c2]; x[at + 1u] = m[r1][c2]; y[at + 1u] = m[r2][c1];
		}
	}
	#pragma unroll
	for (uint32_t g = 0; g < 5u; ++g) { p[g] = gf_mul4(gf_pack(x[4u * g], x[4u * g + 1u], x[4u * g + 2u], x[4u * g + 3u]), gf_pack(y[4u * g], y[4u * g + 1u], y[4u * g + 2u], y[4u * g + 3u])); }
	#pragma unroll
	for (uint32_t i = 0; i < 9u; ++i) { cof[i] = gf_byte(p[(2u * i) >> 2], (2u * i) & 3u) ^ gf_byte(p[(2u * i + 1u) >> 2], (2u * i + 1u) & 3u); }
	const uint32_t dp = gf_mul4(gf_pack(m[0][0], m[0][1], m[0][2], 0), gf_pack(cof[0], cof[1], cof[2], 0));
	const uint32_t det = gf_byte(dp, 0) ^ gf_byte(dp, 1) ^ gf_byte(dp, 2);
	if (det == 0) { return false; }
	const uint32_t d4 = gf_inv(det) * 0x01010101u;
	#pragma unroll
	for (uint32_t g = 0; g < 3u; ++g) {
		const uint32_t out = gf_mul4(gf_pack(cof[4u * g], cof[4u * g + 1u], cof[4u * g + 2u], cof[4u * g + 3u]), d4);
		#pragma unroll
		for (uint32_t j = 0; j < 4u; ++j) { const uint32_t i = 4u * g + j; if (i < 9u) { inv[i % 3u][i / 3u] = gf_byte(out, j); } }   // (cof[3 c + r] d)
	}
	return true;
}

} // namespace msc
