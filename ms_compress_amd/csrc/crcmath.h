// crcmath.h -- the CRC-32 algebra and tables the CRC kernels (crc32.hip) and the syncer's scan (sync.hip) share. Device code and constexpr
// builders only; a file that includes it gets its own copy of the tables (a const at namespace scope has internal linkage).
//
// CRC-32 is linear over GF(2): with raw(M) the register after M from an initial value of 0, and |M| in bytes,
//   raw(A || B) = raw(A) * x^(8 |B|)  ^  raw(B)                 (mod P; leading zero bytes leave raw() alone)
//   crc32(M)    = raw(M)  ^  0xFFFFFFFF * x^(8 |M|)  ^  0xFFFFFFFF
// A register is a polynomial with the coefficient of x^0 in bit 31 (zlib's multmodp form), so "a zero byte more" is "times x^8".
#pragma once
#include "../../include/mscomp_amd.h"
#include "common.h"

namespace msc {

#define CRC_POLY 0xEDB88320u
#define CRC_ONE  0x80000000u                              // x^0
#define CRC_ROW  MSCOMP_AMD_CRC_ROW_BYTES                 // bytes a wave takes per step: 64 lanes x 64 bytes
#define CRC_RUN  (CRC_ROW / 64u)                          // ... a lane's run in it: four 16-byte loads

// a * b mod P, the bits of a from x^0 up
__host__ __device__ constexpr uint32_t crc_mul(uint32_t a, uint32_t b)
{
	uint32_t p = 0;
	for (int i = 0; i < 32; ++i) { p ^= b & (0u - (a >> 31)); a <<= 1; b = (b >> 1) ^ (CRC_POLY & (0u - (b & 1u))); }
	return p;
}

// What the kernels read: slicing tables t[j][b] = raw(b, then j zero bytes); a[k][b] = (b in byte k of a register) * x^(8 (CRC_ROW - CRC_RUN)):
// a lane's register carried over the other lanes' runs of a row; c[l] = x^(8 CRC_RUN (63 - l)): lane l's run to the end of the row;
// x2n[k] = x^(2^k). Built by the compiler.
struct CrcTables { uint32_t t[16][256]; uint32_t a[4][256]; uint32_t c[64]; uint32_t x2n[64]; };
constexpr CrcTables make_crc_tables()
{
	CrcTables r{};
	for (uint32_t b = 0; b < 256u; ++b) {
		uint32_t v = b;
		for (int i = 0; i < 8; ++i) { v = (v >> 1) ^ (CRC_POLY & (0u - (v & 1u))); }
		r.t[0][b] = v;
	}
	for (uint32_t j = 1; j < 16u; ++j) { for (uint32_t b = 0; b < 256u; ++b) { const uint32_t v = r.t[j - 1u][b]; r.t[j][b] = (v >> 8) ^ r.t[0][v & 255u]; } }
	r.x2n[0] = CRC_ONE >> 1;
	for (uint32_t k = 1; k < 64u; ++k) { r.x2n[k] = crc_mul(r.x2n[k - 1u], r.x2n[k - 1u]); }
	uint32_t run = CRC_ONE, adv = CRC_ONE;                               // x^(8 CRC_RUN), x^(8 (CRC_ROW - CRC_RUN))
	for (uint32_t k = 0, n = 8u * CRC_RUN; n; ++k, n >>= 1) { if (n & 1u) { run = crc_mul(run, r.x2n[k]); } }
	for (uint32_t k = 0, n = 8u * (CRC_ROW - CRC_RUN); n; ++k, n >>= 1) { if (n & 1u) { adv = crc_mul(adv, r.x2n[k]); } }
	r.c[63] = CRC_ONE;
	for (uint32_t l = 63; l-- > 0;) { r.c[l] = crc_mul(r.c[l + 1u], run); }
	for (uint32_t k = 0; k < 4u; ++k) {                                   // linear in b: the eight single bits, then their sums
		r.a[k][0] = 0;
		for (uint32_t b = 1; b < 256u; ++b) { const uint32_t low = b & (0u - b); r.a[k][b] = low == b ? crc_mul(b << (8u * k), adv) : r.a[k][b ^ low] ^ r.a[k][low]; }
	}
	return r;
}
__device__ const CrcTables g_crc_tab = make_crc_tables();

// x^n (n = 8 d < 2^53): square and multiply over the bits of n
__device__ __forceinline__ uint32_t crc_xpow(u64 n)
{
	uint32_t r = CRC_ONE;
	for (uint32_t k = 0; n; ++k, n >>= 1) { if (n & 1u) { r = crc_mul(r, g_crc_tab.x2n[k]); } }
	return r;
}
// the two terms of crc32() that do not depend on the data
__device__ __forceinline__ uint32_t crc_seed(u64 len) { return len ? crc_mul(0xFFFFFFFFu, crc_xpow(len << 3)) ^ 0xFFFFFFFFu : 0u; }

// sixteen bytes more on a register, by the slicing tables
__device__ __forceinline__ uint32_t crc_step16(const uint32_t (*t)[256], uint32_t st, uint4 v)
{
	const uint32_t x = v.x ^ st;
	return t[15][x & 255u] ^ t[14][(x >> 8) & 255u] ^ t[13][(x >> 16) & 255u] ^ t[12][x >> 24] ^
	       t[11][v.y & 255u] ^ t[10][(v.y >> 8) & 255u] ^ t[9][(v.y >> 16) & 255u] ^ t[8][v.y >> 24] ^
	       t[7][v.z & 255u] ^ t[6][(v.z >> 8) & 255u] ^ t[5][(v.z >> 16) & 255u] ^ t[4][v.z >> 24] ^
	       t[3][v.w & 255u] ^ t[2][(v.w >> 8) & 255u] ^ t[1][(v.w >> 16) & 255u] ^ t[0][v.w >> 24];
}
// the 16 bytes at the 16-aligned address q of a part that starts at p: whole, or its bytes from p on behind zeros, or -- all in front of p -- zeros
__device__ __forceinline__ uint4 crc_load_front(uintptr_t q, uintptr_t p)
{
	if (q >= p) { return *reinterpret_cast<const uint4*>(q); }
	uint32_t w[4] = {0, 0, 0, 0};
	if (q + 16u > p) { for (uint32_t j = (uint32_t)(p - q); j < 16u; ++j) { w[j >> 2] |= (uint32_t)*reinterpret_cast<const uint8_t*>(q + j) << (8u * (j & 3u)); } }
	return make_uint4(w[0], w[1], w[2], w[3]);
}

} // namespace msc
