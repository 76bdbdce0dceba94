// gfmath_host.cpp -- csrc/gfmath.h compiled for the host and printed, for tests/test_gfmath_host.py to hold against tests/parity_model.py:
//   x2     gf_x2 of every byte in every lane of a dword, under three patterns of the other three bytes
//   mulc   gf_mulc: all 65536 products in every lane, the other lanes holding other bytes
//   mul    gf_mul: all 65536 products
//   exp    gf_exp(0 .. 765)
//   inv    gf_inv(1 .. 255)
//   invert gf_invert of alpha^(p_r i_c) for every parity subset of {0, 1, 2}: every member with one parity, every member pair with two,
//          every member triple with three. Checked HERE, A inv = I by a product from log / antilog tables built below (nothing of the
//          header's shift-and-add), with two different fillings of the entries outside the e x e corner, which must not matter; the counts
//          are printed, and every SAMPLE-th matrix (and some of one entry) as a line "M e p.. i.. inv.." for the test to invert again by Gauss-Jordan.
// Not part of the library: built and run by the test alone.
#include <stdio.h>
#include <stdint.h>
#include "gfmath.h"

using namespace msc;

static const uint32_t PATTERNS[3] = {0x00000000u, 0xA55A3CC3u, 0xFFFFFFFFu};
static const unsigned SAMPLE = 2039;

static uint32_t t_exp[510], t_log[256];
static uint32_t t_mul(uint32_t a, uint32_t b) { return a && b ? t_exp[t_log[a] + t_log[b]] : 0u; }

static unsigned long long n_checked, n_bad, n_singular, n_garbage;

static void one(uint32_t e, const uint32_t* p, const uint32_t* i)
{
	uint32_t inv[2][GF_ROWS][GF_ROWS];
	bool ok[2];
	for (uint32_t fill = 0; fill < 2u; ++fill) {
		uint32_t a[GF_ROWS][GF_ROWS];
		for (uint32_t r = 0; r < GF_ROWS; ++r) {
			for (uint32_t c = 0; c < GF_ROWS; ++c) {
				a[r][c] = r < e && c < e ? t_exp[(p[r] * i[c]) % 255u] : fill ? 0xDEADBE00u + 37u * r + c : 0u;
				inv[fill][r][c] = 0x5A5A5A5Au;
			}
		}
		ok[fill] = gf_invert(e, a, inv[fill]);
		if (e == GF_ROWS) { ok[1] = ok[0]; break; }                           // (no entry outside the corner)
	}
	++n_checked;
	if (!ok[0] || !ok[1]) { ++n_singular; return; }
	bool bad = false, differs = false;
	for (uint32_t r = 0; r < e; ++r) {
		for (uint32_t c = 0; c < e; ++c) {
			uint32_t s = 0;
			for (uint32_t x = 0; x < e; ++x) { s ^= t_mul(t_exp[(p[r] * i[x]) % 255u], inv[0][x][c]); }
			bad |= s != (r == c ? 1u : 0u) || inv[0][r][c] > 255u;
			differs |= e < GF_ROWS && inv[1][r][c] != inv[0][r][c];
		}
	}
	n_bad += bad; n_garbage += differs;
	if (n_checked % SAMPLE == 0 || (e == 1u && i[0] % 50u == 28u)) {
		printf("M %u", e);
		for (uint32_t r = 0; r < e; ++r) { printf(" %u", p[r]); }
		for (uint32_t c = 0; c < e; ++c) { printf(" %u", i[c]); }
		for (uint32_t r = 0; r < e; ++r) { for (uint32_t c = 0; c < e; ++c) { printf(" %u", inv[0][r][c]); } }
		printf("\n");
	}
}

int main()
{
	uint32_t x = 1;
	for (uint32_t i = 0; i < 255u; ++i) { t_exp[i] = t_exp[i + 255u] = x; t_log[x] = i; x <<= 1; if (x & 0x100u) { x ^= 0x11Du; } }

	printf("x2");
	for (uint32_t pat = 0; pat < 3u; ++pat) {
		for (uint32_t lane = 0; lane < 4u; ++lane) {
			for (uint32_t v = 0; v < 256u; ++v) { printf(" %x", gf_x2((PATTERNS[pat] & ~(0xFFu << (8u * lane))) | v << (8u * lane))); }
		}
	}
	printf("\nmulc");
	for (uint32_t lane = 0; lane < 4u; ++lane) {
		for (uint32_t c = 0; c < 256u; ++c) {
			for (uint32_t v = 0; v < 256u; ++v) { printf(" %x", gf_mulc((PATTERNS[1] & ~(0xFFu << (8u * lane))) | v << (8u * lane), c)); }
		}
	}
	printf("\nmul");
	for (uint32_t a = 0; a < 256u; ++a) { for (uint32_t b = 0; b < 256u; ++b) { printf(" %x", gf_mul(a, b)); } }
	printf("\nexp");
	for (uint32_t n = 0; n <= 765u; ++n) { printf(" %x", gf_exp(n)); }
	printf("\ninv");
	for (uint32_t a = 1; a < 256u; ++a) { printf(" %x", gf_inv(a)); }
	printf("\n");

	for (uint32_t set = 1; set < 8u; ++set) {                                // the parities of a subset in rising order, as the damage pass lists them
		uint32_t p[GF_ROWS] = {0, 0, 0}, i[GF_ROWS] = {0, 0, 0}, e = 0;
		for (uint32_t b = 0; b < 3u; ++b) { if (set >> b & 1u) { p[e++] = b; } }
		for (i[0] = 0; i[0] < 255u; ++i[0]) {
			if (e == 1u) { one(e, p, i); continue; }
			for (i[1] = i[0] + 1u; i[1] < 255u; ++i[1]) {
				if (e == 2u) { one(e, p, i); continue; }
				for (i[2] = i[1] + 1u; i[2] < 255u; ++i[2]) { one(e, p, i); }
			}
		}
	}
	printf("invert checked %llu bad %llu singular %llu garbage %llu\n", n_checked, n_bad, n_singular, n_garbage);
	return 0;
}
