// lz_tag_study.c -- CPU study (dev tool): would a 4-bit tag in the spare bits of the 16-bit bucket entries pay? Per token start of the greedy
// parse of 4 KiB chunks (the positions lznt1_chunk4_kernel's lazy walk lands on) it counts the finishing events (the position is not settled by
// what its lane scans by itself) and the finishing steps (64 candidates each) under three rules:
//   now   -- 12-bit hash buckets, the lane scans the 4 oldest entries;
//   tag   -- the same buckets, every entry carries bits 16-19 of the hash product: the lane looks at the 8 oldest entries and scans the first 4
//            whose tag equals its own; the finishing steps start behind what the lane has seen;
//   exact -- buckets of the 16-bit key (hash product >> 16): the ideal that no tag can beat.
// A position is settled when a scanned candidate reached max_len or no older entry of its bucket is left unseen.
//   usage: lz_tag_study <file> [first byte = 0] [bytes = 4 MiB]
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdint.h>
static uint32_t prod(const uint8_t* d) { uint32_t k = d[0] | (d[1] << 8) | (d[2] << 16); return k * 0x9E3779B1u; }
static uint32_t hash12(uint32_t x) { uint32_t h = x >> 20; return h ? h : 1; }
static uint32_t shift_of(uint32_t pos) { if (pos <= 16) return 12; uint32_t b = 32 - __builtin_clz(pos - 1); return 12 - (b - 4); }
static uint32_t lcp(const uint8_t* c, uint32_t q, uint32_t p, uint32_t maxlen) { uint32_t l = 0; while (l < maxlen && c[q + l] == c[p + l]) l++; return l; }
int main(int argc, char** argv)
{
	if (argc < 2) { fprintf(stderr, "usage: lz_tag_study <file> [first byte] [bytes]\n"); return 2; }
	FILE* f = fopen(argv[1], "rb"); if (!f) return 1;
	fseek(f, 0, SEEK_END); size_t N = ftell(f); fseek(f, 0, SEEK_SET);
	uint8_t* all = malloc(N + 64); memset(all + N, 0, 64); if (fread(all, 1, N, f) != N) return 1; fclose(f);
	size_t first = argc > 2 ? strtoul(argv[2], 0, 0) : 0, len = argc > 3 ? strtoul(argv[3], 0, 0) : (4u << 20);
	if (first > N) first = N;
	if (len > N - first) len = N - first;
	const uint8_t* d = all + first;
	double chunks = 0, ev[3] = {0}, st[3] = {0}, tok = 0;
	static uint16_t list[4096]; static uint32_t x[4096];
	for (size_t cb = 0; cb < len; cb += 4096) {
		const uint8_t* c = d + cb; const uint32_t n = len - cb < 4096 ? len - cb : 4096; chunks++;
		for (uint32_t p = 0; p + 2 < n; ++p) x[p] = prod(c + p);
		uint32_t p = 0;
		while (p < n) {
			tok++;
			uint32_t best = 0;
			if (p > 0 && p + 3 <= n) {
				const uint32_t mask3 = (1u << shift_of(p)) + 2, maxlen = n - p < mask3 ? n - p : mask3;
				// the older entries of my 12-bit bucket, oldest first
				uint32_t nc = 0; const uint32_t h = hash12(x[p]);
				for (uint32_t q = 0; q < p; ++q) if (hash12(x[q]) == h) list[nc++] = q;
				// exact Find (oldest first, strictly longer wins, stop at max_len) and the index of the entry that reached max_len
				uint32_t reach = nc;
				for (uint32_t j = 0; j < nc; ++j) { const uint32_t l = lcp(c, list[j], p, maxlen); if (l >= 3 && l > best) best = l; if (l == maxlen) { reach = j; break; } }
				// now: entries 0..3 by the lane; settled if reach < 4 or nc <= 4
				if (nc > 4 && reach >= 4) { ev[0]++; const uint32_t last = reach < nc ? reach : nc - 1; st[0] += (last - 4) / 64 + 1; }
				// tag: of entries 0..7 the first four with my tag; seen = entries up to the fourth such one (or 8)
				{
					const uint32_t tag = (x[p] >> 16) & 15u; uint32_t seen = nc < 8 ? nc : 8, m = 0; int reached = 0;
					for (uint32_t j = 0; j < (nc < 8 ? nc : 8); ++j) {
						if (((x[list[j]] >> 16) & 15u) != tag) continue;
						if (j == reach) reached = 1;
						if (++m == 4) { seen = j + 1; break; }
					}
					// (an entry with another tag holds another key: it can neither match nor reach max_len. The lane cannot know what the entries it has
					// not looked at hold: any entry left unseen leaves the position unsettled.)
					const int left = seen < nc;
					if (!reached && left) { ev[1]++; const uint32_t last = reach < nc ? reach : nc - 1; st[1] += (last - seen) / 64 + 1; }
				}
				// exact: the entries with my 16-bit key only
				{
					uint32_t nk = 0, rk = ~0u;
					for (uint32_t j = 0; j < nc; ++j) if ((x[list[j]] >> 16) == (x[p] >> 16)) { if (j == reach) rk = nk; nk++; }
					if (nk > 4 && (rk == ~0u || rk >= 4)) { ev[2]++; const uint32_t last = rk != ~0u ? rk : nk - 1; st[2] += (last - 4) / 64 + 1; }
				}
			}
			p += best >= 3 ? best : 1;
		}
	}
	const char* nm = strrchr(argv[1], '/'); nm = nm ? nm + 1 : argv[1];
	printf("%-10s chunks %.0f tokens/chunk %.0f | finishing events / steps per chunk: now %.1f / %.1f | first 4 tag-matching of 8 %.1f / %.1f | exact 16-bit keys %.1f / %.1f\n",
	       nm, chunks, tok / chunks, ev[0] / chunks, st[0] / chunks, ev[1] / chunks, st[1] / chunks, ev[2] / chunks, st[2] / chunks);
	free(all);
	return 0;
}
