// lz_empty_study.c -- CPU model (dev tool): two questions about the eager scan of LZNT1's window parse (csrc/lznt1.hip lz_window), in which every
// active lane compares its LZ_SELF = 4 oldest candidates, all four stages for the whole wave:
//   1. would a wave-uniform skip of a candidate stage that NO lane needs pay? The depth of a window is the largest number of eager candidates
//      (0 to 4) that any active lane has; a stage k is skippable in the windows of depth <= k.
//   2. would running the second compare stage (bytes 8..15) per candidate index pay? In the windows where it runs at all (a candidate of some
//      active lane agrees on 8 bytes while max_len > 8), how many of the four candidate indices need it?
// The model parses every 4 KiB chunk as the kernel does (lz_stage_study.c: 12-bit hash, position-ordered buckets, max_len rule, greedy walk window
// by window, finishing steps that stop at max_len) and prints per member: parsed windows per chunk, active lanes per window, the fraction of the
// windows at each depth, the fraction whose second stage runs and, of all windows, the fraction in which 1 / 2 / 3 / 4 candidate indices need it.
//
// Result over the 12 members (51 746 chunks): depth 4 in 0.928 of the parsed windows (0.002 / 0.018 / 0.024 / 0.028 at depths 0 to 3; per member
// from 0.862, ooffice, to 1.000, nci / osdb / sao), 60.6 active lanes on average: a skip pays four scalar tests per window to save a stage in
// 7 % of them. The second stage runs in 0.608 of the windows, with 1 / 2 / 3 / 4 indices needing it in 0.117 / 0.079 / 0.046 / 0.367 of all
// windows: 0.55 skipped candidate-stages per window, about 6 vector instructions, against four more scalar tests. Both closed (DESIGN.md
// section 8, profiles/HISTORY.md round 21).
//   build: gcc -O2 -o lz_empty_study tools/dev/lz_empty_study.c      usage: lz_empty_study [file index 0..11 ...]   (default: all 12 corpus files)
#include "../../ms_compress_amd/csrc/corpus.c"
#include <stdio.h>
#include <stdlib.h>

#define SELF 4u
static uint32_t hash_of(const uint8_t* c) { const uint32_t k = c[0] | c[1] << 8 | c[2] << 16, h = (k * 0x9E3779B1u) >> 20; return h ? h : 1u; }
static uint32_t shift_of(uint32_t p) { return p <= 16 ? 12 : 12 - ((32 - __builtin_clz(p - 1)) - 4); }
static uint32_t lcp(const uint8_t* c, uint32_t q, uint32_t p, uint32_t lim) { uint32_t l = 0; while (l < lim && c[q + l] == c[p + l]) { ++l; } return l; }

typedef struct { double windows, active, depth[SELF + 1], stage2, need[SELF + 1]; } Cnt;

static void chunk(const uint8_t* src, uint32_t n, Cnt* k)
{
	static uint8_t c[4096 + 64];
	static uint16_t bucket[4096], rankof[4096]; static uint32_t start[4097], cnt[4097];
	memset(c, 0, sizeof c); memcpy(c, src, n);
	memset(cnt, 0, sizeof cnt);
	for (uint32_t p = 0; p + 2 < n; ++p) { cnt[hash_of(c + p)]++; }
	start[0] = 0; for (uint32_t h = 1; h <= 4096; ++h) { start[h] = start[h - 1] + cnt[h - 1]; }
	memset(cnt, 0, sizeof cnt);
	for (uint32_t p = 0; p + 2 < n; ++p) { const uint32_t h = hash_of(c + p); rankof[p] = (uint16_t)cnt[h]; bucket[start[h] + cnt[h]++] = (uint16_t)p; }
	uint32_t entry = 0;
	for (uint32_t wb = 0; wb < n; wb += 64) {
		const uint32_t we = wb + 64 < n ? wb + 64 : n;
		if (entry >= we) { continue; }
		uint32_t key[64] = {0}, maxl[64] = {0}, depth = 0, active = 0;
		int needs[SELF] = {0};
		for (uint32_t p = entry > wb ? entry : wb; p < we; ++p) {
			if (p == 0 || p + 3 > n) { continue; }
			const uint32_t i = p - wb, m3 = (1u << shift_of(p)) + 2, s = start[hash_of(c + p)];
			maxl[i] = n - p < m3 ? n - p : m3;
			active++;
			const uint32_t have = rankof[p] < SELF ? rankof[p] : SELF;
			if (have > depth) { depth = have; }
			for (uint32_t j = 0; j < have; ++j) {
				const uint32_t q = bucket[s + j], l = lcp(c, q, p, maxl[i]), kk = (l << 12) | (q ^ 4095u);
				needs[j] |= l >= 8 && maxl[i] > 8;
				if (kk > key[i]) { key[i] = kk; }
			}
		}
		k->windows++; k->active += active; k->depth[depth]++;
		const int nneed = needs[0] + needs[1] + needs[2] + needs[3];
		k->stage2 += nneed > 0; k->need[nneed]++;
		// the greedy walk; a token start with a fifth candidate and max_len not reached is finished over all its candidates
		uint32_t p = entry > wb ? entry : wb;
		while (p < we) {
			const uint32_t i = p - wb;
			uint32_t kb = key[i];
			if (maxl[i] && rankof[p] > SELF && (kb >> 12) < maxl[i]) {
				const uint32_t s = start[hash_of(c + p)];
				for (uint32_t j = SELF; j < rankof[p] && (kb >> 12) < maxl[i]; ++j) {
					const uint32_t q = bucket[s + j], l = lcp(c, q, p, maxl[i]), kk = (l << 12) | (q ^ 4095u);
					if (kk > kb) { kb = kk; }
				}
			}
			p += (kb >> 12) >= 3 ? (kb >> 12) : 1;
		}
		entry = p;
	}
}

static void line(const char* name, double ch, const Cnt* k)
{
	const double w = k->windows ? k->windows : 1.0;
	printf("%-8s %7.0f | %7.1f %6.1f | %5.3f %5.3f %5.3f %5.3f %5.3f | %5.3f | %5.3f %5.3f %5.3f %5.3f\n", name, ch, k->windows / ch, k->active / w,
	       k->depth[0] / w, k->depth[1] / w, k->depth[2] / w, k->depth[3] / w, k->depth[4] / w, k->stage2 / w,
	       k->need[1] / w, k->need[2] / w, k->need[3] / w, k->need[4] / w);
}

int main(int argc, char** argv)
{
	int files[12], nf = 0;
	for (int a = 1; a < argc && nf < 12; ++a) { files[nf++] = atoi(argv[a]); }
	if (nf == 0) { for (int i = 0; i < 12; ++i) { files[nf++] = i; } }
	Cnt all = {0}; double chunks_all = 0;
	printf("%-8s %7s | %7s %6s | %5s %5s %5s %5s %5s | %5s | %5s %5s %5s %5s\n", "file", "chunks", "windows", "active", "d=0", "d=1", "d=2", "d=3", "d=4", "st2", "n=1", "n=2", "n=3", "n=4");
	for (int f = 0; f < nf; ++f) {
		const uint64_t N = mscorpus_file_size(files[f]);
		uint8_t* d = malloc(N); mscorpus_generate(files[f], d, N);
		Cnt k = {0}; double ch = 0;
		for (uint64_t o = 0; o < N; o += 4096) { chunk(d + o, (uint32_t)(N - o < 4096 ? N - o : 4096), &k); ch++; }
		line(mscorpus_file_name(files[f]), ch, &k);
		all.windows += k.windows; all.active += k.active; all.stage2 += k.stage2;
		for (uint32_t i = 0; i <= SELF; ++i) { all.depth[i] += k.depth[i]; all.need[i] += k.need[i]; }
		chunks_all += ch;
		free(d);
	}
	line("all", chunks_all, &all);
	printf("(windows: parsed windows per chunk; active: active lanes per window; d=k: fraction of the windows whose deepest active lane has k eager candidates;\n"
	       " st2: fraction whose second stage runs; n=k: fraction of ALL windows in which k of the four candidate indices need the second stage)\n");
	return 0;
}
