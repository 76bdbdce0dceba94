// lz_stage_study.c -- CPU model (dev tool): how often would a two-stage candidate compare in LZNT1's window parse (csrc/lznt1.hip lz_window) need
// its second stage? Stage 1 compares the first W bytes of a candidate with the position's (W = 8 or 12); stage 2 (bytes W..15 and the long tail)
// is wave-wide work, so it runs for a whole finishing step, or a whole window's eager scan, as soon as ONE existing candidate of ONE lane agrees
// on all W bytes while max_len > W. The model parses every 4 KiB chunk as the kernel does (12-bit hash, position-ordered buckets, LZ_SELF = 4 eager
// candidates per lane, max_len rule, greedy walk window by window, finishing steps of 64 candidates that stop at max_len) and prints per member
//   steps:   finishing steps per chunk, and the fraction of them in which a valid candidate reaches W bytes;
//   windows: parsed windows per chunk, and the fraction of them in which an eager candidate of an active lane reaches W bytes.
// The second stage costs 3 to 7 vector instructions where it runs and saves 9 per candidate where it does not: worth building below 0.6 (steps) and
// 0.8 (windows).
//   build: gcc -O2 -o lz_stage_study tools/dev/lz_stage_study.c      usage: lz_stage_study [file index 0..11 ...]   (default: all 12 corpus files)
#include "../../ms_compress_amd/csrc/corpus.c"
#include <stdio.h>
#include <stdlib.h>

#define SELF 4u
#define NW 2                                                  // stage widths studied
static const uint32_t width[NW] = { 8, 12 };
static uint32_t hash_of(const uint8_t* c) { const uint32_t k = c[0] | c[1] << 8 | c[2] << 16, h = (k * 0x9E3779B1u) >> 20; return h ? h : 1u; }
static uint32_t shift_of(uint32_t p) { return p <= 16 ? 12 : 12 - ((32 - __builtin_clz(p - 1)) - 4); }
static uint32_t lcp(const uint8_t* c, uint32_t q, uint32_t p, uint32_t lim) { uint32_t l = 0; while (l < lim && c[q + l] == c[p + l]) { ++l; } return l; }

typedef struct { double windows, steps, events, win_hit[NW], step_hit[NW], step_cands; } Cnt;

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
		// the eager scan of every active lane: key of the best of its first SELF candidates
		uint32_t key[64] = {0}, maxl[64] = {0};
		int hit[NW] = {0};
		for (uint32_t p = entry > wb ? entry : wb; p < we; ++p) {
			if (p == 0 || p + 3 > n) { continue; }
			const uint32_t i = p - wb, m3 = (1u << shift_of(p)) + 2, s = start[hash_of(c + p)];
			maxl[i] = n - p < m3 ? n - p : m3;
			for (uint32_t j = 0; j < SELF && j < rankof[p]; ++j) {
				const uint32_t q = bucket[s + j], l = lcp(c, q, p, maxl[i]), kk = (l << 12) | (q ^ 4095u);
				for (int w = 0; w < NW; ++w) { hit[w] |= l >= width[w] && maxl[i] > width[w]; }
				if (kk > key[i]) { key[i] = kk; }
			}
		}
		k->windows++;
		for (int w = 0; w < NW; ++w) { k->win_hit[w] += hit[w]; }
		// the greedy walk; a token start with a fifth candidate and max_len not reached is finished, 64 candidates per step
		uint32_t p = entry > wb ? entry : wb;
		while (p < we) {
			const uint32_t i = p - wb;
			uint32_t kb = key[i];
			if (maxl[i] && rankof[p] > SELF && (kb >> 12) < maxl[i]) {
				const uint32_t s = start[hash_of(c + p)];
				k->events++;
				for (uint32_t b = SELF; b < rankof[p]; b += 64) {
					int sh[NW] = {0};
					for (uint32_t j = b; j < b + 64 && j < rankof[p]; ++j) {
						const uint32_t q = bucket[s + j], l = lcp(c, q, p, maxl[i]), kk = (l << 12) | (q ^ 4095u);
						for (int w = 0; w < NW; ++w) { sh[w] |= l >= width[w] && maxl[i] > width[w]; }
						if (kk > kb) { kb = kk; }
						k->step_cands++;
					}
					k->steps++;
					for (int w = 0; w < NW; ++w) { k->step_hit[w] += sh[w]; }
					if ((kb >> 12) == maxl[i]) { break; }
				}
			}
			p += (kb >> 12) >= 3 ? (kb >> 12) : 1;
		}
		entry = p;
	}
}

static void line(const char* name, double ch, const Cnt* k)
{
	printf("%-8s %7.0f | %7.1f %7.1f %6.1f  %5.3f %5.3f | %7.1f  %5.3f %5.3f\n", name, ch, k->events / ch, k->steps / ch, k->steps ? k->step_cands / k->steps : 0.0,
	       k->steps ? k->step_hit[0] / k->steps : 0.0, k->steps ? k->step_hit[1] / k->steps : 0.0,
	       k->windows / ch, k->win_hit[0] / k->windows, k->win_hit[1] / k->windows);
}

int main(int argc, char** argv)
{
	int files[12], nf = 0;
	for (int a = 1; a < argc && nf < 12; ++a) { files[nf++] = atoi(argv[a]); }
	if (nf == 0) { for (int i = 0; i < 12; ++i) { files[nf++] = i; } }
	Cnt all = {0}; double chunks_all = 0;
	printf("%-8s %7s | %7s %7s %6s  %5s %5s | %7s  %5s %5s\n", "file", "chunks", "events", "steps", "cands", ">=8", ">=12", "windows", ">=8", ">=12");
	for (int f = 0; f < nf; ++f) {
		const uint64_t N = mscorpus_file_size(files[f]);
		uint8_t* d = malloc(N); mscorpus_generate(files[f], d, N);
		Cnt k = {0}; double ch = 0;
		for (uint64_t o = 0; o < N; o += 4096) { chunk(d + o, (uint32_t)(N - o < 4096 ? N - o : 4096), &k); ch++; }
		line(mscorpus_file_name(files[f]), ch, &k);
		all.windows += k.windows; all.steps += k.steps; all.events += k.events; all.step_cands += k.step_cands;
		for (int w = 0; w < NW; ++w) { all.win_hit[w] += k.win_hit[w]; all.step_hit[w] += k.step_hit[w]; }
		chunks_all += ch;
		free(d);
	}
	line("all", chunks_all, &all);
	printf("(events, steps, windows: per chunk; cands: valid candidates per finishing step; >=W: fraction of the steps / windows whose second stage runs)\n");
	return 0;
}
