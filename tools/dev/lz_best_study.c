// lz_best_study.c -- CPU model (dev tool): how often does a finishing step of LZNT1's window parse (csrc/lznt1.hip lz_window) change the best
// match of its position? A step reduces the keys (len << 12 | 4095 - q) of up to 64 candidates to their maximum and takes it if it is above the
// best so far. Its candidates are younger than the best's and the older one wins on equal length, so the reduction can return something new only
// if a candidate is STRICTLY longer than the best and at least 3 bytes long (a best below 3 bytes is "no match" to everything downstream). The
// model parses every 4 KiB chunk as the kernel does (lz_stage_study.c's parse: 12-bit hash, position-ordered buckets, LZ_SELF = 4 eager candidates,
// max_len rule, greedy walk window by window, finishing steps of 64 candidates that stop at max_len), computes every step BOTH ways -- the
// maximum of the keys, and the threshold rule: the winners are the candidates of at least max(len(best) + 1, 3) bytes, the oldest of the longest
// of them is the new best -- and stops if the two ever disagree on the match (start and length, for 3 bytes and more) or on "max_len reached".
// It prints per member
//   steps:  finishing events and steps per chunk, and the fractions of the steps with no winner, exactly one, several;
//   events: the fraction of the finishing events that leave the best as they found it (no write-back of the key needed).
// A step without a winner needs neither the key build nor the DPP maximum (about 10 of its 24 vector instructions), a step with one winner can
// read the winner's lane (about 8).
//   build: gcc -O2 -o lz_best_study tools/dev/lz_best_study.c      usage: lz_best_study [file index 0..11 ...]   (default: all 12 corpus files)
#include "../../ms_compress_amd/csrc/corpus.c"
#include <stdio.h>
#include <stdlib.h>

#define SELF 4u
static uint32_t hash_of(const uint8_t* c) { const uint32_t k = c[0] | c[1] << 8 | c[2] << 16, h = (k * 0x9E3779B1u) >> 20; return h ? h : 1u; }
static uint32_t shift_of(uint32_t p) { return p <= 16 ? 12 : 12 - ((32 - __builtin_clz(p - 1)) - 4); }
static uint32_t lcp(const uint8_t* c, uint32_t q, uint32_t p, uint32_t lim) { uint32_t l = 0; while (l < lim && c[q + l] == c[p + l]) { ++l; } return l; }
static uint32_t match_of(uint32_t key) { return key >= (3u << 12) ? key : 0u; }     // below 3 bytes: no match, whichever key

typedef struct { double events, steps, none, one, several, unchanged; } Cnt;

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
		for (uint32_t p = entry > wb ? entry : wb; p < we; ++p) {
			if (p == 0 || p + 3 > n) { continue; }
			const uint32_t i = p - wb, m3 = (1u << shift_of(p)) + 2, s = start[hash_of(c + p)];
			maxl[i] = n - p < m3 ? n - p : m3;
			for (uint32_t j = 0; j < SELF && j < rankof[p]; ++j) {
				const uint32_t q = bucket[s + j], l = lcp(c, q, p, maxl[i]), kk = (l << 12) | (q ^ 4095u);
				if (kk > key[i]) { key[i] = kk; }
			}
		}
		// the greedy walk; a token start with a fifth candidate and max_len not reached is finished, 64 candidates per step
		uint32_t p = entry > wb ? entry : wb;
		while (p < we) {
			const uint32_t i = p - wb;
			uint32_t kb = key[i];                              // the best by the maximum of the keys
			uint32_t kt = key[i];                              // the best by the threshold rule
			if (maxl[i] && rankof[p] > SELF && (kb >> 12) < maxl[i]) {
				const uint32_t s = start[hash_of(c + p)];
				k->events++;
				for (uint32_t b = SELF; b < rankof[p]; b += 64) {
					const uint32_t need = (kt >> 12) + 1 > 3 ? (kt >> 12) + 1 : 3;
					uint32_t winners = 0, wbest = 0;
					for (uint32_t j = b; j < b + 64 && j < rankof[p]; ++j) {
						const uint32_t q = bucket[s + j], l = lcp(c, q, p, maxl[i]), kk = (l << 12) | (q ^ 4095u);
						if (kk > kb) { kb = kk; }
						if (l >= need) { winners++; if (kk > wbest) { wbest = kk; } }
					}
					if (winners) { kt = wbest; }
					k->steps++;
					k->none += winners == 0; k->one += winners == 1; k->several += winners > 1;
					if (match_of(kb) != match_of(kt) || ((kb >> 12) == maxl[i]) != ((kt >> 12) == maxl[i])) {
						fprintf(stderr, "the two rules disagree: position %u, step at %u: %08x against %08x\n", p, b, kb, kt); exit(1);
					}
					if ((kt >> 12) == maxl[i]) { break; }
				}
				k->unchanged += kt == key[i];
			}
			p += (kt >> 12) >= 3 ? (kt >> 12) : 1;
		}
		entry = p;
	}
}

static void line(const char* name, double ch, const Cnt* k)
{
	printf("%-8s %7.0f | %7.1f %7.1f  %5.3f %5.3f %5.3f | %5.3f\n", name, ch, k->events / ch, k->steps / ch,
	       k->steps ? k->none / k->steps : 0.0, k->steps ? k->one / k->steps : 0.0, k->steps ? k->several / k->steps : 0.0,
	       k->events ? k->unchanged / k->events : 0.0);
}

int main(int argc, char** argv)
{
	int files[12], nf = 0;
	for (int a = 1; a < argc && nf < 12; ++a) { files[nf++] = atoi(argv[a]); }
	if (nf == 0) { for (int i = 0; i < 12; ++i) { files[nf++] = i; } }
	Cnt all = {0}; double chunks_all = 0;
	printf("%-8s %7s | %7s %7s  %5s %5s %5s | %5s\n", "file", "chunks", "events", "steps", "none", "one", "more", "same");
	for (int f = 0; f < nf; ++f) {
		const uint64_t N = mscorpus_file_size(files[f]);
		uint8_t* d = malloc(N); mscorpus_generate(files[f], d, N);
		Cnt k = {0}; double ch = 0;
		for (uint64_t o = 0; o < N; o += 4096) { chunk(d + o, (uint32_t)(N - o < 4096 ? N - o : 4096), &k); ch++; }
		line(mscorpus_file_name(files[f]), ch, &k);
		all.events += k.events; all.steps += k.steps; all.none += k.none; all.one += k.one; all.several += k.several; all.unchanged += k.unchanged;
		chunks_all += ch;
		free(d);
	}
	line("all", chunks_all, &all);
	printf("(events, steps: per chunk; none / one / more: fraction of the finishing steps in which no candidate, exactly one, several are strictly longer than\n"
	       " the best so far and at least 3 bytes long; same: fraction of the finishing events that leave the best as they found it.\n"
	       " Every step was computed as the maximum of the keys and by the threshold rule: they agreed throughout.)\n");
	return 0;
}
