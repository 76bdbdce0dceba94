// lz_tail_study.c -- CPU model (dev tool) of the long-match work of LZNT1's window parse (csrc/lznt1.hip lz_window): the same 12-bit hash,
// position-ordered buckets, LZ_SELF = 4 candidates per lane, max_len rule and greedy walk, window by window as the one-wave kernel walks a chunk.
// Counts per 4 KiB chunk, for the parent's form (every lane extends every 16-byte candidate with lz_lcp_tail, 16 bytes per iteration) and for
// the on-demand form (16-byte compares only; the walk stops on a long-pending position and the wave extends its candidates, 256 bytes per step).
// The parse itself, and so the finishing steps, are the same in both forms.
//   build: gcc -O2 -o lz_tail_study tools/dev/lz_tail_study.c      usage: lz_tail_study [file index 0..11 ...]   (default: all 12 corpus files)
#include "../../ms_compress_amd/csrc/corpus.c"
#include <stdio.h>
#include <stdlib.h>

#define SELF 4u
static uint32_t hash_of(const uint8_t* c) { const uint32_t k = c[0] | c[1] << 8 | c[2] << 16, h = (k * 0x9E3779B1u) >> 20; return h ? h : 1u; }
static uint32_t shift_of(uint32_t p) { return p <= 16 ? 12 : 12 - ((32 - __builtin_clz(p - 1)) - 4); }
static uint32_t lcp(const uint8_t* c, uint32_t q, uint32_t p, uint32_t lim) { uint32_t l = 0; while (l < lim && c[q + l] == c[p + l]) { ++l; } return l; }
// lz_lcp_tail: iterations of 16 bytes from byte 16 on (the last may run past max_len; the kernel clamps afterwards)
static uint32_t tail_iters(const uint8_t* c, uint32_t q, uint32_t p, uint32_t maxlen, uint32_t* len)
{
	uint32_t l = 16, it = 0;
	for (;;) { ++it; const uint32_t f = lcp(c, q + l, p + l, 16); l += f; if (f < 16 || l >= maxlen) { break; } }
	*len = l < maxlen ? l : maxlen; return it;
}
// lz_lcp_wave: steps of 256 bytes from byte 16 on
static uint32_t wave_steps(const uint8_t* c, uint32_t q, uint32_t p, uint32_t maxlen, uint32_t* len)
{
	uint32_t l = 16, st = 0;
	for (;;) { ++st; const uint32_t f = lcp(c, q + l, p + l, 256); if (f < 256) { l += f; break; } l += 256; if (l >= maxlen) { break; } }
	*len = l < maxlen ? l : maxlen; return st;
}

typedef struct { double ev, steps, coll_ev, eager_it, fin_it, lp_stops, coop; } Cnt;

static void chunk(const uint8_t* src, uint32_t n, Cnt* k)
{
	static uint8_t c[4096 + 4096 + 64];                      // zeros behind the chunk, as in LDS
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
		uint32_t keyf[64] = {0}, maxl[64] = {0}, nc[64] = {0}, l16[64] = {0};   // full key (both forms' parse), max_len, candidates, 16-byte mask
		uint32_t eag[SELF] = {0};
		for (uint32_t p = (entry > wb ? entry : wb); p < we; ++p) {
			const uint32_t i = p - wb;
			if (p == 0 || p + 3 > n) { continue; }
			const uint32_t m3 = (1u << shift_of(p)) + 2; maxl[i] = n - p < m3 ? n - p : m3;
			const uint32_t h = hash_of(c + p), s = start[h]; nc[i] = rankof[p];
			for (uint32_t j = 0; j < SELF && j < nc[i]; ++j) {
				const uint32_t q = bucket[s + j], cap = maxl[i] < 16 ? maxl[i] : 16;
				uint32_t l = lcp(c, q, p, cap);
				if (l == 16 && maxl[i] > 16) { l16[i] |= 1u << j; const uint32_t it = tail_iters(c, q, p, maxl[i], &l); if (it > eag[j]) { eag[j] = it; } }
				const uint32_t kk = (l << 12) | (q ^ 4095u);
				if (kk > keyf[i]) { keyf[i] = kk; }
			}
		}
		for (uint32_t j = 0; j < SELF; ++j) { k->eager_it += eag[j]; }
		// the greedy walk (the kernel jumps over literal runs and taken matches; it lands on exactly the token starts)
		uint32_t p = entry > wb ? entry : wb;
		while (p < we) {
			const uint32_t i = p - wb;
			uint32_t key = keyf[i];
			if (l16[i]) {                                          // long-pending: the on-demand form extends here, oldest first
				k->lp_stops++;
				const uint32_t s = start[hash_of(c + p)];
				for (uint32_t j = 0; j < SELF; ++j) {
					if (!(l16[i] >> j & 1u)) { continue; }
					uint32_t l; k->coop += wave_steps(c, bucket[s + j], p, maxl[i], &l);
					if (l == maxl[i]) { break; }
				}
			}
			if (nc[i] > SELF && (key >> 12) < maxl[i]) {           // unresolved: finishing steps of 64 candidates
				const uint32_t s = start[hash_of(c + p)];
				uint32_t same = 0;
				for (uint32_t j = 0; j < nc[i]; ++j) { const uint8_t* a = c + bucket[s + j]; same += a[0] == c[p] && a[1] == c[p + 1] && a[2] == c[p + 2]; }
				k->ev++; k->coll_ev += same <= SELF;
				for (uint32_t b = SELF; b < nc[i]; b += 64) {
					uint32_t it_max = 0;
					for (uint32_t j = b; j < b + 64 && j < nc[i]; ++j) {
						const uint32_t q = bucket[s + j], cap = maxl[i] < 16 ? maxl[i] : 16;
						uint32_t l = lcp(c, q, p, cap);
						if (l == 16 && maxl[i] > 16) { const uint32_t it = tail_iters(c, q, p, maxl[i], &l); if (it > it_max) { it_max = it; } }
						const uint32_t kk = (l << 12) | (q ^ 4095u);
						if (kk > key) { key = kk; }
					}
					k->steps++; k->fin_it += it_max;
					if ((key >> 12) == maxl[i] || b + 64 >= nc[i]) { break; }
				}
			}
			p += (key >> 12) >= 3 ? (key >> 12) : 1;
		}
		entry = p;
	}
}

int main(int argc, char** argv)
{
	int files[12], nf = 0;
	for (int a = 1; a < argc && nf < 12; ++a) { files[nf++] = atoi(argv[a]); }
	if (nf == 0) { for (int i = 0; i < 12; ++i) { files[nf++] = i; } }
	Cnt all = {0}; double chunks_all = 0;
	printf("%-8s %7s | %7s %7s | %7s | %9s %7s | %8s %7s\n", "file", "chunks", "events", "steps", "coll.ev", "eager.it", "fin.it", "lp.stops", "coop");
	for (int f = 0; f < nf; ++f) {
		const uint64_t N = mscorpus_file_size(files[f]);
		uint8_t* d = malloc(N); mscorpus_generate(files[f], d, N);
		Cnt k = {0}; double ch = 0;
		for (uint64_t o = 0; o < N; o += 4096) { chunk(d + o, (uint32_t)(N - o < 4096 ? N - o : 4096), &k); ch++; }
		printf("%-8s %7.0f | %7.1f %7.1f | %7.1f | %9.1f %7.1f | %8.1f %7.1f\n", mscorpus_file_name(files[f]), ch, k.ev / ch, k.steps / ch, k.coll_ev / ch,
		       k.eager_it / ch, k.fin_it / ch, k.lp_stops / ch, k.coop / ch);
		all.ev += k.ev; all.steps += k.steps; all.coll_ev += k.coll_ev; all.eager_it += k.eager_it; all.fin_it += k.fin_it; all.lp_stops += k.lp_stops;
		all.coop += k.coop; chunks_all += ch;
		free(d);
	}
	const double ch = chunks_all;
	printf("%-8s %7.0f | %7.1f %7.1f | %7.1f | %9.1f %7.1f | %8.1f %7.1f\n", "all", ch, all.ev / ch, all.steps / ch, all.coll_ev / ch, all.eager_it / ch,
	       all.fin_it / ch, all.lp_stops / ch, all.coop / ch);
	printf("per chunk, parent's form: eager lz_lcp_tail wave-iterations %.1f + finishing %.1f; on-demand form: finishing %.1f + %.1f long-pending stops "
	       "with %.1f cooperative 256-byte steps\n", all.eager_it / ch, all.fin_it / ch, all.fin_it / ch, all.lp_stops / ch, all.coop / ch);
	return 0;
}
