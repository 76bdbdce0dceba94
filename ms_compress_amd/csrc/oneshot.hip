// oneshot.hip -- the drop-in one-shot entry points (host pointers): H2D, one-unit batch on the GPU, D2H, with three kinds of pipelining for
// large buffers. No CPU encoder exists here. Host code only.
//
// Reference boundary mirrored here: ms_compress / ms_decompress (the reference's src/mscomp.cpp:103-133), lznt1_compress
// (src/lznt1_compress.cpp:233), xpress_compress (src/xpress_compress.cpp:240), xpress_huff_compress (src/xpress_huff_compress.cpp:247).
#include "host.h"
#include <mutex>
#include <thread>
#include <condition_variable>

using namespace msc;

extern "C" {   // (C linkage reaches into the namespace: one_shot_tls below is a dynamic symbol of the library)
namespace {

// One context per calling host thread (the reference is reentrant: SURVEY.md 8b "Threading"), destroyed with its thread. The
// plans of recent calls are kept: a caller that compresses buffers of one size (pages, records, fixed blocks) pays the table
// upload once and gets the captured hipGraph from its second call on.
struct OneShotTls {
	mscomp_amd_ctx* ctx = nullptr;
	hipStream_t exec = nullptr, h2d = nullptr, d2h = nullptr;   // non-blocking streams: kernels, uploads, downloads
	std::vector<hipEvent_t> ev;                         // two per slice of a pipelined call
	uint64_t* h_len = nullptr; int32_t* h_st = nullptr; size_t h_cap = 0;   // pinned: per-slice results
	DevBuf d_meta;
	struct Entry { MSCompFormat format; bool decompress; uint64_t in_len, out_cap; mscomp_amd_plan* plan; uint64_t used; };
	std::vector<Entry> plans;
	uint64_t tick = 0;
	void drop()
	{
		for (auto& e : plans) { mscomp_amd_plan_destroy(e.plan); }
		plans.clear();
		if (ctx) { mscomp_amd_ctx_destroy(ctx); ctx = nullptr; }
		for (auto e : ev) { (void)hipEventDestroy(e); }
		ev.clear();
		if (h_len) { (void)hipHostFree(h_len); h_len = nullptr; h_st = nullptr; h_cap = 0; }
		d_meta.release();
		if (exec) { (void)hipStreamDestroy(exec); exec = nullptr; }
		if (h2d) { (void)hipStreamDestroy(h2d); h2d = nullptr; }
		if (d2h) { (void)hipStreamDestroy(d2h); d2h = nullptr; }
	}
	bool slices(size_t n)                               // events, pinned result slots and device result slots for n slices
	{
		while (ev.size() < 2 * n) { hipEvent_t e = nullptr; if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) { return false; } ev.push_back(e); }
		if (h_cap < n) {
			if (h_len) { (void)hipHostFree(h_len); h_len = nullptr; h_cap = 0; }
			void* q = nullptr;
			if (hipHostMalloc(&q, n * 16, hipHostMallocDefault) != hipSuccess) { return false; }
			h_len = static_cast<uint64_t*>(q); h_st = reinterpret_cast<int32_t*>(h_len + n); h_cap = n;
		}
		return d_meta.reserve(n * 16);
	}
	~OneShotTls() { drop(); }
	MSCompStatus plan_for(MSCompFormat f, bool dec, uint64_t in_len, uint64_t out_cap, mscomp_amd_plan** out)
	{
		for (auto& e : plans) {
			if (e.format == f && e.decompress == dec && e.in_len == in_len && e.out_cap == out_cap && e.plan->lznt1_sa == (!dec && f == MSCOMP_LZNT1 && lznt1_sa_for(ctx))) { e.used = ++tick; *out = e.plan; return MSCOMP_OK; }
		}
		const uint64_t z = 0;
		mscomp_amd_plan* p = nullptr;
		const MSCompStatus s = plan_create_impl(ctx, f, dec, 1, &z, &in_len, &z, &out_cap, &p);
		if (s != MSCOMP_OK) { return s; }
		p->run.never = true;
		if (plans.size() >= 8) {
			size_t lru = 0;
			for (size_t i = 1; i < plans.size(); ++i) { if (plans[i].used < plans[lru].used) { lru = i; } }
			mscomp_amd_plan_destroy(plans[lru].plan);
			plans.erase(plans.begin() + (long)lru);
		}
		plans.push_back(Entry{ f, dec, in_len, out_cap, p, ++tick });
		*out = p;
		return MSCOMP_OK;
	}
};

OneShotTls& one_shot_tls() { thread_local OneShotTls tls; return tls; }

} // namespace
} // extern "C"
mscomp_amd_ctx* msc::one_shot_ctx() { return one_shot_tls().ctx; }

// Page-locking of caller buffers for the large host-pointer calls. hipHostRegister refuses a range that overlaps a registered one, and a range
// one thread unregisters while another thread's copy of the same pages is in flight would pull the pages from under that copy (two threads may
// legally compress the SAME input at once: the reference only forbids aliasing in / out). So registrations go through this table: the same range
// is shared (counted), an overlapping but different range waits until the other call has released its own, and a range that cannot be registered
// at all (locked-memory limits) is simply not pinned -- the copies then go through the runtime's staging buffers.
struct HostPins {
	struct Ent { const uint8_t* b; size_t n; int refs; std::vector<std::thread::id> owners; };
	std::mutex mu; std::condition_variable cv; std::vector<Ent> ents;
	bool pin(const void* ptr, size_t n)                       // true: the range is page-locked (and mapped) until unpin
	{
		if (!ptr || !n) { return false; }
		const uint8_t* b = static_cast<const uint8_t*>(ptr);
		const std::thread::id me = std::this_thread::get_id();
		std::unique_lock<std::mutex> lk(mu);
		for (;;) {
			bool overlap = false;
			for (auto& e : ents) {
				if (e.b == b && e.n == n) { ++e.refs; e.owners.push_back(me); return true; }
				if (b < e.b + e.n && e.b < b + n) {
					// a different range that overlaps one THIS thread holds (a call whose in and out overlap): waiting would wait for ourselves --
					// the range is simply not pinned and its copies go through the runtime's staging buffers
					for (auto& o : e.owners) { if (o == me) { return false; } }
					overlap = true;
				}
			}
			if (!overlap) { break; }
			cv.wait(lk);
		}
		// (hipHostRegister of tens of megabytes takes milliseconds and runs under the table's lock: large one-shot calls of different threads
		// register one after the other; their copies and kernels still overlap)
		if (hipHostRegister(const_cast<uint8_t*>(b), n, hipHostRegisterMapped | hipHostRegisterPortable) != hipSuccess) { (void)hipGetLastError(); return false; }
		ents.push_back(Ent{ b, n, 1, { me } });
		return true;
	}
	// A call that does NOT pin its input (the staged paths) but reads a range another thread's call has registered: the runtime then copies
	// from it as from pinned memory (asynchronously), so the registration must outlive that copy. hold() takes a reference on every entry that
	// overlaps the range (the entries are returned and given back with release() once the copy is done).
	std::vector<std::pair<const uint8_t*, size_t>> hold(const void* ptr, size_t n)
	{
		std::vector<std::pair<const uint8_t*, size_t>> held;
		if (!ptr || !n) { return held; }
		const uint8_t* b = static_cast<const uint8_t*>(ptr);
		std::unique_lock<std::mutex> lk(mu);
		for (auto& e : ents) { if (b < e.b + e.n && e.b < b + n) { ++e.refs; held.push_back({ e.b, e.n }); } }
		return held;
	}
	void release(const std::vector<std::pair<const uint8_t*, size_t>>& held)
	{
		std::unique_lock<std::mutex> lk(mu);
		for (auto& h : held) {
			for (size_t i = 0; i < ents.size(); ++i) {
				if (ents[i].b == h.first && ents[i].n == h.second) {
					if (--ents[i].refs == 0) { (void)hipHostUnregister(const_cast<uint8_t*>(ents[i].b)); ents.erase(ents.begin() + (long)i); cv.notify_all(); }
					break;
				}
			}
		}
	}
	void unpin(const void* ptr, size_t n)
	{
		const uint8_t* b = static_cast<const uint8_t*>(ptr);
		const std::thread::id me = std::this_thread::get_id();
		std::unique_lock<std::mutex> lk(mu);
		for (size_t i = 0; i < ents.size(); ++i) {
			if (ents[i].b == b && ents[i].n == n) {
				for (size_t k = 0; k < ents[i].owners.size(); ++k) { if (ents[i].owners[k] == me) { ents[i].owners.erase(ents[i].owners.begin() + (long)k); break; } }
				if (--ents[i].refs == 0) { (void)hipHostUnregister(const_cast<uint8_t*>(b)); ents.erase(ents.begin() + (long)i); cv.notify_all(); }
				return;
			}
		}
	}
};
static HostPins g_pins;
void* msc::host_pins_hold(const void* ptr, size_t n)
{
	auto v = g_pins.hold(ptr, n);
	if (v.empty()) { return nullptr; }
	return new (std::nothrow) std::vector<std::pair<const uint8_t*, size_t>>(std::move(v));
}
void msc::host_pins_release(void* token)
{
	if (!token) { return; }
	auto* v = static_cast<std::vector<std::pair<const uint8_t*, size_t>>*>(token);
	g_pins.release(*v);
	delete v;
}

// one large host buffer through the GPU with the link busy in both directions while the kernels run. LZNT1 chunks
// are independent and the output is their concatenation (lznt1_compress.cpp:262), so the buffer is cut into slices of 1024 chunks:
// slice k + 1 is on its way up (stream h2d) and slice k - 1 on its way down (stream d2h) while slice k is compressed (the
// context's stream); a slice's place in the caller's output is known once the sizes of the slices before it are back (16 bytes per
// slice into pinned memory). The caller's buffers are page-locked for the duration of the call when the runtime allows it
// (hipHostRegister: uploads and downloads then really overlap; measured on the MI355X box: 85 MB both ways at once 0.92 ms pinned,
// 1.7 ms pageable); without it the copies still work.
// Slices of about 24 MiB (6 144 chunks: three rounds of the chunk kernel's 2 048 resident blocks; with 4 MiB slices the kernels ran at a
// third of their batch rate and the call took 4.9 instead of 2.7 ms), equal in size, at least two (MSCOMP_AMD_ONE_SLICE_MB: hooks.hip env_one_slice).
static MSCompStatus lznt1_compress_pipelined(OneShotTls& tls, const uint8_t* in, size_t in_len, uint8_t* out, size_t* out_len)
{
	mscomp_amd_ctx* c = tls.ctx;
	const size_t cap = *out_len, ONE_SLICE = env_one_slice();
	const size_t ns = (in_len + ONE_SLICE / 2) / ONE_SLICE < 2 ? 2 : (in_len + ONE_SLICE / 2) / ONE_SLICE;
	const size_t SL = ((in_len + ns - 1) / ns + 4095) & ~(size_t)4095;          // bytes per slice: whole chunks
	const size_t scap = (lznt1_max_compressed_size(SL) + 2 + 15) & ~(size_t)15;
	if (!tls.slices(ns) || !c->one_in.reserve(in_len + 64) || !c->one_out.reserve(ns * scap + 64)) { return MSCOMP_MEM_ERROR; }
	uint8_t* d_in = static_cast<uint8_t*>(c->one_in.p); uint8_t* d_out = static_cast<uint8_t*>(c->one_out.p);
	uint64_t* d_len = static_cast<uint64_t*>(tls.d_meta.p); int32_t* d_st = reinterpret_cast<int32_t*>(d_len + ns);
	const size_t most = lznt1_max_compressed_size(in_len) + 2, out_span = cap < most ? cap : most;
	const bool reg_in = g_pins.pin(in, in_len);
	const bool reg_out = out_span && g_pins.pin(out, out_span);
	MSCompStatus rs = MSCOMP_OK;
	for (size_t k = 0; k < ns && rs == MSCOMP_OK; ++k) {
		const size_t o = k * SL, len = in_len - o < SL ? in_len - o : SL;
		if (hipMemcpyAsync(d_in + o, in + o, len, hipMemcpyHostToDevice, tls.h2d) != hipSuccess || hipEventRecord(tls.ev[2 * k], tls.h2d) != hipSuccess) { rs = MSCOMP_ERRNO; }
	}
	for (size_t k = 0; k < ns && rs == MSCOMP_OK; ++k) {
		const size_t o = k * SL, len = in_len - o < SL ? in_len - o : SL;
		mscomp_amd_plan* p = nullptr;
		rs = tls.plan_for(MSCOMP_LZNT1, false, len, scap, &p);
		if (rs != MSCOMP_OK) { break; }
		if (hipStreamWaitEvent(tls.exec, tls.ev[2 * k], 0) != hipSuccess) { rs = MSCOMP_ERRNO; break; }
		rs = mscomp_amd_plan_execute(p, d_in + o, d_out + k * scap, d_len + k, d_st + k);
		if (rs != MSCOMP_OK) { break; }
		if (hipMemcpyAsync(tls.h_len + k, d_len + k, 8, hipMemcpyDeviceToHost, tls.exec) != hipSuccess ||
		    hipMemcpyAsync(tls.h_st + k, d_st + k, 4, hipMemcpyDeviceToHost, tls.exec) != hipSuccess ||
		    hipEventRecord(tls.ev[2 * k + 1], tls.exec) != hipSuccess) { rs = MSCOMP_ERRNO; }
	}
	size_t total = 0;
	bool fits = true;
	for (size_t k = 0; k < ns && rs == MSCOMP_OK; ++k) {
		if (hipEventSynchronize(tls.ev[2 * k + 1]) != hipSuccess) { rs = MSCOMP_ERRNO; break; }
		if (tls.h_st[k] != MSCOMP_OK) { rs = (MSCompStatus)tls.h_st[k]; break; }
		const size_t len = (size_t)tls.h_len[k];
		if (fits && total + len <= cap) {
			if (len && hipMemcpyAsync(out + total, d_out + k * scap, len, hipMemcpyDeviceToHost, tls.d2h) != hipSuccess) { rs = MSCOMP_ERRNO; }
		} else { fits = false; }                                    // MSCOMP_BUF_ERROR (lznt1_compress.cpp:251,267): nothing behind the capacity is written
		total += len;
	}
	(void)hipStreamSynchronize(tls.h2d); (void)hipStreamSynchronize(tls.exec);
	if (hipStreamSynchronize(tls.d2h) != hipSuccess && rs == MSCOMP_OK) { rs = MSCOMP_ERRNO; }
	if (reg_in) { g_pins.unpin(in, in_len); }
	if (reg_out) { g_pins.unpin(out, out_span); }
	if (rs != MSCOMP_OK) { return rs; }
	if (!fits) { return MSCOMP_BUF_ERROR; }
	if (cap - total >= 2) { out[total] = 0; out[total + 1] = 0; }   // the uncounted End_of_buffer bytes (lznt1_compress.cpp:270)
	*out_len = total;
	return MSCOMP_OK;
}

// The same call without staging copies (51 MB: 2.28 -> 2.08 ms; MSCOMP_AMD_ONE_ZEROCOPY=0 switches it off): the caller's buffers are page-locked AND mapped, the chunk kernel
// reads its 4 KiB chunks straight from host memory over PCIe (every input byte once, 16 bytes per lane) and the placement kernel writes the
// images straight into the caller's output. One launch for the whole buffer: no slices, no copies in HBM. -100 = could not map (the caller falls
// back to the sliced path).
// (decompress = true works too, but is slower than the staged path for 51 MB: 2.26 instead of 2.01 ms -- the decoder reads its input twice and
// writes its output in 64-byte rows; not used)
static MSCompStatus lznt1_zero_copy(OneShotTls& tls, bool decompress, const uint8_t* in, size_t in_len, uint8_t* out, size_t* out_len)
{
	mscomp_amd_ctx* c = tls.ctx;
	const size_t cap = *out_len;
	const size_t most = decompress ? (in_len / 3 + 1) * 4096 : lznt1_max_compressed_size(in_len) + 2, out_span = cap < most ? cap : most;   // (what the format can produce: see one_shot)
	if (!out_span || !c->one_meta.reserve(64)) { return (MSCompStatus)-100; }
	if (!g_pins.pin(in, in_len)) { return (MSCompStatus)-100; }
	if (!g_pins.pin(out, out_span)) { g_pins.unpin(in, in_len); return (MSCompStatus)-100; }
	void* din = nullptr; void* dout = nullptr;
	MSCompStatus rs = MSCOMP_OK;
	struct { uint64_t len; int32_t st; int32_t pad; } meta = { 0, MSCOMP_ERRNO, 0 };
	if (hipHostGetDevicePointer(&din, const_cast<uint8_t*>(in), 0) != hipSuccess || hipHostGetDevicePointer(&dout, out, 0) != hipSuccess) { (void)hipGetLastError(); rs = (MSCompStatus)-100; }
	if (rs == MSCOMP_OK) {
		uint64_t* d_len = static_cast<uint64_t*>(c->one_meta.p); int32_t* d_st = reinterpret_cast<int32_t*>(d_len + 1);
		mscomp_amd_plan* p = nullptr;
		rs = tls.plan_for(MSCOMP_LZNT1, decompress, in_len, out_span, &p);
		if (rs == MSCOMP_OK) { rs = mscomp_amd_plan_execute(p, static_cast<const uint8_t*>(din), static_cast<uint8_t*>(dout), d_len, d_st); }
		if (rs == MSCOMP_OK && (hipMemcpyAsync(&meta, d_len, sizeof meta, hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess)) { rs = MSCOMP_ERRNO; }
	}
	g_pins.unpin(in, in_len); g_pins.unpin(out, out_span);
	if (rs != MSCOMP_OK) { return rs; }
	if (meta.st != MSCOMP_OK) { return (MSCompStatus)meta.st; }
	*out_len = (size_t)meta.len;
	return MSCOMP_OK;
}

static MSCompStatus one_shot(MSCompFormat format, bool decompress, const uint8_t* in, size_t in_len, uint8_t* out, size_t* out_len)
{
	if (!out_len || (in_len && !in) || (*out_len && !out)) { return MSCOMP_ARG_ERROR; }
	OneShotTls& tls = one_shot_tls();
	int dev = 0;
	if (hipGetDevice(&dev) != hipSuccess) { return MSCOMP_ERRNO; }   // no GPU / no HIP runtime: fail loudly, never fall back
	if (tls.ctx && tls.ctx->device != dev) { tls.drop(); }
	if (!tls.ctx) {
		if (hipStreamCreateWithFlags(&tls.exec, hipStreamNonBlocking) != hipSuccess || hipStreamCreateWithFlags(&tls.h2d, hipStreamNonBlocking) != hipSuccess ||
		    hipStreamCreateWithFlags(&tls.d2h, hipStreamNonBlocking) != hipSuccess) { tls.drop(); return MSCOMP_ERRNO; }
		MSCompStatus s = mscomp_amd_ctx_create(dev, tls.exec, &tls.ctx); if (s != MSCOMP_OK) { tls.drop(); return s; }
	}
	mscomp_amd_ctx* c = tls.ctx;
	DeviceGuard g(c->device);
	const size_t cap = *out_len;
	const bool zero_copy = g_sw.one_zero_copy.load(std::memory_order_relaxed) != 0;
	if (!decompress && format == MSCOMP_LZNT1 && in_len >= env_one_slice() + env_one_slice() / 2) {
		// (MSCOMP_AMD_ONE_ZEROCOPY=0 / mscomp_amd_debug_set_one_shot(1): always the sliced path below)
		if (zero_copy) { const MSCompStatus z = lznt1_zero_copy(tls, false, in, in_len, out, out_len); if ((int)z != -100) { return z; } }
		return lznt1_compress_pipelined(tls, in, in_len, out, out_len);
	}
	// The device copy of the output is sized by what the format can PRODUCE, never by a generous caller capacity (legal in the
	// reference: *out_len = 1 << 40 must not become a hipMalloc of a terabyte). Compression: at most ms_max_compressed_size (+ the
	// two uncounted LZNT1 End_of_buffer bytes), and a unit that fits that bound gets the status and bytes it would get with any larger
	// capacity. LZNT1 decompression: a chunk takes at least 3 bytes and gives at most 4096. Xpress / Xpress+Huffman decompression
	// has no such bound (a 10-byte match token can stand for 4 GiB), so the device capacity starts at 16 x the input and grows only
	// when the decoder says MSCOMP_BUF_ERROR: OK and DATA_ERROR are final at any capacity, because everything the decoders of
	// xpress_decompress.cpp:405-462 / xpress_huff_decompress.cpp:39-162 test before the output runs full is independent of where it ends.
	size_t dev_cap = cap;
	if (!decompress) {
		size_t most = format == MSCOMP_LZNT1 ? lznt1_max_compressed_size(in_len) + 2 : format == MSCOMP_XPRESS ? xpress_max_compressed_size(in_len) : xpress_huff_max_compressed_size(in_len);
		if (most < dev_cap) { dev_cap = most; }
	} else if (format == MSCOMP_LZNT1) {
		const size_t most = (in_len / 3 + 1) * 4096; if (most < dev_cap) { dev_cap = most; }
	} else {
		const size_t first = in_len * 16 + (1u << 20); if (first < dev_cap) { dev_cap = first; }
	}
	if (!c->one_in.reserve(in_len + 64) || !c->one_meta.reserve(64)) { return MSCOMP_MEM_ERROR; }
	uint8_t* d_in = static_cast<uint8_t*>(c->one_in.p);
	uint64_t* d_len = static_cast<uint64_t*>(c->one_meta.p); int32_t* d_st = reinterpret_cast<int32_t*>(d_len + 1);
	// (another thread's large LZNT1 call may have page-locked this very input: keep its registration alive until our copy is through)
	struct Held { std::vector<std::pair<const uint8_t*, size_t>> v; ~Held() { if (!v.empty()) { g_pins.release(v); } } } held{ g_pins.hold(in, in_len) };
	// Xpress / Xpress+Huffman compression of ONE large buffer (round 6): the buffer goes up in ranges of ONE_RANGE_CHUNKS chunks
	// on the upload stream and the match finding of a range -- chain links and Find, the two kernels that can run on part of a unit: a chunk's links
	// and matches depend on the chunks in front of it only -- starts as soon as the range (and the 64 bytes behind it that the last positions compare
	// into) has landed, under the upload of the next one; parse / Huffman / encode (or the Xpress emit kernels) follow over the whole buffer as
	// before: one stream's flag words, and the place of an Xpress+Huffman chunk in the output, couple all chunks. A copy from pageable memory holds
	// the calling thread, not the GPU, so no page-locking is needed for the overlap. (64 KiB chunks per range, 256 = 16 MiB; 51 MB, ms per call
	// Xpress / Xpress+Huffman: 32: 5.22 / 5.85, 64: 4.38 / 4.99, 128: 4.04 / 4.65, 256: 3.91 / 4.55, one copy: 4.23 / 4.92)
	const uint32_t ONE_RANGE_CHUNKS = env_one_range_chunks();
	const bool ranged = !decompress && (format == MSCOMP_XPRESS || format == MSCOMP_XPRESS_HUFF) && in_len >= env_one_ranged_min() &&
	                    zero_copy;                                             // (mscomp_amd_debug_set_one_shot(1) / MSCOMP_AMD_ONE_ZEROCOPY=0: the one-copy path, for A/B runs and tests)
	if (!ranged && in_len && hipMemcpyAsync(d_in, in, in_len, hipMemcpyHostToDevice, c->stream) != hipSuccess) { return MSCOMP_ERRNO; }
	struct { uint64_t len; int32_t st; int32_t pad; } meta;
	for (bool first = true;; first = false) {
		if (!c->one_out.reserve(dev_cap + 64)) { return MSCOMP_MEM_ERROR; }
		mscomp_amd_plan* p = nullptr;
		MSCompStatus s = tls.plan_for(format, decompress, in_len, dev_cap, &p);
		if (s != MSCOMP_OK) { return s; }
		if (ranged && first) {
			const uint32_t nch = p->n_chunks, nr = (nch + ONE_RANGE_CHUNKS - 1u) / ONE_RANGE_CHUNKS;
			if (!tls.slices(nr)) { return MSCOMP_MEM_ERROR; }
			uint16_t* links = static_cast<uint16_t*>(c->links.p); uint16_t* lasthead = static_cast<uint16_t*>(c->lasthead.p);
			uint16_t* mlen3 = static_cast<uint16_t*>(c->mlen3.p); uint16_t* moff = mlen3 + 1;
			const uint32_t max_off = format == MSCOMP_XPRESS ? 0x2000u : 0xFFFFu; const int clip = format == MSCOMP_XPRESS ? 0 : 1;
			if (hipEventRecord(tls.ev[0], c->stream) != hipSuccess || hipStreamWaitEvent(tls.h2d, tls.ev[0], 0) != hipSuccess) { return MSCOMP_ERRNO; }   // (the staging buffer's last reader was on the execution stream)
			for (uint32_t r = 0; r < nr; ++r) {
				const uint32_t c0 = r * ONE_RANGE_CHUNKS, cnt = nch - c0 < ONE_RANGE_CHUNKS ? nch - c0 : ONE_RANGE_CHUNKS;
				const size_t b0 = (size_t)c0 * 65536u + (r ? 64u : 0u);
				size_t b1 = (size_t)(c0 + cnt) * 65536u + 64u; if (b1 > in_len) { b1 = in_len; }
				if (b1 > b0 && hipMemcpyAsync(d_in + b0, in + b0, b1 - b0, hipMemcpyHostToDevice, tls.h2d) != hipSuccess) { return MSCOMP_ERRNO; }
				if (hipEventRecord(tls.ev[1 + r], tls.h2d) != hipSuccess || hipStreamWaitEvent(c->stream, tls.ev[1 + r], 0) != hipSuccess) { return MSCOMP_ERRNO; }
				{ KernelTimer t(c, "xp_links_kernel"); launch_xp_links_range(c->stream, d_in, p->bt, links, lasthead, c0, cnt); }
				{ KernelTimer t(c, "xp_find_kernel"); launch_xp_find_range(c->stream, d_in, p->bt, links, lasthead, mlen3, moff, max_off, clip, c0, cnt); }
			}
			p->matches_ready = true;
		}
		s = mscomp_amd_plan_execute(p, d_in, static_cast<uint8_t*>(c->one_out.p), d_len, d_st);
		p->matches_ready = false;                            // (a cached plan: whatever happened, its next execution finds its matches itself)
		if (s != MSCOMP_OK) { return s; }
		if (hipMemcpyAsync(&meta, d_len, sizeof meta, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
		    hipStreamSynchronize(c->stream) != hipSuccess) { return MSCOMP_ERRNO; }
		if (meta.st == MSCOMP_BUF_ERROR && dev_cap < cap) {          // only the staging was too small: decode again with room
			dev_cap = dev_cap > cap / 16 ? cap : dev_cap * 16;
			continue;
		}
		break;
	}
	if (meta.st != MSCOMP_OK) { return (MSCompStatus)meta.st; }
	size_t copy = (size_t)meta.len;
	if (!decompress && format == MSCOMP_LZNT1 && cap - copy >= 2) { copy += 2; }    // the uncounted End_of_buffer bytes (lznt1_compress.cpp:270)
	if (copy && hipMemcpy(out, c->one_out.p, copy, hipMemcpyDeviceToHost) != hipSuccess) { return MSCOMP_ERRNO; }
	*out_len = (size_t)meta.len;
	return MSCOMP_OK;
}

extern "C" {

MSCompStatus lznt1_compress(const uint8_t* in, size_t n, uint8_t* out, size_t* out_len)       { return one_shot(MSCOMP_LZNT1, false, in, n, out, out_len); }
MSCompStatus xpress_compress(const uint8_t* in, size_t n, uint8_t* out, size_t* out_len)      { return one_shot(MSCOMP_XPRESS, false, in, n, out, out_len); }
MSCompStatus xpress_huff_compress(const uint8_t* in, size_t n, uint8_t* out, size_t* out_len) { return one_shot(MSCOMP_XPRESS_HUFF, false, in, n, out, out_len); }

// the decompressors (lznt1_decompress.cpp:293 via internal.h:616-630, ...): same staging, the decoding happens on the GPU
MSCompStatus lznt1_decompress(const uint8_t* in, size_t n, uint8_t* out, size_t* out_len)       { return one_shot(MSCOMP_LZNT1, true, in, n, out, out_len); }
MSCompStatus xpress_decompress(const uint8_t* in, size_t n, uint8_t* out, size_t* out_len)      { return one_shot(MSCOMP_XPRESS, true, in, n, out, out_len); }
MSCompStatus xpress_huff_decompress(const uint8_t* in, size_t n, uint8_t* out, size_t* out_len) { return one_shot(MSCOMP_XPRESS_HUFF, true, in, n, out, out_len); }

#ifndef MSCOMP_AMD_NO_FACADE
MSCompStatus ms_decompress(MSCompFormat format, const uint8_t* in, size_t in_len, uint8_t* out, size_t* out_len)
{
	switch ((int)format) {
	case MSCOMP_LZNT1: case MSCOMP_XPRESS: case MSCOMP_XPRESS_HUFF: return one_shot(format, true, in, in_len, out, out_len);
	case MSCOMP_NONE:                                               // mscomp.cpp:26-32
		if (!out_len || in_len > *out_len) { return out_len ? MSCOMP_BUF_ERROR : MSCOMP_ARG_ERROR; }
		if (in_len) { memcpy(out, in, in_len); }
		*out_len = in_len; return MSCOMP_OK;
	default: return MSCOMP_ARG_ERROR;                                // mscomp.cpp:131
	}
}
MSCompStatus ms_compress(MSCompFormat format, const uint8_t* in, size_t in_len, uint8_t* out, size_t* out_len)
{
	switch ((int)format) {
	case MSCOMP_LZNT1: case MSCOMP_XPRESS: case MSCOMP_XPRESS_HUFF: return one_shot(format, false, in, in_len, out, out_len);
	case MSCOMP_NONE:                                               // the reference's "copy" codec (mscomp.cpp:26-32): host memcpy
		if (!out_len || in_len > *out_len) { return out_len ? MSCOMP_BUF_ERROR : MSCOMP_ARG_ERROR; }
		if (in_len) { memcpy(out, in, in_len); }
		*out_len = in_len; return MSCOMP_OK;
	default: return MSCOMP_ARG_ERROR;                                // mscomp.cpp:115
	}
}
#endif

} // extern "C"

