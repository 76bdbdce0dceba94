// ctx.hip -- the context of the C-ABI of libmscomp_amd.so (include/mscomp_amd.h): version and size bounds, context create / destroy, the
// profiler, the LZNT1 dictionary flavour. Host code only, as the other files of the ABI: plan.hip and launch.hip (host plans), plan_dev.hip
// (plans with device tables), hooks.hip (test hooks, switches, environment), oneshot.hip (the drop-in entry points).
//
// Reference boundary mirrored here: ms_max_compressed_size (the reference's src/mscomp.cpp:96-101).
#include "host.h"
#include <mutex>

using namespace msc;

// the flavour a plan created in `c` right now would get
bool msc::lznt1_sa_for(const mscomp_amd_ctx* c) { return (c->lznt1_sa >= 0 ? c->lznt1_sa : g_sw.lznt1_sa_default.load(std::memory_order_relaxed)) != 0; }

// Bytes an OPTIONAL fast-path scratch buffer may take: the environment's cap, and never more than half of what the device has free
// right now (what the buffer already holds counts as free: reserve() reuses it). The fast paths have fallbacks that need no scratch,
// so a plan never fails for them (the environment's defaults assume a 288 GB device that is otherwise empty; a caller may hold most of it).
uint64_t msc::optional_scratch_budget(uint64_t env_cap, size_t already_held)
{
	size_t free_b = 0, total_b = 0;
	if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); return env_cap; }
	const uint64_t half = ((uint64_t)free_b + already_held) / 2;
	return env_cap < half ? env_cap : half;
}

extern "C" {

const char* mscomp_amd_version(void) { return "mscomp_amd 0.6 (gfx950, HIP; LZNT1 / Xpress / Xpress+Huffman compressors and decompressors, LZNT1 streaming, host batches over several GPUs)"; }

size_t lznt1_max_compressed_size(size_t n)       { return lznt1_max_out(n); }
size_t xpress_max_compressed_size(size_t n)      { return xpress_max_out(n); }
size_t xpress_huff_max_compressed_size(size_t n) { return xpress_huff_max_out(n); }
#ifndef MSCOMP_AMD_NO_FACADE   /* define when src/mscomp.cpp of the reference is linked too */
size_t ms_max_compressed_size(MSCompFormat f, size_t n)
{
	switch ((int)f) {
	case MSCOMP_NONE:        return n;
	case MSCOMP_LZNT1:       return lznt1_max_compressed_size(n);
	case MSCOMP_XPRESS:      return xpress_max_compressed_size(n);
	case MSCOMP_XPRESS_HUFF: return xpress_huff_max_compressed_size(n);
	default:                 return (size_t)-1;                          // mscomp.cpp:98
	}
}
#endif

// The LZNT1 bucket sort and the Xpress chain links are only bit-exact when the returning same-address LDS atomics of one
// wave instruction are served in lane order (util.hip: lds_lane_order_kernel). That is how gfx950 behaves, but it is not an
// architectural promise, so the library checks the device it is about to use, once per device and process. A device that serves them in
// another order gets the order-independent form of the two kernels (one lane at a time: kernels.h set_serial_atomics -- the same bytes,
// a slower sort); a device on which the check cannot RUN is refused (MSCOMP_ERRNO): wrong bytes must never leave silently.
static int lane_order_verdict(int device, hipStream_t st)
{
	static std::mutex mu;
	static int verdict[64];                            // 0 = unknown, 1 = in order, -1 = out of order / check failed
	if (device >= 64) { device = 63; }
	std::lock_guard<std::mutex> lk(mu);
	if (verdict[device] == 0) {
		uint32_t* d_bad = nullptr;
		uint32_t bad = 0xFFFFFFFFu;
		if (hipMalloc(reinterpret_cast<void**>(&d_bad), 64) == hipSuccess) {
			bad = run_lds_lane_order_check(st, 0x5EEDu + (uint32_t)device, 64, 64, 97, d_bad);     // 64 blocks x 64 rounds x 64 lanes x {add, exchange}
			if (bad == 0) { bad = run_lds_lane_order_check(st, 0xC0FFEEu, 64, 64, 2048, d_bad); }
			(void)hipFree(d_bad);
		}
		verdict[device] = bad == 0 ? 1 : (bad == 0xFFFFFFFFu ? -1 : 2);             // 2 = runs, out of order: the serial form
		if (verdict[device] == 2) { set_serial_atomics(device, 1); }
	}
	return verdict[device];
}

MSCompStatus mscomp_amd_ctx_create(int device, void* hip_stream, mscomp_amd_ctx** out)
{
	if (!out) { return MSCOMP_ARG_ERROR; }
	*out = nullptr;
	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) { return MSCOMP_ERRNO; }
	DeviceGuard g(device);
	if (!g.ok) { return MSCOMP_ERRNO; }
	if (lane_order_verdict(device, (hipStream_t)hip_stream) < 1) { return MSCOMP_ERRNO; }
	mscomp_amd_ctx* c = new (std::nothrow) mscomp_amd_ctx();
	if (!c) { return MSCOMP_MEM_ERROR; }
	c->device = device; c->stream = (hipStream_t)hip_stream;
	c->cpd_blocks = compact_dev_blocks();
	c->crc_blocks = crc_dev_blocks();
	(void)place_blocks(false); (void)place_blocks(true);           // (the grid of the LZNT1 placement, kept per device in util.hip: asked here, not inside a capture)
	*out = c;
	return MSCOMP_OK;
}

void mscomp_amd_ctx_destroy(mscomp_amd_ctx* c)
{
	if (!c) { return; }
	DeviceGuard g(c->device);
	(void)hipStreamSynchronize(c->stream);
	for (auto& r : c->recs) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
	for (auto e : c->free_events) { (void)hipEventDestroy(e); }
	for (DevBuf* b : c->bufs()) { b->release(); }
	for (DevBuf& b : c->table_pool) { b.release(); }
	if (c->h_tab) { (void)hipHostFree(c->h_tab); }
	if (c->h_tab_ev) { (void)hipEventDestroy(c->h_tab_ev); }
	delete c;
}

void mscomp_amd_profile_enable(mscomp_amd_ctx* c, int on) { if (c) { c->profiling = on != 0; } }

int mscomp_amd_profile_read(mscomp_amd_ctx* c, const char** names, double* ms, uint64_t* launches, int cap)
{
	if (!c) { return 0; }
	DeviceGuard g(c->device);
	(void)hipStreamSynchronize(c->stream);
	int n = 0;
	for (auto& r : c->recs) {
		float t = 0.f; (void)hipEventElapsedTime(&t, r.a, r.b);
		int k = 0;
		for (; k < n; ++k) { if (names[k] == r.name) { break; } }
		if (k == n) { if (n >= cap) { continue; } names[n] = r.name; ms[n] = 0; launches[n] = 0; ++n; }
		ms[k] += t; launches[k] += 1;
		c->free_events.push_back(r.a); c->free_events.push_back(r.b);
	}
	c->recs.clear();
	return n;
}

// The LZNT1 dictionary flavour is a property of a PLAN, fixed when the plan is created (the reference fixes it when the library is built,
// config.h:83-88): from its context's setting (mscomp_amd_ctx_set_lznt1_sa_dict) or, when the context has none, from the process default below.
// Changing either never touches a plan that exists, so callers that run plans concurrently keep their bytes. The one-shot entries (ms_compress,
// ms_deflate: no context argument) and the host-batch entry create their plans per call and follow the process default of that moment.
void mscomp_amd_set_lznt1_sa_dict(int on) { g_sw.lznt1_sa_default.store(on ? 1 : 0, std::memory_order_relaxed); }
int  mscomp_amd_get_lznt1_sa_dict(void) { return g_sw.lznt1_sa_default.load(std::memory_order_relaxed); }
MSCompStatus mscomp_amd_ctx_set_lznt1_sa_dict(mscomp_amd_ctx* c, int on)
{
	if (!c || on < -1 || on > 1) { return MSCOMP_ARG_ERROR; }
	c->lznt1_sa = on;
	return MSCOMP_OK;
}

} // extern "C"
