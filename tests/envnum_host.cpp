// envnum_host.cpp -- csrc/envnum.h on the CPU (tests/test_envnum_host.py compiles and runs it). Reads lines of NAME=VALUE settings joined
// by ';' (NAME alone: unset) and prints, for the first name of each line, what that variable's accessor in csrc/hooks.hip computes: the
// accessors' expressions, restated here over E in place of getenv and without their caches (the test holds every ranged(...) call of this file
// to the one of the same variable in hooks.hip, text for text). The constants are the defaults of kernels.h and host.h.
#include "envnum.h"
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>

#define XPS_SEG 16384u
#define XPS_WARM 16384u
#define XPS_ROUNDS 8u
#define LZB_MIN_KB 32
#define LZG_HOPS 8u
#define HB_SLOTS 8

using msc::envnum::ranged;
static std::map<std::string, std::string> g_env;
static const char* E(const char* name) { auto it = g_env.find(name); return it == g_env.end() ? nullptr : it->second.c_str(); }

static uint64_t mib_budget(const char* e, long def) { const long v = ranged(e, LONG_MIN, LONG_MAX, def); return (uint64_t)(v < 0 ? 0 : v) << 20; }
static uint32_t env_xps_seg() { const uint32_t v = (uint32_t)(ranged(E("MSCOMP_AMD_XPS_SEG_KB"), 4, 65536, XPS_SEG >> 10) << 10); return v; }

static bool eval(const std::string& name, unsigned long long& out)
{
	if (name == "MSCOMP_AMD_LZG_MAX_MB") { out = mib_budget(E("MSCOMP_AMD_LZG_MAX_MB"), 65536); }
	else if (name == "MSCOMP_AMD_XHC_SCR_MAX_MB") { out = mib_budget(E("MSCOMP_AMD_XHC_SCR_MAX_MB"), 32768); }
	else if (name == "MSCOMP_AMD_ONE_SLICE_MB") { out = (size_t)ranged(E("MSCOMP_AMD_ONE_SLICE_MB"), 1, 4096, 24) << 20; }
	else if (name == "MSCOMP_AMD_ONE_RANGED_MIN_MB") { out = (size_t)ranged(E("MSCOMP_AMD_ONE_RANGED_MIN_MB"), 1, 65536, 8) << 20; }
	else if (name == "MSCOMP_AMD_ONE_RANGE_CHUNKS") { out = (uint32_t)ranged(E("MSCOMP_AMD_ONE_RANGE_CHUNKS"), 1, 65536, 256); }
	else if (name == "MSCOMP_AMD_HOST_BATCH_MB") { out = (size_t)ranged(E("MSCOMP_AMD_HOST_BATCH_MB"), 1, 65536, 0) << 20; }
	else if (name == "MSCOMP_AMD_HOST_SLOTS") { out = (size_t)ranged(E("MSCOMP_AMD_HOST_SLOTS"), 1, HB_SLOTS, HB_SLOTS); }
	else if (name == "MSCOMP_AMD_XPS_SEG_KB") { out = env_xps_seg(); }
	else if (name == "MSCOMP_AMD_XPS_WARM_KB") { const uint32_t v = (uint32_t)(ranged(E("MSCOMP_AMD_XPS_WARM_KB"), 1, 65536, XPS_WARM >> 10) << 10); out = v < env_xps_seg() ? v : env_xps_seg(); }
	else if (name == "MSCOMP_AMD_XPS_ROUNDS") { out = (uint32_t)ranged(E("MSCOMP_AMD_XPS_ROUNDS"), 1, 256, XPS_ROUNDS); }
	else if (name == "MSCOMP_AMD_LZB_MIN_KB") { out = (uint32_t)(ranged(E("MSCOMP_AMD_LZB_MIN_KB"), 1, (1 << 20) - 1, LZB_MIN_KB) << 10); }
	else if (name == "MSCOMP_AMD_LZG_HOPS") { out = (uint32_t)ranged(E("MSCOMP_AMD_LZG_HOPS"), 1, 999, LZG_HOPS); }
	else { return false; }
	return true;
}

int main()
{
	char line[512];
	while (fgets(line, sizeof line, stdin)) {
		line[strcspn(line, "\n")] = 0;
		g_env.clear();
		std::string first;
		for (char* tok = strtok(line, ";"); tok; tok = strtok(nullptr, ";")) {
			char* eq = strchr(tok, '=');
			const std::string name = eq ? std::string(tok, eq) : std::string(tok);
			if (first.empty()) { first = name; }
			if (eq) { g_env[name] = eq + 1; }
		}
		unsigned long long v = 0;
		if (!eval(first, v)) { printf("?\n"); continue; }
		printf("%llu\n", v);
	}
	return 0;
}
