// envnum.h -- how the library reads the string of an environment variable (null: the variable is unset). Pure functions of that string: no
// cache, no HIP, and no look-up of their own -- hooks.hip, which holds one accessor per variable, is the only file that asks the environment.
// tests/envnum_host.cpp runs them on the CPU.
#pragma once
#include <cstdlib>

namespace msc { namespace envnum {

// a ranged integer: what atol reads (blanks skipped, "12abc" is 12, no digits is 0) when the variable is set and that lies in [lo, hi], else def
inline long ranged(const char* s, long lo, long hi, long def)
{
	const long v = s ? atol(s) : def;
	return s && v >= lo && v <= hi ? v : def;
}
// the two flag forms: the variable is set (to anything, the empty string too); its first character is c (c = 0: set and empty)
inline bool is_set(const char* s) { return s != nullptr; }
inline bool starts(const char* s, char c) { return s && *s == c; }

} } // namespace msc::envnum
