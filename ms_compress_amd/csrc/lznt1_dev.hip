// lznt1_dev.hip -- the DEV instances of the LZNT1 chunk kernels (compress plans with device tables, kernels.h launch_lznt1_chunks), in a code
// object of their own: lznt1.hip's keeps the host plans' kernels alone.
#define LZNT1_DEV_TU
#include "lznt1.hip"
