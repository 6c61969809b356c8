// The signature table of libttd_rt.so's plan exports (kernels/abi.h): ttd_abi_count / ttd_abi_entry.
#include "common.h"

TTD_ABI_TABLE(ttd_abi)
