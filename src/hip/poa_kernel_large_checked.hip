// The large capacity class (poa_kernel_large.hip) with the per-row score
// check compiled in (poa_kernel_checked.hip), under
// launch_poa_kernel_large_checked.
#define RGA_POA_LARGE_CLASS 1
#define RGA_POA_SCORE_CHECK 1
#include "hip/poa_kernel.hip"
