// The POA kernel compiled for the large capacity class (kPoaLargeLimits,
// 4095 nodes per window): the same source as poa_kernel.hip, with the class
// selected by a macro, under a launch function of its own
// (launch_poa_kernel_large). The regular class's translation unit does not
// see this one, so its code is what it was before the large class existed.
#define RGA_POA_LARGE_CLASS 1
#include "hip/poa_kernel.hip"
