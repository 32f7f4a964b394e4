// The POA kernel with the per-row score check compiled in (CHECKED,
// poa_kernel.hip; the rule is poa_score_row_refused in poa_types.hpp): the
// same source as poa_kernel.hip for the variants that run unbanded rows
// (narrow, mid, full), timed and untimed, under a launch function of its own
// (launch_poa_kernel_checked). A translation unit of its own, as the large
// class has one: the unchecked kernels do not see the check, and the units
// compile in parallel.
#define RGA_POA_SCORE_CHECK 1
#include "hip/poa_kernel.hip"
