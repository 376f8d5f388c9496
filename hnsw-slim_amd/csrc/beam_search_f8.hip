// beam_search_f8.hip -- the strict and fast kernels over the index's fp8 (E4M3) row copy: hs::strict_kernel_f8 / hs::fast_kernel_f8 (see beam_search.hip, narrow_rows.hip)
#define HS_TU_ROWS 5
#include "beam_search.hip"
