// beam_search_f16.hip -- the strict and fast kernels over the index's fp16 row copy: hs::strict_kernel_f16 / hs::fast_kernel_f16 (see beam_search.hip, narrow_rows.hip)
#define HS_TU_ROWS 2
#include "beam_search.hip"
