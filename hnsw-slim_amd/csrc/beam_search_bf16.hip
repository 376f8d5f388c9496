// beam_search_bf16.hip -- the strict and fast kernels over the index's bf16 row copy: hs::strict_kernel_bf16 / hs::fast_kernel_bf16 (see beam_search.hip, narrow_rows.hip)
#define HS_TU_ROWS 4
#include "beam_search.hip"
