// beam_search_i8.hip -- the strict and fast kernels over the index's i8 row copy: hs::strict_kernel_i8 / hs::fast_kernel_i8 (see beam_search.hip, narrow_rows.hip)
#define HS_TU_ROWS 3
#include "beam_search.hip"
