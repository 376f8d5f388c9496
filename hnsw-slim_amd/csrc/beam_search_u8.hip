// beam_search_u8.hip -- the strict and fast kernels over the index's u8 row copy: hs::strict_kernel_u8 / hs::fast_kernel_u8 (see beam_search.hip, narrow_rows.hip)
#define HS_TU_ROWS 1
#include "beam_search.hip"
