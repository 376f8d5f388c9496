// flat_search_f16.hip -- the flat kernel over the index's fp16 row copy: hs::flat_kernel_f16 (see flat_search.hip, narrow_rows.hip)
#define HS_TU_ROWS 2
#include "flat_search.hip"
