// flat_search_bf16.hip -- the flat kernel over the index's bf16 row copy: hs::flat_kernel_bf16 (see flat_search.hip, narrow_rows.hip)
#define HS_TU_ROWS 4
#include "flat_search.hip"
