// flat_search_u8.hip -- the flat kernel over the index's u8 row copy: hs::flat_kernel_u8 (see flat_search.hip, narrow_rows.hip)
#define HS_TU_ROWS 1
#include "flat_search.hip"
