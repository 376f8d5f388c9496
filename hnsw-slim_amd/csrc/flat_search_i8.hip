// flat_search_i8.hip -- the flat kernel over the index's i8 row copy: hs::flat_kernel_i8 (see flat_search.hip, narrow_rows.hip)
#define HS_TU_ROWS 3
#include "flat_search.hip"
