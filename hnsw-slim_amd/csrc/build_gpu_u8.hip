// build_gpu_u8.hip -- the batched build's search and link kernels over u8 rows in natural order: hs::bg_search_kernel_u8,
// hs::bg_link_kernel_u8 (see build_gpu.hip, build_rows.hpp)
#define HS_BG_ROWS 1
#include "build_gpu.hip"
