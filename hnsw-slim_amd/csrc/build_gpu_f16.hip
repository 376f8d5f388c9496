// build_gpu_f16.hip -- the batched build's search and link kernels over fp16 rows in natural order: hs::bg_search_kernel_f16,
// hs::bg_link_kernel_f16 (see build_gpu.hip, build_rows.hpp)
#define HS_BG_ROWS 2
#include "build_gpu.hip"
