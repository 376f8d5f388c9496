// flat_search_f8.hip -- the flat kernel over the index's fp8 (E4M3) row copy: hs::flat_kernel_f8 (see flat_search.hip, narrow_rows.hip)
#define HS_TU_ROWS 5
// The IP object widens one element per instruction (v_cvt_f32_fp8 with a byte select, as the u8 kernels do): v_cvt_pk_f32_fp8 writes an
// aligned register pair, and with it the compiled d = 128 / 96 IP shapes spilled 12 B per lane and two d = 960 shapes 4 .. 8 B more than
// their u8 twins.  The L2 object and the strict / fast kernels keep the packed conversion.
#if HS_TU_METRIC == 1
#define HS_F8_SINGLE 1
#endif
#include "flat_search.hip"
