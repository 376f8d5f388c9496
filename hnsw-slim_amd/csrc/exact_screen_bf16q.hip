// exact_screen_bf16q.hip -- exact k-NN for bf16 queries over the bf16 rows of a resident index: exact_screen_f16q.hip
// compiled for the other 16-bit element, an object of its own so that hs::xh_screen_kernel's code object stays what it was and a kernel
// trace shows hs::xb_screen_kernel as a row of its own.  The split of the work is that file's -- query pack in slot order, a 64-query
// tile in LDS as half words in operand layout, one 16-byte global load per lane and matrix step straight from the narrow copy, lists,
// re-rank and fallback scan of exact_screen.hip -- because a bf16 row and an fp16 row are the same bytes per step.  What differs:
//   the matrix step     v_mfma_f32_32x32x16_bf16; a product of two bf16 values has 16 significand bits and is exact in fp32 unless it
//                       underflows, which the fp16 screen could rule out and this one cannot;
//   the margin          exact_screen_margin as it stands: its (d + 8) 2^-120 term covers underflowed products and bf16 subnormals the
//                       pipeline may flush (exact_screen_margin.hpp, "The bf16 screen"), so nothing is counted per row or per query --
//                       XhInfo.sub is written as zero and never read;
//   the pre-test        the fp16 screen's one FMA and compare, with one more reason to send a query to the full test: an L2 query of
//                       squared norm below 2^-40, where absolute underflow terms are no longer small beside the relative slack the
//                       pre-test's proof spends (exact_screen_bf16_pre_skip);
//   widening            a shift, for the fp32 copy of the queries, the norms and the hand-over (xb_widen_kernel).
#define HS_XH_BF16 1
// the names of this object (kernels' host stubs and launch entries have external linkage)
#define xh_rowinfo_kernel xb_rowinfo_kernel
#define xh_widen_kernel xb_widen_kernel
#define xh_pack_kernel xb_pack_kernel
#define xh_screen_kernel xb_screen_kernel
#define xh_screen_body xb_screen_body
#define xh_steps xb_steps
#define xh_load xb_load
#define xh_is_sub xb_is_sub
#define xh_wide xb_wide
#define xh_h8 xb_h8
#define XhScan XbScan
#define XhGroup XbGroup
#define xh_supported xb_supported
#define xh_slice xb_slice
#define xh_screen_lds_bytes xb_screen_lds_bytes
#define xh_kernel_name xb_kernel_name
#define launch_exact_f16q_rowinfo launch_exact_bf16q_rowinfo
#define launch_exact_f16q_widen launch_exact_bf16q_widen
#define launch_exact_screen_f16q launch_exact_screen_bf16q
#include "exact_screen_f16q.hip"
