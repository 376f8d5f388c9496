// search_tu.hpp -- what a search kernel file (beam_search.hip, flat_search.hip, lean_search.hip) is compiled as: the build makes
// one object per metric and row format from each of them (Makefile), and these macros say which one this is.
#pragma once
#include <cstdint>

// -DHS_TU_METRIC=0 holds the L2 kernels and everything that is not per metric, -DHS_TU_METRIC=1 the inner-product kernels (the
// kernel instantiations are the build's critical path).  Without the macro one translation unit holds both (make asm / prof / asan).
#if !defined(HS_TU_METRIC)
#define HS_TU_HAS_L2 1
#define HS_TU_HAS_IP 1
#elif HS_TU_METRIC == 0
#define HS_TU_HAS_L2 1
#define HS_TU_HAS_IP 0
#else
#define HS_TU_HAS_L2 0
#define HS_TU_HAS_IP 1
#endif

// HS_TU_ROWS = 1 | 2 (the *_u8.hip / *_f16.hip files): the same kernels over the index's narrow copy of the rows
// (hs_index_set_row_format), as objects of their own per row format and metric so that a kernel trace shows them as separate rows;
// those hold the narrow entry points and their launchers, nothing else.  The narrow kernels take the rows as a kernel argument of
// their own (DevIndex and SearchArgs are what they were).  What differs between the row formats, all of it, beside the expression
// the search body reads its rows from (HS_ROW_SRC / HS_ROWS_READ, per file):
#if !defined(HS_TU_ROWS)
#define HS_TU_ROWS 0
#endif
#if HS_TU_ROWS == 0
#define HS_ROWS_ID f32               // the launchers' names (engine.hpp HS_LAUNCHER)
#define HS_KERNEL(name) name         // the kernels' names
#define HS_ROWS_PARAM                // their trailing parameter (before FilterArgs in the filter-set form)
#define HS_ROWS_ARG                  // the launcher's `rows` as that parameter
#else
#if HS_TU_ROWS == 1
#define HS_ROWS_ID u8
#define HS_KERNEL(name) name##_u8
namespace hs { typedef uint8_t TuRow; }
#else
#define HS_ROWS_ID f16
#define HS_KERNEL(name) name##_f16
namespace hs { typedef _Float16 TuRow; }
#endif
#define HS_ROWS_PARAM , const TuRow *rows
#define HS_ROWS_ARG , reinterpret_cast<const TuRow *>(rows)
#endif
