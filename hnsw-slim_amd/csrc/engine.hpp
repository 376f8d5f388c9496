// engine.hpp -- device-side index view + launch interface shared by the kernels (*.hip), the launch plan (search_plan.cpp) and the C ABI (capi_*.cpp).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "heap_emul.hpp"

namespace hs {

// Read-only index resident in HBM (one copy per GPU).
struct DevIndex {
  const float *vec;         // n x dim fp32, row-major, rows 64-byte aligned when dim % 16 == 0
  const uint32_t *row_ptr0; // n+1     : CSR row pointers of the level-0 adjacency
  const uint32_t *cols;     // n_edges : neighbour ids (level 0 first, then upper-level slices)
  const uint32_t *up_base;  // n       : first up_ptr entry of node i, 0xFFFFFFFF when level(i)==0
  const uint32_t *up_ptr;   //         : level-l slice of i = cols[up_ptr[b+l-1] .. up_ptr[b+l])
  const uint32_t *tile0;    // n x tile_stride: level-0 ids of node i padded with 0xFFFFFFFF to one
                            //         aligned tile (stride 16/32/48/64 ids), or null when max degree > 64
  const uint2 *uptile;      // (#upper slots) x up_stride {neighbour id, up_base[neighbour]}: level l of node i sits at slot
                            //         up_base[i] + l - 1, padded with 0xFFFFFFFF; null when an upper list exceeds 64 ids
  const uint64_t *labels;   // n
  const uint8_t *deleted;   // n       : delete mark as the reference reads it
  uint32_t n, dim, tile_stride, up_stride, ep_base;   // ep_base = up_base[enterpoint]
  int32_t maxlevel, threshold_level;
  uint32_t enterpoint;
  int32_t has_deleted, kind, metric;
};

enum : uint32_t { ST_TODO = 0, ST_DONE = 1, ST_OVERFLOW = 2, ST_HAZARD = 3 };

struct SearchArgs {
  const float *queries;  // nq x dim (device)
  uint32_t nq, k, ef;    // ef = max(ef_, k)   (hnswalg_slim.h:2080)
  uint32_t cand_cap;     // candidate-heap capacity (entries)
  uint32_t hash_slots;   // visited-set tier-1 (LDS) slots
  uint32_t *spill;       // per-query tier-2 region in global memory (nullable): [spill_slots u32 visited-set
                         // slots][cand2_cap x 8 B candidate-heap slots], spill_stride words apart
  uint32_t spill_slots, spill_stride, cand2_cap, log_cap;  // then log_cap x 8 B: result-set insertion log, then hop_cap bytes
  int32_t mode;          // hs_mode
  int32_t mark_ep;       // tag the enter point visited before the descent (slim (q,k) overloads)
  uint32_t select_mask;  // process query qi iff (1 << status[qi]) & select_mask
  uint32_t grid;         // workgroups to launch (grid-stride over queries)
  uint32_t *out_labels32;
  uint64_t *out_labels64;
  float *out_dists;
  uint32_t *out_counts;
  uint32_t *stats;       // nq x 4 {n_dist, n_hops, n_nbr, pass that answered}   (nullable)
  Pair *raw_top;         // nq x raw_stride (nullable; strict kernel only)
  uint32_t *raw_size;    // nq
  uint32_t raw_stride;
  uint32_t *status;      // nq
  uint32_t *counters;    // [0] visited-set overflows, [1] candidate-heap overflows, [2] tie hazards, [3] tier-2 spills (this pass)
  uint32_t pass_id;
  uint32_t hash_fill_shift;   // visited-set tier 1 is frozen at 1 - 2^-shift of its slots (0 = the default 2: 75 %)
  uint32_t flat;         // fast kernel: start the level-0 search without the candidate heap (beam_search.hip, FLAT)
  uint32_t hop_cap;      // bytes of the per-expansion accept counts behind the insertion log (one per expansion of the flat start)
  uint32_t vis_bits;     // fast kernel: 0 = visited-set tier 1 in 32-bit slots; else the width of the id space for the
                         // 16-bit form (search_common.hpp; hash_slots / 4 buckets, a power of two, vis_bits - log2(buckets) <= 16)
  // Fast kernel in two launches (see launch_order): phase 1 stops after the upper-level descent and leaves
  // {level-0 entry node, its distance, n_dist, n_hops} in entry[qi]; phase 2 takes its queries in the order order[] gives
  // and starts each from its entry.  phase 0: one launch does both, in index order.
  uint32_t phase;
  uint4 *entry;
  const uint32_t *order;
  // Last-resort pass (strict kernel, pass_id 2): candidate heap and tier-2 visited set in per-WORKGROUP regions of global memory
  // (cand_cap entries / spill_slots words each, indexed by blockIdx.x), so that the launch -- which goes out with every batch and is
  // normally empty -- asks for a dozen KiB of LDS instead of a drained CU.  Null in every other pass.
  void *fb_cand;
  uint32_t *fb_spill;
  // Flat kernel (flat_search.hip): visited set of fl_nb 16-byte buckets; bucket = h mod fl_nb, remainder = h div fl_nb =
  // umulhi(h, fl_mul) >> fl_sh (exact for h < 2^vis_bits; remainders fit 15 bits)
  uint32_t fl_nb, fl_mul, fl_sh;
};

// Filter set of a search (filter_set.hip; fast and strict kernels).  nf bitmap rows of `stride` words: bit i & 31 of word i >> 5 of
// row f is set iff filter f allows internal id i; query qi (its index in THIS launch's arrays, whatever order or pass takes it)
// searches under row of_query[qi].  A node is excluded iff it is marked deleted or its bit is clear.  A query whose filter index
// is >= nf touches no row: count 0, padding outputs, *bad raised.
// A kernel ARGUMENT OF ITS OWN of the filter-set entry points (hs::strict_kernel / hs::fast_kernel overloads and their narrow
// twins), as the narrow rows are: SearchArgs and the kernels that take only it are what they were, instruction for instruction
// -- their register and scratch lines are pinned (tests/test_f32_free_cpu.py), and SearchArgs' size is part of those lines.
struct FilterArgs {
  const uint32_t *rows;
  const uint32_t *of_query;
  uint32_t *bad;
  uint32_t stride, nf;
};

// Bytes of dynamic LDS one query (one wavefront) needs.
size_t strict_lds_bytes(uint32_t dim, uint32_t ef, uint32_t cand_cap, uint32_t hash_slots);
size_t fast_lds_bytes(uint32_t dim, uint32_t ef, uint32_t cand_cap, uint32_t hash_slots);
// Fast path availability for this shape (level-0 tile present, threshold_level == 0, k < ef <= 512).  has_filter: the search
// names a filter set, which counts as delete marks do (the !bare_bone branches).
bool fast_supported(const DevIndex &ix, uint32_t ef, uint32_t k, bool has_filter = false);
// Which instantiation of the fast kernel answers a call that fast_supported() admits: the one table the fast launchers and
// launch_fast_del / _md dispatch on (search_plan.cpp; host only, no HIP call; hs_debug_fast_shape hands it out).
//   d16  : the distance pass over fp32 rows -- dim / 16 compiled in (> 0), -dim / 4 for a compiled-in dim % 4 == 0 shape off the
//          SIMD16 path (< -1), 0 = runtime dim with dim % 16 == 0, -1 = any runtime dim.  (The narrow objects hold the d16 = 0
//          shapes only and take slots / wb from here.)
//   slots: result-set entries per lane S = 1 | 2 | 4 | 8 for ef <= 64 | 128 | 256 | 512
//   wb   : ef == k on a bare index: the variant that watches ties across the capacity boundary (S <= 2)
// bare = no delete marks and no filter set (the reference's bare_bone_search).
struct FastShape { int32_t d16, slots, wb; };
FastShape fast_shape(int metric, uint32_t dim, uint32_t ef, uint32_t k, bool bare);

// Strict kernel: the reference's result/candidate arrays with libstdc++ heap mechanics, reference
// output order.  Fast kernel: same traversal and candidate mechanics, result set kept as a sorted
// register array; queries whose answer could depend on the result heap's layout are flagged ST_HAZARD.
// order[] = the queries sorted by decreasing entry[].y (distance of the level-0 entry), bucket-exact: the queries likely
// to take the most expansions start first, so that a launch does not end on a few late-started long ones.
hipError_t launch_order(const uint4 *entry, uint32_t *order, uint32_t nq, hipStream_t stream);
// Lean kernel (lean_search.hip): the fast kernel's algorithm with a keys-only result set (no ids, no LDS staging of the merge).
bool lean_supported(const DevIndex &ix, uint32_t ef, uint32_t k);
size_t lean_lds_bytes(uint32_t dim, uint32_t ef, uint32_t cand_cap, uint32_t hash_slots);
// Flat kernel (flat_search.hip): lazy candidate heap -- replayed from the insertion log only when its layout decides a pop.
bool flatk_supported(const DevIndex &ix, uint32_t ef, uint32_t k);
size_t flatk_lds_bytes(uint32_t dim, uint32_t ef, uint32_t nb);
uint32_t flatk_waves_per_cu(uint32_t dim, uint32_t ef);
hipError_t flat_heap_ops(const uint32_t *d_ops, uint32_t n_ops, uint2 *d_spill, uint2 *d_heap, uint2 *d_pops, uint32_t *d_n, int wave_pop,
                         uint32_t lds_slots, hipStream_t stream);

// ---- launching a search kernel ----------------------------------------------------------------------------------------------
// launch_search (search_launch.cpp) is the one way in: the kernel family (hs_plan_family) over rows of format row_fmt (ROWS_F32:
// ix.vec; ROWS_U8 | ROWS_F16: narrow_rows, the index's copy of ix.vec in the lane-major layout of narrow_rows.hip), metric ix.metric.
// f != null: the search runs under that filter set -- the !bare_bone branches whether or not the index has delete marks
// (hnswalg.h:1421, hnswalg_slim.h:1884); strict and fast kernels only.  It launches nothing and returns
//   hipErrorInvalidDevicePointer  when the row array the kernel would read is null and the index is not empty (an index may drop
//                                 its fp32 rows, hs_index_set_f32_resident: no search kernel dereferences null on the device);
//   hipErrorInvalidValue          for a narrow format with dim % 16 != 0, for a family / format / metric that does not exist or has
//                                 no kernel (the lean kernel has no narrow twin), and for a filter set handed to the flat or lean kernel.
// Behind it is a table [family][row format][metric] of launchers, one per (family, row format, metric), each defined by the
// object that holds its kernels (beam_search.hip: strict and fast; flat_search.hip: flat; lean_search.hip: lean), each computing
// its LDS size from its own layout function and picking the instantiation for the shape.  HS_LAUNCHER names them -- here, where
// they are defined, and in the table -- with rows = f32 | u8 | f16 and metric = l2 | ip.
using SearchLauncher = hipError_t (*)(const DevIndex &, const SearchArgs &, const void *rows, hipStream_t, const FilterArgs *);
hipError_t launch_search(int family, int row_fmt, const DevIndex &ix, const SearchArgs &a, const void *narrow_rows, hipStream_t stream,
                         const FilterArgs *f);
#define HS_LAUNCHER_(family, rows, metric) launch_##family##_##rows##_##metric
#define HS_LAUNCHER(family, rows, metric) HS_LAUNCHER_(family, rows, metric)   // (rows may itself be a macro: HS_ROWS_ID of the kernel files)
#define HS_LAUNCHERS(family, rows) HS_LAUNCHER(family, rows, l2), HS_LAUNCHER(family, rows, ip)
std::remove_pointer_t<SearchLauncher> HS_LAUNCHERS(strict, f32), HS_LAUNCHERS(strict, f16), HS_LAUNCHERS(strict, u8), HS_LAUNCHERS(fast, f32),
    HS_LAUNCHERS(fast, f16), HS_LAUNCHERS(fast, u8), HS_LAUNCHERS(flat, f32), HS_LAUNCHERS(flat, f16), HS_LAUNCHERS(flat, u8), HS_LAUNCHERS(lean, f32);

// Narrow rows (narrow_rows.hip): launch_narrow_convert fills rows [row0, row0 + nrows) of the index's u8 / fp16 copy (fmt = ROWS_U8
// | ROWS_F16) from d_vec and lowers *d_first_bad (preset to 0xFFFFFFFF) to the smallest row that holds a value the format cannot
// represent.  launch_narrow_widen is the inverse of the conversion: rows [row0, row0 + nrows) of d_vec from the copy (exact).
hipError_t launch_narrow_convert(const float *d_vec, void *d_out, int fmt, uint32_t row0, uint32_t nrows, uint32_t dim, uint32_t *d_first_bad,
                                 hipStream_t stream);
hipError_t launch_narrow_widen(const void *d_rows, float *d_vec, int fmt, uint32_t row0, uint32_t nrows, uint32_t dim, hipStream_t stream);
// Filter sets (filter_set.hip).  launch_filter_pack: rows [0, count) of d_allowed (count x n bytes, non-zero = allowed) into count
// bitmap rows of row_words words at d_words, padding bits and words zero.  launch_filter_unpack: one bitmap row into n bytes (0 / 1).
hipError_t launch_filter_pack(const uint8_t *d_allowed, uint32_t *d_words, uint32_t n, uint32_t count, uint32_t row_words, hipStream_t stream);
hipError_t launch_filter_unpack(const uint32_t *d_row, uint8_t *d_allowed, uint32_t n, hipStream_t stream);

}  // namespace hs
