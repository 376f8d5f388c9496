/* hnsw_slim_amd.h -- C ABI of the MI355X-native HNSW / HNSW-Slim batched search engine.
 *
 * This is the drop-in boundary for the reference's searchKnn -> searchBaseLayerST -> distance path
 * (SURVEY.md section 8b).  Plain pointers and sizes only; every entry point names the reference
 * interface it replaces (paths relative to /root/reference/third_party/hnswlib/).  The C++ facade
 * hnsw-slim_amd/hnswlib/hnswlib_amd.h re-creates hnswlib::HierarchicalNSW / HierarchicalNSWSlim /
 * L2Space / InnerProductSpace on top of these calls.
 *
 * Error convention: every call returns an hs_status; hs_last_error() gives the thread-local message,
 * which reuses the reference's exception texts ("Cannot open file", "Index seems to be corrupted or
 * unsupported", ...) so the facade can re-throw std::runtime_error with the same what().
 * There is NO CPU fallback: without a HIP device every search entry point fails with HS_ERR_DEVICE.
 */
#ifndef HNSW_SLIM_AMD_H
#define HNSW_SLIM_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hs_index hs_index;

typedef enum {
  HS_OK = 0,
  HS_ERR_IO = 1,          /* "Cannot open file"                         hnswalg.h:785, hnswalg_slim.h:757 */
  HS_ERR_CORRUPT = 2,     /* "Index seems to be corrupted or unsupported" hnswalg.h:823-836.  Also every file, conversion input and
                           * patch stream whose graph would send a kernel out of bounds (the preconditions of csrc/index_check.hpp:
                           * ids, list counts and offsets, levels, enter point, level ownership).  Guaranteed: a refused input has
                           * reached no device array, and an index it was meant for, host image included, is exactly as before. */
  HS_ERR_NOMEM = 3,       /* "Not enough memory: ..."                   hnswalg_slim.h:785-788 */
  HS_ERR_INVALID = 4,     /* bad argument                                */
  HS_ERR_UNSUPPORTED = 5, /* e.g. SlimQ with dim < 64, brute force k > 64  */
  HS_ERR_DEVICE = 6,      /* HIP runtime error / no device               */
  HS_ERR_CAPACITY = 7     /* a query outgrew even the fallback on-chip scratch */
} hs_status;

typedef enum { HS_KIND_HNSW = 0, HS_KIND_SLIM = 1, HS_KIND_SLIMQ = 2 } hs_kind;   /* hnswalg.h:18 / hnswalg_slim.h:29 / hnswalg_slimq.h:41 */
typedef enum { HS_METRIC_L2 = 0, HS_METRIC_IP = 1 } hs_metric; /* space_l2.h:208 / space_ip.h:342  */

/* Which searchKnn overload a batch call reproduces. */
typedef enum {
  /* HierarchicalNSWSlim::searchKnn(const void*, size_t k, tableint* result)  hnswalg_slim.h:2030-2131:
   * k uint32 labels per query in the reference's post-nth_element array order. */
  HS_MODE_SLIM_IDS = 0,
  /* priority_queue-returning overloads: HierarchicalNSW::searchKnn hnswalg.h:1378-1440 and
   * HierarchicalNSWSlim::searchKnn(q,k) hnswalg_slim.h:1907-2028: <=k (dist,label) pairs per query. */
  HS_MODE_PQ = 1
} hs_mode;

typedef struct {
  uint64_t n, dim;
  int32_t kind, metric, maxlevel, threshold_level;
  uint32_t enterpoint;
  int32_t has_deleted;
  uint64_t n_edges;      /* entries of the CSR column array (all levels) */
  uint64_t device_bytes; /* HBM held by this index */
  uint64_t max_degree0;
  uint64_t index_size;   /* the reference's indexSize() for this index: hnswalg.h:1533-1547, hnswalg_slim.h:2435-2444,
                            hnswalg_slimq.h:2047-2057 (graph structure of the CPU layout, without the vectors) */
} hs_info;

const char *hs_last_error(void);

/* Number of HIP devices visible (0 when none); does not initialise a device context. */
int hs_device_count(void);

/* loadIndex(path, space, max_elements): hnswalg.h:781-893 (HS_KIND_HNSW), hnswalg_slim.h:753-815
 * (HS_KIND_SLIM), hnswalg_slimq.h:1218-1313 (HS_KIND_SLIMQ).  Parses the reference's serialized index, repacks it
 * (row-major vectors + CSR adjacency + fixed-stride tiles; RaBitQ records for SlimQ) and uploads it to HIP device
 * `device`.  ef starts at 10 as in the reference.  Both metrics take every dim. */
hs_status hs_index_load(const char *path, int kind, int metric, size_t dim, size_t max_elements,
                        int device, hs_index **out);
/* The same, from the serialized bytes already in host memory (what saveIndex would have written: hnswalg.h:748-779,
 * hnswalg_slim.h:717-751, hnswalg_slimq.h:1161-1216) -- for hosts that receive the index over a socket
 * (hnsw_slim_server.cc:59-81) or keep it in a buffer; nothing is written to disk.  The bytes are not retained. */
hs_status hs_index_load_mem(const void *bytes, size_t len, int kind, int metric, size_t dim, size_t max_elements,
                            int device, hs_index **out);
/* Upload an index the host has already parsed (no file involved): what a caller that holds the reference's public members
 * (hnswalg_slim.h:30 onwards, all public) or its own graph hands over.  Node i owns levels[i] + 1 consecutive neighbour lists,
 * level 0 first; list t = list_ids[list_ptr[t] .. list_ptr[t+1]).  labels NULL = row index, deleted NULL = none marked.
 * kind: HS_KIND_HNSW or HS_KIND_SLIM (selects the searchKnn overload semantics); threshold_level applies to Slim.
 * What a list may hold: any ids < n, in any order -- an id named twice or more, the node's own id (a self-loop), ids of marked nodes,
 * nothing at all.  The lists are stored as given and answered as the reference answers them: its visited array skips the later
 * occurrences at level 0 (hnswalg.h:392-393), its upper-level descent has no visited array and evaluates a repeated id again
 * (:1389-1415), and the counters say so.  (An index with a level-0 list that repeats an id is served by the fast / strict kernels, never
 * by the flat kernel: hs_plan_in.has_dup0.)  n == 0 is an index without elements: every search on it returns count 0.
 * What the arrays must satisfy (csrc/index_check.hpp; HS_ERR_INVALID otherwise, before anything is uploaded, no index created):
 * 0 <= levels[i] <= maxlevel, enterpoint < n, levels[enterpoint] >= maxlevel >= 0, threshold_level >= 0, list_ptr non-decreasing,
 * every id < n, and every id in a level-l list (l >= 1) names a node of level >= l.  The arrays are checked before the device is
 * asked for: without a device, bad arrays report HS_ERR_INVALID and good ones HS_ERR_DEVICE. */
hs_status hs_index_from_host_arrays(int kind, int metric, size_t n, size_t dim, const float *vectors, const uint64_t *labels,
                                    const uint8_t *deleted, const int32_t *levels, const uint64_t *list_ptr,
                                    const uint32_t *list_ids, uint32_t enterpoint, int32_t maxlevel, int32_t threshold_level,
                                    int device, hs_index **out);
/* patchFromStream(std::istream&, bool to_add): hnswalg_slim.h:2292-2340, wire format of genPatch :1427-1476 as the reference's
 * server frames it (hnsw_slim_server_patch.cc:280-290, after its `finished` word): u64 cur_element_count, u64 changed_old_cnt,
 * u64 changed_new_cnt, then per changed node  u32 id | 8 B {level, total_neighbor} (old node) or 16 B {level, total, label}
 * (new node) | u32 neighborsSize | blob | the vector (new node, to_add).  Applies to a HS_KIND_SLIM index that was loaded with
 * max_elements > its element count (the reference needs the same room, hnswalg_slim.h:784).  Only the changed nodes' rows of the
 * vectors and level-0 tiles are rewritten in HBM; the small structure arrays are rebuilt.  Like the reference, the stream
 * does not move the enter point.  Not to be called while a search on this index is in flight.
 * The records are staged and the image as it would stand after them is checked whole (csrc/index_check.hpp: a staged record answers
 * for its node, the image for every other; a chunk of a diff may name new nodes whose records come in a later chunk: until then they
 * have no lists, which every kernel tests) before a byte changes.  A refused stream (HS_ERR_CORRUPT, HS_ERR_CAPACITY,
 * HS_ERR_UNSUPPORTED) has reached no device array and leaves the host image byte for byte as it was: hs_slim_index_save, the next
 * patch and hs_slim_convert_diff work from the unchanged image. */
hs_status hs_index_patch(hs_index *ix, const void *bytes, size_t len, int to_add);
/* ---- live updates of a resident vanilla index: addPoint, markDelete, unmarkDelete, saveIndex, getDataByLabel ----------------
 * A HS_KIND_HNSW index loaded with max_elements > its element count keeps its host image (as a patchable Slim index does) and
 * device arrays for max_elements rows.  The calls below change such an index in place.  As hs_index_patch: not while a search on the
 * index is in flight (each call synchronises the device); a filter set created for the old n is refused after an add; filter sets
 * survive marks untouched (marks are never folded into their rows).
 *
 * addPoint(data, label) for `count` NEW labels (hnswalg.h:1248-1376): row i becomes internal id n + i.  The insertion runs on the
 * host image exactly as the reference's (threads == 1: its serial order; more threads: as hs_build_hnsw, timing dependent); on the
 * device only the changed nodes are written -- one staging copy, one kernel (csrc/index_update.hip): level-0 tile row, fp32 row
 * and / or narrow row, label, mark -- and the small structure arrays (CSR, upper levels) are rebuilt whole.  A level-0 list that
 * outgrows the tile stride re-tiles everything.  All or nothing, checked before anything changes:
 *   HS_ERR_CAPACITY    "The number of elements exceeds the specified limit" (:1274-1277; also an index loaded without room)
 *   HS_ERR_UNSUPPORTED a label that already exists (this entry adds; hs_index_upsert_points updates); a row the index's narrow row format cannot
 *                      represent (the message names the row of the call and the value); a Slim / SlimQ index
 *   HS_ERR_INVALID     a label that appears twice in the call
 * Levels come from the index's level generator: after a load it is a default-constructed std::default_random_engine, as the
 * reference's is (its loading constructor, hnswalg.h:78-83, seeds nothing); hs_index_seed_levels seeds it as the building
 * constructor does (:113) and discards `drawn` draws, which resumes a build that has added `drawn` points exactly. */
hs_status hs_index_add_points(hs_index *ix, const float *rows, const uint64_t *labels, size_t count, int threads);
hs_status hs_index_seed_levels(hs_index *ix, size_t seed, size_t drawn);
/* markDelete (on != 0, hnswalg.h:923-958) / unmarkDelete (on == 0, :968-1001) of `count` labels of any HS_KIND_HNSW index (no host
 * image needed).  All or nothing, HS_ERR_INVALID with the reference's texts: "Label not found", "The requested to delete element is
 * already deleted", "The requested to undelete element is not deleted" (a label named twice in one call meets its own first mark).
 * hs_info.has_deleted follows num_deleted_ > 0 in both directions (:1421): the first mark moves a bare index from the flat kernel
 * to the fast / strict kernels, removing the last mark moves it back.  HS_ERR_UNSUPPORTED on Slim / SlimQ indexes. */
hs_status hs_index_mark_deleted(hs_index *ix, const uint64_t *labels, size_t count, int on);
/* saveIndex (hnswalg.h:748-779) of the host image, marks and added points included.  HS_ERR_INVALID for an index without one. */
hs_status hs_index_save(const hs_index *ix, const char *path);
/* getDataByLabel (hnswalg.h:896-917): out[dim], read back from the device -- the fp32 row, or the narrow row of an index without
 * fp32 rows, widened (exact).  HS_ERR_INVALID "Label not found" for a label that is missing or marked deleted. */
hs_status hs_index_get_row(hs_index *ix, uint64_t label, float *out);
size_t hs_index_capacity(const hs_index *ix);        /* getMaxElements: rows the index has room for */
size_t hs_index_deleted_count(const hs_index *ix);   /* getDeletedCount */

/* ---- upsert, replace_deleted and resizeIndex on a resident vanilla index ---------------------------------------------------------
 * The same kind of index as above (HS_KIND_HNSW, loaded with max_elements > its element count), the same rules about searches in
 * flight.  Everything runs on the host image exactly as the reference's serial code (updatePoint hnswalg.h:1067-1157,
 * repairConnectionsForUpdate :1159-1236, addPoint(.., replace_deleted) :1025-1065, deleted_elements as its std::unordered_set), so
 * hs_index_save writes the reference's bytes; on the device the rewritten nodes -- fp32 row and / or narrow row, label, mark,
 * level-0 tile row -- and the level-0 neighbours the update touched leave in one staging copy and one kernel, as
 * hs_index_add_points' records do.  updateNeighborProbability is 1.0.
 *
 * hs_index_set_replace_deleted: the constructor's allow_replace_deleted_.  Turning it on fills deleted_elements from the current
 * marks in increasing id, as loadIndex does (:882-888); from then on hs_index_mark_deleted keeps it.  HS_ERR_INVALID on an index
 * without a host image, HS_ERR_UNSUPPORTED on Slim / SlimQ.
 *
 * hs_index_upsert_points: `count` points serially, in call order, each exactly addPoint(row, label, replace_flags[i]);
 * replace_flags NULL = all 0.  An existing label is updated (and un-marked first when replacement is not allowed); a new label with
 * its flag set and a vacancy takes the slot `*deleted_elements.begin()` -- the slot's old label leaves the index, the mark goes;
 * otherwise the point is appended.  A label may occur more than once in a call: later occurrences are updates.  All or nothing -- a
 * pre-pass plays labels, vacancies and capacity and refuses before anything changes:
 *   HS_ERR_INVALID     "Replacement of deleted elements is disabled in constructor" (:1027-1030)
 *   HS_ERR_INVALID     "Can't use addPoint to update deleted elements if replacement of deleted elements is enabled." (:1257-1263)
 *   HS_ERR_CAPACITY    "The number of elements exceeds the specified limit" (:1274-1277; also an index loaded without room)
 *   HS_ERR_UNSUPPORTED a row the index's narrow row format cannot represent (named as hs_index_add_points names it); Slim / SlimQ
 * No `threads`: the order is the reference's serial one; bulk appends of new labels stay with hs_index_add_points.
 * hs_info.has_deleted follows the number of marks after every call: a replacement that removes the last mark returns the index
 * to the flat kernel.  Filter sets are per internal id: updates and replacements leave n unchanged, so an existing set stays valid
 * and a reused slot KEEPS ITS BIT -- the caller rewrites it (hs_filter_set_write) if the new label's admission differs; after
 * appends a set is refused, as after hs_index_add_points.
 *
 * hs_index_resize: resizeIndex (:689-717).  HS_ERR_INVALID "Cannot resize, max element is less than the current number of
 * elements"; HS_ERR_INVALID on an index without a host image.  Growing allocates the per-node device arrays (fp32 rows where
 * resident, narrow rows where present, level-0 tiles, labels, marks) at the new capacity and fills them by device-to-device copies
 * -- no row crosses the host link -- then frees the old ones; HS_ERR_NOMEM, index as it was, when the new arrays cannot be
 * allocated.  Shrinking to a value >= the element count lowers only the reported capacity (the device arrays stay).  Search
 * outputs do not change; filter sets stay valid; hs_index_capacity and hs_info.index_size follow, hs_info.device_bytes changes by
 * the narrow copy's capacity term only (rows are counted per element, the narrow copy per row of capacity). */
hs_status hs_index_set_replace_deleted(hs_index *ix, int on);
hs_status hs_index_upsert_points(hs_index *ix, const float *rows, const uint64_t *labels, const uint8_t *replace_flags, size_t count);
hs_status hs_index_resize(hs_index *ix, size_t new_max_elements);

/* ---- narrow rows (no counterpart in the reference) -------------------------------------------------------------------
 * Besides the resident fp32 rows an index can hold a u8 or fp16 copy of them, and the flat kernel -- the default kernel of every
 * bare index -- then reads that copy (hs::flat_kernel_u8 / hs::flat_kernel_f16) and a quarter / half of the row bytes.  The copy must
 * represent every stored value exactly: u8 -> fp32 and fp16 -> fp32 are exact, the query stays fp32 and the distance is the same
 * fp32 recipe in the same order, so distances, labels, counters and tie behaviour are bit-identical to HS_ROWS_F32.  It is an
 * explicit call because it is a contract on the data: it costs device memory (one value of the format per value of the fp32 array's
 * row capacity: max(n, max_elements) x dim x 1 or 2 bytes, included in hs_info.device_bytes while it exists) and a later
 * hs_index_patch may only add representable rows (HS_ERR_UNSUPPORTED otherwise, index untouched).
 * What reads what: while the fp32 rows are resident (the state after hs_index_set_row_format) the flat kernel reads the copy and
 * every other kernel (strict / fast: filters, delete marks, exact order, ef > 512, threshold_level > 0, the re-run pass,
 * hs_search_batch_raw) reads the fp32 rows.  After hs_index_set_f32_resident(ix, 0) the fp32 rows are gone and EVERY search
 * kernel reads the copy: the kernel choice stays what it was and the narrow twin of the chosen kernel is launched
 * (hs::flat_kernel_u8 / _f16, hs::fast_kernel_u8 / _f16, hs::strict_kernel_u8 / _f16, the re-run pass included), with the same
 * bits in every output.  The index then occupies a quarter (u8) or half (fp16) of the row bytes instead of 5/4 or 3/2 of them. */
typedef enum { HS_ROWS_F32 = 0, HS_ROWS_F16 = 1, HS_ROWS_U8 = 2 } hs_row_format;
/* Builds (or, for HS_ROWS_F32, drops) the narrow copy of the rows on the index's device.  Not to be called while a search on this
 * index is in flight (as hs_index_patch).  HS_ERR_UNSUPPORTED, index left exactly as it was, when a stored value is not
 * representable (the message names the first offending row and the value), for a SlimQ index, and for dim % 16 != 0 (the flat
 * kernel does not serve those). */
hs_status hs_index_set_row_format(hs_index *ix, int format);
int hs_index_row_format(const hs_index *ix);
/* Host only, no device: *first_bad = n when every value of rows[n x dim] is representable in `format`, else the index of the
 * first row that is not.  Representable: x == (float)(T)x, NaN and +-inf never -- u8: the integers 0 .. 255 (and -0.0f, read back
 * as +0.0f, which cannot change a distance); fp16: every finite fp16 value, subnormals included. */
hs_status hs_rows_representable(const float *rows, size_t n, size_t dim, int format, uint64_t *first_bad);
/* on = 0: free the resident fp32 rows of an index that holds a narrow copy; from then on EVERY search kernel reads the copy.
 * on = 1: re-create them from the copy (widening is exact; a u8 index reads +0.0f where -0.0f was stored).
 * hs_info.device_bytes falls / rises by exactly max(n, max_elements) x dim x 4.  Both are idempotent.  on = 0 on an index in
 * HS_ROWS_F32 format is HS_ERR_INVALID.  While the fp32 rows are absent hs_index_set_row_format to any OTHER format (HS_ROWS_F32
 * included) is HS_ERR_INVALID, index untouched: restore the fp32 rows first.  hs_index_patch works in both states (the patched
 * rows go into the copy; a patch that forces a re-tile rebuilds the copy from the host image in bounded chunks and never
 * allocates the fp32 array).  The lean kernel (diagnostic, chosen by environment only) has no narrow twin: HS_KERNEL=lean and
 * HS_LEAN_MIN_EF fall through to the fast kernel on such an index.  Not to be called while a search on this index is in
 * flight (as hs_index_patch). */
hs_status hs_index_set_f32_resident(hs_index *ix, int on);
int hs_index_f32_resident(const hs_index *ix);
/* Host only, no device: out[n x dim] of `format` (HS_ROWS_U8: bytes, HS_ROWS_F16: IEEE half words) in the lane-major layout of
 * the device copy, out[r * dim + s * (dim / 8) + 2 i + e] = rows[r][16 i + 2 s + e]; *first_bad as hs_rows_representable;
 * nothing is written beyond row *first_bad.  HS_ERR_INVALID for a format other than U8 / F16, HS_ERR_UNSUPPORTED for
 * dim % 16 != 0. */
hs_status hs_rows_to_narrow(const float *rows, size_t n, size_t dim, int format, void *out, uint64_t *first_bad);
/* hs_index_load, but the rows go to the device in `format` only: the result equals load + set_row_format(format) +
 * set_f32_resident(0), and the fp32 array is never allocated on the device (the rows are converted on the host,
 * hs_rows_to_narrow, and uploaded in chunks of at most 64 MiB).  Refusals as hs_index_set_row_format (unrepresentable value with
 * the first offending row named, SlimQ, dim % 16 != 0); *out stays NULL. */
hs_status hs_index_load_narrow(const char *path, int kind, int metric, size_t dim, size_t max_elements, int device,
                               int format, hs_index **out);
void hs_index_free(hs_index *ix);                        /* ~HierarchicalNSW* / clear(): hnswalg_slim.h:154-167 */
hs_status hs_set_ef(hs_index *ix, size_t ef);            /* setEf: hnswalg.h:184, hnswalg_slim.h:193 */
hs_status hs_index_info(const hs_index *ix, hs_info *out);
/* Name of the device kernel that served pass 0 of the most recent search call on this index ("hs::flat_kernel", ...): the kernel
 * a rocprofv3 kernel trace of that call shows; for measurement scripts, no counterpart in the reference. */
const char *hs_last_kernel(const hs_index *ix);

/* Output-order policy of the result set.  0 (default): the fast kernel answers, each query's entries
 * come out sorted by ascending distance; the k-subset (ids and distances) is exactly the reference's --
 * queries where the reference's choice depends on its heap layout (a distance tie across the k-th
 * boundary) are detected and re-run with the reference's heap mechanics.  1: every query runs the strict
 * kernel and HS_MODE_SLIM_IDS reproduces the reference's post-nth_element array ORDER as well
 * (hnswalg_slim.h:2126-2130 leaves an unordered k-subset). */
hs_status hs_set_exact_order(hs_index *ix, int on);

/* On-chip scratch sizing per query (0 = automatic from ef): candidate-heap capacity and visited-set
 * hash slots (power of two).  Queries that outgrow it are re-run with a whole CU's LDS. */
hs_status hs_set_capacity(hs_index *ix, uint32_t cand_cap, uint32_t hash_slots);

/* Batched searchKnn over nq host-resident queries (nq x dim, row-major fp32).  Outputs (host):
 *   mode HS_MODE_SLIM_IDS: out_labels32[nq*k] (required); out_dists[nq*k] (nullable) in the same order.
 *   mode HS_MODE_PQ      : out_labels64[nq*k] + out_dists[nq*k] (required): the pairs left in
 *                          top_candidates after popping down to k, heap-array order; out_counts[nq].
 *   out_counts[nq] (nullable): number of valid entries per query (min(k, found)); unused slots hold
 *                          0xFFFFFFFF / UINT64_MAX / +inf.
 *   stats (nullable): nq x 4 uint32 {n_dist, n_hops, n_nbr_read, pass}  (SURVEY.md 8d); pass = 0 first
 *                          pass, 1 tie re-run (strict kernel), 2 scratch-overflow re-run.
 * Synchronous: includes H2D of queries and D2H of results.
 * Value range (every graph search entry: this one, the filtered, filter-set, async, device and SlimQ ones): rows and queries must
 * be finite.  The answer is the reference's for every FINITE distance, over the whole fp32 range -- subnormal products, sums and
 * distances are kept as the reference compiled without fast-math keeps them, inner-product distances may change sign inside one
 * result set, magnitudes up to FLT_MAX (tests/test_gpu_value_range.py).  A distance that is not finite (an L2 sum or an inner
 * product that overflows, a NaN) makes the outcome unspecified: the kernels use FLT_MAX and +inf as "no value", as the empty
 * threshold and as reduction identities, and nothing on the hot path checks for it. */
hs_status hs_search_batch(hs_index *ix, const float *queries, size_t nq, size_t k, int mode,
                          uint32_t *out_labels32, uint64_t *out_labels64, float *out_dists,
                          uint32_t *out_counts, uint32_t *stats);

/* searchKnn(q, k, BaseFilterFunctor* isIdAllowed): hnswalg.h:1378-1440 with :347-349,441-444, and
 * hnswalg_slim.h:1783-1905 with :462-618.  The functor is a host callback, so the caller evaluates it once
 * per element: allowed[i] != 0 iff (*isIdAllowed)(label of internal id i) (hs_labels() gives the labels).
 * Always the priority_queue result shape (HS_MODE_PQ outputs).  Slim indexes: threshold_level == 0 only. */
hs_status hs_search_batch_filtered(hs_index *ix, const float *queries, size_t nq, size_t k,
                                   const uint8_t *allowed, uint64_t *out_labels64, float *out_dists,
                                   uint32_t *out_counts, uint32_t *stats);
/* External labels by internal id (n entries), to evaluate a filter functor on the host. */
hs_status hs_labels(const hs_index *ix, uint64_t *out_labels);

/* ---- filter sets: device-resident filters, one per query in one batch (no counterpart in the reference, where a filter is a
 * host functor handed to one searchKnn call) ------------------------------------------------------------------------------
 * A filter set is nf filters over the n internal ids of one index, held on the index's device as bitmaps: bit i & 31 of word
 * i >> 5 of row f is set iff filter f allows internal id i (the "by internal id" convention of allowed[] above); a row is
 * hs_filter_row_words(n) words -- ceil(n / 32) rounded up to a multiple of 4, so that rows start 16-byte aligned -- and every
 * padding bit is zero.  A search names the set and one filter index per query: queries under different filters (tenants, ACL
 * groups, categories) run in ONE launch, and nothing is rebuilt or uploaded per call.
 * The index's own delete marks still apply and are never folded into the rows: a node is excluded iff it is marked deleted OR
 * its bit is clear, so a later hs_index_patch that marks nodes deleted needs no rewrite of the set.
 * A set is bound to the device it was created on and to the n it was created for: a search is refused with HS_ERR_INVALID,
 * nothing launched, when the index holds another n (it grew through hs_index_patch: create a new set), lives on another device,
 * or is a SlimQ index. */
typedef struct hs_filter_set hs_filter_set;
/* Host only, no device.  hs_filter_pack: allowed[nf x n] bytes (non-zero = allowed) -> out_words[nf x hs_filter_row_words(n)]. */
size_t hs_filter_row_words(size_t n);
hs_status hs_filter_pack(const uint8_t *allowed, size_t n, size_t nf, uint32_t *out_words);
/* nf rows for the index's current n, all bits zero.  Refused as hs_search_batch_filtered refuses (SlimQ: HS_ERR_INVALID; a Slim
 * index with threshold_level > 0: HS_ERR_UNSUPPORTED), and nf == 0 with HS_ERR_INVALID; *out stays NULL. */
hs_status hs_filter_set_create(hs_index *ix, size_t nf, hs_filter_set **out);
void hs_filter_set_free(hs_filter_set *fs);
/* Rows [first, first + count) from count x n host bytes (staged through a bounded device buffer and packed on the device), from
 * host words in hs_filter_pack's layout (a plain copy), or from count x n DEVICE bytes (a mask computed on the GPU, e.g. a torch
 * bool / uint8 tensor; packed asynchronously on `stream`).  Not to be called while a search that reads those rows is in flight on
 * another stream. */
hs_status hs_filter_set_write(hs_filter_set *fs, size_t first, size_t count, const uint8_t *allowed);
hs_status hs_filter_set_write_bits(hs_filter_set *fs, size_t first, size_t count, const uint32_t *words);
hs_status hs_filter_set_write_dev(hs_filter_set *fs, size_t first, size_t count, const uint8_t *d_allowed, void *stream);
/* Row f unpacked into out_allowed[n] (0 / 1); the set's shape (every output nullable; device_bytes = nf x row_words x 4). */
hs_status hs_filter_set_read(hs_filter_set *fs, size_t f, uint8_t *out_allowed);
hs_status hs_filter_set_info(const hs_filter_set *fs, uint64_t *nf, uint64_t *n, uint64_t *row_words, uint64_t *device_bytes);
/* hs_search_batch_filtered with query i under row filter_of_query[i] of the set: same outputs (HS_MODE_PQ), same bits as a
 * hs_search_batch_filtered call with that row's allowed[].  Synchronous, host pointers; a filter index >= nf is HS_ERR_INVALID
 * before anything is launched. */
hs_status hs_search_batch_filter_set(hs_index *ix, const hs_filter_set *fs, const float *queries, size_t nq, size_t k,
                                     const uint32_t *filter_of_query, uint64_t *out_labels64, float *out_dists,
                                     uint32_t *out_counts, uint32_t *stats);
/* The same with DEVICE pointers, asynchronous on `stream`; pair with hs_search_check like the other _dev entries.  The filter
 * indices cannot be checked on the host: a query whose index is >= nf reads no row, returns count 0 with padding labels and
 * distances (the other queries of the batch are not disturbed) and raises a sticky per-stream counter that the next
 * hs_search_check on that stream reports as HS_ERR_INVALID, with the number of such queries in the message. */
hs_status hs_search_batch_filter_set_dev(hs_index *ix, const hs_filter_set *fs, const float *d_queries, size_t nq, size_t k,
                                         const uint32_t *d_filter_of_query, uint64_t *d_out_labels64, float *d_out_dists,
                                         uint32_t *d_out_counts, uint32_t *d_stats, void *stream);

/* Same search with DEVICE pointers, asynchronous on `stream` (a hipStream_t; NULL = default stream).
 * No host synchronisation happens here; call hs_search_check() after synchronising to learn whether
 * any query exhausted the fallback scratch. */
hs_status hs_search_batch_dev(hs_index *ix, const float *d_queries, size_t nq, size_t k, int mode,
                              uint32_t *d_out_labels32, uint64_t *d_out_labels64, float *d_out_dists,
                              uint32_t *d_out_counts, uint32_t *d_stats, void *stream);
hs_status hs_search_check(hs_index *ix, void *stream);
/* Parity/debug entry: a sequence of candidate_set operations (std::push_heap / std::pop_heap with compare_by_first_rev,
 * hnswalg_slim.h:177-183, 331-332, 353-354, 408-411) through the flat kernel's heap code on the device.  ops: 3 words each
 * {0 = push | 1 = pop, distance bits, id}; wave_pop selects the whole-wave pop; lds_slots: heap slots kept in LDS (the rest
 * in global memory).  out_heap / out_pops: 2 words per entry (n_ops entries of room each); out_n: {final size, pops}. */
hs_status hs_debug_heap_ops(const uint32_t *ops, size_t n_ops, int wave_pop, uint32_t lds_slots, uint32_t *out_heap, uint32_t *out_pops,
                            uint32_t *out_n);

/* Parity/debug entries: the launch plan of a search batch -- which kernel serves pass 0, whether the pass is split, every scratch
 * share -- as the pure function of the three structs below that the search path itself calls (csrc/search_plan.hpp).  The
 * structs are diagnostic: their layout may change between versions.
 * hs_plan_diag: the diagnostic environment knobs, as hs_debug_plan_input reads them once per process. */
typedef enum { HS_PLAN_KERNEL_DEFAULT = 0, HS_PLAN_KERNEL_LEAN = 1, HS_PLAN_KERNEL_FAST = 2 } hs_plan_kernel;   /* HS_KERNEL */
typedef enum { HS_PLAN_ZERO_COPY_ON = 0, HS_PLAN_ZERO_COPY_OFF = 1, HS_PLAN_ZERO_COPY_IN = 2 } hs_plan_zero_copy; /* HS_ZERO_COPY: unset, "0", "in" */
typedef struct hs_plan_diag {
  int32_t kernel;              /* HS_KERNEL=lean|fast (hs_plan_kernel); any other value is the default choice */
  int32_t lean_forced;         /* HS_LEAN_MIN_EF is set: the lean kernel where it can serve, never the flat one */
  uint32_t lean_min_ef;        /* ... from this ef upwards (64 when unset) */
  int32_t order;               /* HS_ORDER: -1 = unset (split pass 0 from 6144 queries), 0 = never, 1 = always, 2 = always, the fast
                                * kernel without the order launch */
  int32_t flat;                /* HS_FLAT=0 -> 0: the fast kernel uses its candidate heap from the first expansion; else 1 */
  int32_t vis16;               /* HS_VIS16=0 -> 0: the fast kernel's visited set in 32-bit slots everywhere; else 1 */
  int32_t flat_waves_per_cu;   /* HS_FLAT_WAVES_PER_CU: residency the flat kernel's LDS share is planned for (0 = the kernel's own) */
  int32_t zero_copy;           /* HS_ZERO_COPY (hs_plan_zero_copy); not part of the launch plan */
  int32_t verbose;             /* HS_VERBOSE is set; not part of the launch plan */
  int32_t slimq_fused;         /* HS_SLIMQ_FUSED=0 -> 0 (read at every SlimQ load); not part of the launch plan */
} hs_plan_diag;
/* Everything the plan may depend on. */
typedef struct hs_plan_in {
  uint64_t n, dim;
  int32_t has_tile0, has_uptile;   /* level-0 / upper-level adjacency tiles exist (max degree <= 64) */
  int32_t maxlevel, threshold_level, has_deleted, kind;
  uint64_t ef, k, nq;              /* ef as hs_set_ef left it (the search runs with max(ef, k)); nq: queries of the launch group */
  int32_t mode;
  uint32_t user_cand_cap, user_hash_slots;   /* hs_set_capacity */
  uint32_t grow_cand, grow_hash;             /* doublings hs_search_check learnt from earlier batches */
  int32_t exact_order, want_raw, has_filter; /* hs_set_exact_order; raw outputs requested; the search names a filter set */
  int32_t row_fmt, f32_resident;             /* hs_index_set_row_format, hs_index_set_f32_resident */
  int32_t has_dup0;                          /* some level-0 list names an id twice: such an index is never the flat kernel's */
  hs_plan_diag diag;
} hs_plan_in;
typedef enum { HS_PLAN_FLAT = 0, HS_PLAN_LEAN = 1, HS_PLAN_FAST = 2, HS_PLAN_STRICT = 3 } hs_plan_family;
typedef struct hs_plan_out {
  int32_t family, rows;        /* pass 0: kernel family (hs_plan_family) and the row format it reads (hs_row_format) */
  int32_t split, skip_order;   /* pass 0 runs as descent / order / level-0 search; ... without the order launch */
  uint32_t ef, mark_ep;
  uint32_t cand_cap, hash_slots, vis_bits, hash_fill_shift, flat;   /* pass 0 (SearchArgs fields of the same names) */
  uint32_t lds_bytes;          /* dynamic LDS a pass-0 workgroup asks for (the family's *_lds_bytes) */
  /* the flat kernel's visited set, planned whether or not that kernel serves pass 0: buckets nb, multiplier m, shift s, id-space
   * bits B, fits the LDS; bucket = h mod nb and remainder = h div nb = umulhi(h, m) >> s must be exact for every h < 2^B and the
   * remainders must fit 15 bits (tests/test_host_cpu.py) */
  uint32_t fl_nb, fl_mul, fl_sh, fl_bits, fl_ok;
  int32_t rerun_rows;          /* the re-run pass (strict kernel): its row format, statuses, scratch */
  uint32_t rerun_select_mask, rerun_cand_cap, rerun_hash_slots;
  uint32_t spill_stride, log_cap, hop_cap;   /* words of tier-2 scratch per query and two of its regions */
  const char *name;            /* what hs_last_kernel reports after the batch */
} hs_plan_out;
/* Host only, no device needed.  HS_ERR_INVALID / HS_ERR_CAPACITY as the search itself would return them. */
hs_status hs_debug_search_plan(const hs_plan_in *in, hs_plan_out *out);
/* Fills *in from a live index and the process's knobs, through the function every search launch uses. */
hs_status hs_debug_plan_input(const hs_index *ix, size_t k, size_t nq, int has_filter, int want_raw, hs_plan_in *in);
/* Parity/debug entry, host only: which instantiation of the fast kernel (hs::fast_kernel) a call launches once the plan names that
 * family -- the table the launchers themselves dispatch on (csrc/engine.hpp fast_shape).  bare: no delete marks and no filter set.
 * d16: the distance pass over fp32 rows, dim / 16 compiled in (> 0) or -dim / 4 for a compiled-in dim off the 16-wide path (< -1);
 * 0 / -1 are the runtime-dim shapes for dim % 16 == 0 / any dim (the narrow-row twins run 0 at every dim).  slots: result-set
 * entries per lane, 1 | 2 | 4 | 8 for ef <= 64 | 128 | 256 | 512.  wb: the ef == k variant that watches ties across the capacity
 * boundary.  HS_ERR_INVALID for a bad metric, dim = 0 or max(ef, k) beyond 512 (no fast shape). */
typedef struct hs_fast_shape { int32_t d16, slots, wb; } hs_fast_shape;
hs_status hs_debug_fast_shape(int metric, uint64_t dim, uint64_t ef, uint64_t k, int bare, hs_fast_shape *out);

/* Host pointers, asynchronous: H2D of the queries, the search and D2H of the requested outputs are enqueued on `stream`
 * and nothing is valid until that stream is synchronised (hs_search_check does it and reports capacity problems).  The
 * serving shape of the reference's query loop (include/strategy/hnsw_slim_strategy.h:107-118: the clock runs around the
 * whole loop, queries in, labels out): batches issued round-robin on a few streams overlap each other's copies and
 * kernels.  queries and outputs should be page-locked (hs_host_alloc, or hipHostMalloc / hipHostRegister of the
 * caller's own buffers): with pageable memory the copies are staged synchronously.  Staging buffers are per
 * (index, stream): do not reuse a stream for a second call on the same index before the first one's outputs are read.
 * Small batches (up to 2 MiB of queries) in device-mapped page-locked buffers are served IN PLACE: no staging copies, the
 * kernels read each query from `queries` and write the results into the output buffers directly -- so `queries` must stay
 * unchanged, and the outputs unread, until the batch has completed on `stream` (as for the copies, only for longer). */
hs_status hs_search_batch_async(hs_index *ix, const float *queries, size_t nq, size_t k, int mode,
                                uint32_t *out_labels32, uint64_t *out_labels64, float *out_dists,
                                uint32_t *out_counts, uint32_t *stats, void *stream);
void *hs_host_alloc(size_t bytes);   /* page-locked host memory (NULL on failure) */
void hs_host_free(void *p);
/* The device's address of a page-locked host buffer that is mapped into the device's address space (hs_host_alloc, hipHostMalloc,
 * mapped hipHostRegister), or NULL (pageable memory).  hs_search_batch_async serves small batches from such buffers in place;
 * a caller of hs_search_batch_dev may pass this address as d_queries for the same effect (the kernels read each query once). */
void *hs_host_device_pointer(const void *host);

/* ---- search queue: small submissions from many callers, one launch (no counterpart in the reference, whose callers run one
 * searchKnn per query: include/strategy/hnsw_slim_strategy.h:112-114) ---------------------------------------------------------
 * Every search entry above serves one caller's batch with one launch group, and the engine is fast only when that batch is large.
 * A queue on a resident HNSW or Slim index takes small batches from any thread, with host or device buffers, gathers everything
 * pending into one contiguous query array with one kernel (hs::gather_rows_kernel), runs ONE ordinary search launch group over it
 * -- the plan, the kernels and the bits of hs_search_batch_dev for that many queries -- and hands each query's results to its own
 * caller's buffers with one kernel (hs::scatter_results_kernel).  Filter sets let queries under different filters share a launch;
 * a queue lets queries of different callers share one.
 * Grouping.  k, mode and the filter set are fixed per queue; ef is the index's at the moment of the flush.  max_queries: 1..32768
 *   (one launch group always suffices); slots: 1..16 launches in flight, each with its own stream and staging; a flush that finds
 *   every slot busy blocks on the oldest launch.  A submission that would take the pending total past max_queries first flushes
 *   what is pending and then joins the next launch; one with nq > max_queries is refused (HS_ERR_INVALID, nothing changes);
 *   nq == 0 returns a ticket that is already complete.
 * Threads.  Every hs_queue_* call on one queue is safe from any thread; hs_queue_wait blocks outside the queue's lock; several
 *   queues on one index are allowed.
 * Answers.  Each query's outputs are bit for bit what hs_search_batch (with a filter set: hs_search_batch_filter_set) writes for
 *   that query -- labels, distances, counts, the padding of unused slots and all four stats columns -- whatever else shared its
 *   launch.  Required and nullable outputs follow hs_search_batch for the queue's mode (the other mode's label array is ignored).
 * Host submissions may be pageable: the queries are copied at submit into page-locked memory of the queue (the caller's query
 *   buffer is free when submit returns) and the results are copied into the caller's buffers by hs_queue_wait.  Queries in
 *   page-locked, device-mapped memory (hs_host_alloc, hipHostMalloc, mapped hipHostRegister) are NOT copied: the gather reads
 *   them in place, so they must stay unchanged until the ticket's wait returns (as for hs_search_batch_async; measured faster
 *   than staging at 1250- and at 10 000-query submissions).
 * Device submissions: submit records an event on the caller's `stream` and the queue's launch waits for it; the outputs are valid
 *   after hs_queue_wait, or on `stream` after hs_queue_join_stream (which does not release the ticket: its wait, or a drain, does).
 * Errors belong to a launch.  Whoever first completes a launch runs the capacity check of its stream (what hs_search_check does)
 *   and every ticket of that launch then returns that status -- so a device filter index outside the set gives HS_ERR_INVALID to
 *   every ticket of its launch, count 0 for the offending query, and the next launch is clean.  A launch that could not be planned
 *   or enqueued completes all its tickets with the error; nothing ever waits forever.  A ticket is waited once: a second wait, or
 *   an unknown ticket, is HS_ERR_INVALID.
 *   hs_queue_drain releases a ticket only once its launch is complete: an hs_queue_wait from another thread that races a drain
 *   either takes the ticket and returns its launch's status, or finds it released -- HS_ERR_INVALID -- with its outputs already written.
 * Refused at create (HS_ERR_INVALID): a SlimQ index, HS_MODE_SLIM_IDS on a vanilla index, k == 0, max_queries or slots out of
 *   range, a filter set with a mode other than HS_MODE_PQ, a filter set of another index size or device.
 * Index changes (patch, add, upsert, mark, resize, row format) while tickets are outstanding are the caller's to avoid: drain
 *   first, as for every asynchronous entry; hs_index_free with a live queue is likewise the caller's error.  hs_info.device_bytes
 *   of the index is not changed by a queue; the queue reports its own in hs_queue_info. */
typedef struct hs_queue hs_queue;
struct hs_queue_info {
  uint64_t submitted;       /* queries taken by submit so far */
  uint64_t launches;        /* launch groups enqueued so far */
  uint64_t pending;         /* queries submitted and not yet part of a launch */
  uint64_t in_flight;       /* launches enqueued and not yet completed */
  uint64_t largest_launch;  /* queries of the largest launch so far */
  uint64_t device_bytes;    /* HBM held by the queue (the launch arrays of its slots) */
};
hs_status hs_queue_create(hs_index *ix, size_t k, int mode, size_t max_queries, int slots, const hs_filter_set *fs /* nullable */,
                          hs_queue **out);
void hs_queue_free(hs_queue *q);   /* drains first */
hs_status hs_queue_submit(hs_queue *q, const float *queries, size_t nq, const uint32_t *filter_of_query, uint32_t *out_labels32,
                          uint64_t *out_labels64, float *out_dists, uint32_t *out_counts, uint32_t *stats, uint64_t *ticket);
hs_status hs_queue_submit_dev(hs_queue *q, const float *d_queries, size_t nq, const uint32_t *d_filter_of_query,
                              uint32_t *d_out_labels32, uint64_t *d_out_labels64, float *d_out_dists, uint32_t *d_out_counts,
                              uint32_t *d_stats, void *stream, uint64_t *ticket);
hs_status hs_queue_flush(hs_queue *q);                  /* enqueue one launch group for everything pending; does not block on it */
hs_status hs_queue_wait(hs_queue *q, uint64_t ticket);  /* flushes if the ticket is still pending; blocks until its results are in
                                                           the caller's buffers */
hs_status hs_queue_join_stream(hs_queue *q, uint64_t ticket, void *stream);   /* device tickets: `stream` waits, the host does not */
hs_status hs_queue_drain(hs_queue *q);                  /* flush + complete everything, release every ticket; the first error met */
hs_status hs_queue_info(const hs_queue *q, struct hs_queue_info *out);

/* ---- multi-GPU (no counterpart in the reference, which has no notion of a device) --------------------
 * Queries are independent and the index is read-only during search: the index is REPLICATED (hs_index_load once per
 * device), a batch is split into contiguous shards [r*S, (r+1)*S), S = ceil(nq/n), device r searches shard r, and one
 * RCCL all-gather of the packed [S x k] results over xGMI leaves the whole [nq x k] result on every device and on the
 * host.  One process, one stream per device; parity = the single-device result, bit for bit.
 * hs_comm_init: devices = n_gpus HIP device ordinals (NULL: 0..n-1).  Listing one device more than once is the
 * one-GPU rehearsal mode (the exchange then runs as device copies instead of RCCL, which refuses duplicate devices).
 * With more than one real device the first exchange happens here: a 64-byte all-gather per device, verified on every device
 * (HS_ERR_DEVICE if RCCL, its datatype constants or a link are not what the search will rely on). */
typedef struct hs_comm hs_comm;
hs_status hs_comm_init(int n_gpus, const int *devices, hs_comm **out);
void hs_comm_free(hs_comm *c);
int hs_comm_size(const hs_comm *c);
/* ixs: n_gpus replicas, ixs[r] loaded on the communicator's r-th device; queries and outputs are host pointers (outputs
 * as for hs_search_batch; out_dists / out_counts nullable in HS_MODE_SLIM_IDS).  Synchronous. */
hs_status hs_search_batch_sharded(hs_comm *c, hs_index *const *ixs, const float *queries, size_t nq, size_t k, int mode,
                                  uint32_t *out_labels32, uint64_t *out_labels64, float *out_dists, uint32_t *out_counts);
/* The same in two halves, for callers that keep several batches in flight per device (a split batch is a small launch on every
 * device and lasts as long as its longest query; the chip fills up with several of them): hs_search_batch_sharded_async only
 * ENQUEUES the step (H2D of the shards, search, all-gather, D2H of device 0's copy) on the streams of `slot`
 * (0 <= slot < hs_comm_slots()); hs_comm_check(slot) waits for it and reports capacity errors.  queries and outputs must stay
 * valid (page-locked if the copies are to overlap) until then; a slot holds one batch at a time. */
int hs_comm_slots(const hs_comm *c);
hs_status hs_search_batch_sharded_async(hs_comm *c, hs_index *const *ixs, const float *queries, size_t nq, size_t k, int mode,
                                        uint32_t *out_labels32, uint64_t *out_labels64, float *out_dists, uint32_t *out_counts, int slot);
hs_status hs_comm_check(hs_comm *c, hs_index *const *ixs, int slot);
/* device `rank`'s copy of the gathered arrays of the last hs_search_batch_sharded call ([n_gpus * S x k]; valid until the next call) */
hs_status hs_comm_results_dev(hs_comm *c, int rank, const uint32_t **d_labels32, const uint64_t **d_labels64,
                              const float **d_dists, const uint32_t **d_counts);

/* Parity/debug entry: raw top_candidates arrays after the level-0 beam, exactly as the reference holds
 * them before selection (hnswalg_slim.h:2116-2124): raw_dists/raw_ids are nq x max(ef,k), raw_sizes nq.
 * mark_ep_visited selects the (q,k)/(q,k,filter) overloads' extra visited tag (hnswalg_slim.h:1796,1919). */
hs_status hs_search_batch_raw(hs_index *ix, const float *queries, size_t nq, size_t k, int mode,
                              float *raw_dists, uint32_t *raw_ids, uint32_t *raw_sizes, uint32_t *stats);

/* ---- HNSW-SlimQ: HierarchicalNSWSlimQ (hnswalg_slimq.h), the RaBitQ-quantised variant --------------------------
 * hs_index_load(path, HS_KIND_SLIMQ, ..) parses saveIndex's format (hnswalg_slimq.h:1161-1313).  The search is
 * searchKnn(query, k, tableint *result) (hnswalg_slimq.h:1810-1924): greedy descent and a SearchBuffer beam of
 * capacity ef (hs_set_ef = setEf, :346-349) on ESTIMATED distances, every expanded node re-ranked with its exact
 * distance to the raw row of setDataset() and kept in a k-bounded max-heap.  out_labels/out_dists are nq x k in the
 * order the reference reads them out (the heap ARRAY, :1921-1923), ~0 / +inf beyond out_counts[q] entries (the
 * reference leaves those slots undefined).  stats: nq x 4 {expansions, estimates, buffer inserts, revisits}.
 * Float reductions that the reference runs through Eigen (alignment/width dependent order) are defined as
 * left-to-right fp32 sums; see DESIGN.md "SlimQ". */
hs_status hs_slimq_set_dataset(hs_index *ix, const float *base, size_t n, size_t dim);   /* setDataset, :303-305 */
/* t_const of quant::faster_config (the reference draws it from std::random_device at load time, :1274-1276;
 * default here: hs_rabitq_default_tconst(padded_dim, 1)). */
hs_status hs_slimq_set_tconst(hs_index *ix, double t_const);
double hs_slimq_get_tconst(const hs_index *ix);
hs_status hs_slimq_search_batch(hs_index *ix, const float *queries, size_t nq, size_t k, uint64_t *out_labels,
                                float *out_dists, uint32_t *out_counts, uint32_t *stats);
/* device pointers + HIP stream; asynchronous, hs_search_check(ix, stream) reports capacity problems */
hs_status hs_slimq_search_batch_dev(hs_index *ix, const float *d_queries, size_t nq, size_t k, uint64_t *d_out_labels,
                                    float *d_out_dists, uint32_t *d_out_counts, uint32_t *d_stats, void *stream);

/* Parity/debug entry: the query preparation as the kernel computed it; out is nq x (padded + 3 + num_cluster +
 * padded/8) floats: rotated query, {delta, vl, k1xsumq}, g_add per cluster, the 4 bit planes per 64-dim block as raw
 * u32 pairs (rotator.hpp:370-423, query.hpp:112-156, hnswalg_slimq.h:1822-1848). */
hs_status hs_slimq_prepare_debug(hs_index *ix, const float *queries, size_t nq, float *out);
/* Parity/debug entry: the SearchBuffer events of every query in order, two words each (out_trace nq x trace_cap,
 * 0xFFFFFFFF padding): a pop = {node id (bit 31 set when the node had been expanded before, hnswalg_slimq.h:696-704),
 * buffer size}, an insert = {candidate id | 1<<30, bits of its estimated distance} (:745). */
hs_status hs_slimq_trace(hs_index *ix, const float *queries, size_t nq, size_t k, uint32_t *out_trace, size_t trace_cap,
                         uint32_t *stats);

/* ---- exhaustive k-NN (ground truth): hnswlib::BruteforceSearch::searchKnn, bruteforce.h:106-135, for a batch ------
 * Result per query: the k lexicographically smallest (dist, label) pairs -- what the reference's priority_queue of
 * pairs ends up holding whatever the scan order -- sorted ascending; distances by the same fp32 recipes as the
 * graph search.  labels NULL = row index.  dim <= 4096 (dim % 16 == 0 is the tuned kernel), k <= 64.  out_counts[q] = min(k, n).
 * Value range: rows and queries must be finite.  Every finite distance is the reference's, and so is an L2 distance that overflows
 * to +inf: the reference keeps such a pair like any other (`inf <= inf`, bruteforce.h:120), so it is counted and returned, ordered
 * by label among the +inf entries; a returned +inf with a label other than ~0 is an answer, the padding beyond out_counts[q] has
 * label ~0.  Inner-product distances that overflow (non-finite or NaN) are outside the contract. */
hs_status hs_brute_force(const float *base, size_t n, size_t dim, int metric, const uint64_t *labels, const float *queries,
                         size_t nq, size_t k, int device, uint64_t *out_labels, float *out_dists, uint32_t *out_counts);
/* device pointers; synchronises `stream` before returning */
hs_status hs_brute_force_dev(const float *d_base, const uint64_t *d_labels, size_t n, size_t dim, int metric,
                             const float *d_queries, size_t nq, size_t k, uint64_t *d_out_labels, float *d_out_dists,
                             uint32_t *d_out_counts, void *stream);

/* ---- exact k-NN over the rows a resident index already holds ---------------------------------------------------------
 * The exhaustive scan above over the index's own rows, in the format it holds them: fp32, or its u8 / fp16 narrow copy
 * (hs_index_set_row_format; an index that holds both scans the narrow one -- fewer bytes, the same bits -- and an fp32-free
 * index, hs_index_set_f32_resident(ix, 0) / hs_index_load_narrow, its only one).  No second copy of the rows is uploaded.
 * Candidates of query i: the internal ids j < n that are not marked deleted and, when a filter set is named, whose bit is set in
 * row filter_of_query[i] of `fs` (the exclusion rule of hs_search_batch_filter_set).  Result: the min(k, #candidates)
 * lexicographically smallest (dist, label) pairs, ascending; dist by the index's metric with the fp32 recipes of every other
 * path, label the external label.  out_labels64 / out_dists nq x k, ~0 / +inf beyond out_counts[q] (nullable).
 * Without a filter, on an index without delete marks, this is BruteforceSearch::searchKnn (bruteforce.h:106-135) over the index's
 * (row, label) pairs bit for bit, L2 distances that overflow to +inf included (the value range of hs_brute_force).  With a filter it is deliberately NOT the reference's filtered overload: that code takes
 * `lastdist` from a queue that may hold fewer than k entries (bruteforce.h:118-131) and then drops nearer allowed rows depending on
 * the scan order; the answer here is the exact one and does not depend on the order of the rows.
 * fs NULL iff filter_of_query NULL.  HS_ERR_INVALID before anything is launched: null arguments, fs without filter_of_query or the
 * reverse, a set of another n or another device, a (host) filter index >= nf.  HS_ERR_UNSUPPORTED: k == 0 or k > 64, dim > 4096 (or
 * a query tile beyond the on-chip memory: dim 4096 with k above 63), a SlimQ index (its rows are RaBitQ records).  nq == 0: HS_OK.
 * hs_set_ef, hs_set_exact_order and hs_set_capacity do not apply: nothing here is approximate, ordered by a heap or bounded by a
 * scratch capacity.  hs_last_kernel: hs::exact_scan_kernel, hs::exact_scan_kernel_u8 or hs::exact_scan_kernel_f16
 * (hs::exact_scan_general_kernel for dim % 16 != 0, fp32 rows, one lane per row).
 * The host entry groups the queries by filter (a stable sort of filter_of_query) before it forms tiles of 8: a tile skips every
 * 32-row unit that none of its filters allows, so a selective filter costs about the rows it allows. */
hs_status hs_index_exact_search(hs_index *ix, const hs_filter_set *fs, const float *queries, size_t nq, size_t k,
                                const uint32_t *filter_of_query, uint64_t *out_labels64, float *out_dists, uint32_t *out_counts);
/* device pointers + HIP stream; asynchronous (the workspace is cached per index and stream): pair with hs_search_check(ix, stream).
 * A device filter index >= nf cannot be refused up front: that query gets count 0 and padding outputs and the check returns
 * HS_ERR_INVALID, as for hs_search_batch_filter_set_dev.  Tiles are formed in the order given: callers who want the skip group
 * their queries by filter. */
hs_status hs_index_exact_search_dev(hs_index *ix, const hs_filter_set *fs, const float *d_queries, size_t nq, size_t k,
                                    const uint32_t *d_filter_of_query, uint64_t *d_out_labels64, float *d_out_dists,
                                    uint32_t *d_out_counts, void *stream);

/* ---- harness (CPU, not accelerated): produce index files in the reference's formats ------------ */
/* HierarchicalNSW ctor + addPoint loop + saveIndex: hnswalg.h:85-159, 1248-1376, 748-779.
 * labels = row index; threads==1 reproduces the reference's serial build byte for byte. */
hs_status hs_build_hnsw(const float *base, size_t n, size_t dim, int metric, size_t M, size_t ef_construction,
                        const char *branching_factor, size_t seed, int threads, const char *out_path);
/* same with external labels: row i is added as addPoint(base + i*dim, labels[i]) (labels must be distinct) */
hs_status hs_build_hnsw_labeled(const float *base, const uint64_t *labels, size_t n, size_t dim, int metric, size_t M,
                                size_t ef_construction, const char *branching_factor, size_t seed, int threads,
                                const char *out_path);
/* Batched addPoint: the same index file from an insertion order that is parallel and still deterministic.  Points
 * enter in id order, in batches; every point of a batch runs the search half of addPoint against the graph as it stood when the
 * batch began, and the writes (mutuallyConnectNewElement) are applied in ascending id.  The next batch holds
 * min(batch_max, max(1, inserted / grow_div), n - inserted) rows and is cut right after the first row whose level exceeds the top
 * level so far.  batch_max == 1 is the reference's serial order: the bytes of hs_build_hnsw(threads = 1).  Any other schedule
 * writes a graph of its own that does not depend on `threads`, on timing, or on where it was built.
 * device >= 0: the searches, the heuristic and the reverse links run on that HIP device (build_gpu.hip) and write the bytes of the
 * host twin (device == -1, `threads` workers for the searches).  Shapes outside the device path -- M > 31, ef_construction > 512,
 * a row that does not fit the on-chip memory -- build on the host twin with used_gpu = 0.  scratch_ids: the ids one row's visited
 * set may hold on chip (a power of two from 64 to 8192; its candidate heap holds half as many); a row that outgrows it is flagged and searched again with its
 * scratch in device memory, never answered wrong.  In the options 0 means the default (grow_div 16, batch_max 16384,
 * scratch_ids 4096). */
typedef struct hs_batch_build_opts {
  int32_t device;       /* -1: the host twin */
  int32_t threads;      /* host workers (< 1: one) */
  uint64_t grow_div, batch_max, scratch_ids;
} hs_batch_build_opts;
typedef struct hs_batch_build_stats {
  int32_t used_gpu;
  uint32_t reserved;
  uint64_t batches, flagged_rows;
  double kernel_ms;     /* device time from the first kernel to the last (0 on the host twin) */
  double total_ms;      /* wall time of the call, the file write included */
} hs_batch_build_stats;
hs_status hs_build_hnsw_batched(const float *base, const uint64_t *labels /* nullable: the row index */, size_t n, size_t dim, int metric,
                                size_t M, size_t ef_construction, const char *branching_factor, size_t seed,
                                const hs_batch_build_opts *opts, const char *out_path, hs_batch_build_stats *stats /* nullable */);
/* Host only.  The schedule hs_build_hnsw_batched follows for these parameters: *n_batches batches, and for batch b < cap its size
 * (sizes[b]) and the entry point (0xFFFFFFFF: none yet) and top level (-1) before it (entry_points[b], top_levels[b]); the three
 * arrays are nullable and hold `cap` entries. */
hs_status hs_build_schedule(size_t n, size_t M, const char *branching_factor, size_t seed, size_t grow_div, size_t batch_max, size_t cap,
                            uint32_t *sizes, uint32_t *entry_points, int32_t *top_levels, size_t *n_batches);
/* Host only, no device: loadIndex(in_path, space, max_elements), level generator seeded with `seed` and `drawn` draws discarded
 * (hs_index_seed_levels), addPoint(rows + i*dim, labels[i]) for i < count, saveIndex(out_path).  threads == 1 is the reference's
 * serial order: resuming the first n0 rows' build with the remaining rows writes the bytes of the one-shot build.  Refusals as
 * hs_index_add_points (capacity, existing or repeated label), before anything is added; out_path is then not written. */
hs_status hs_hnsw_resume(const char *in_path, int metric, size_t dim, size_t max_elements, const float *rows,
                         const uint64_t *labels, size_t count, size_t seed, size_t drawn, int threads, const char *out_path);
/* Batched addPoint into a resident vanilla index: hs_index_add_points in the order of hs_build_hnsw_batched, continued
 * from the graph the index holds -- fast and still deterministic.  Row i becomes internal id n + i with a level from the index's level
 * generator (hs_index_seed_levels works as for hs_index_add_points); the schedule is hs_build_hnsw_batched's rule started at
 * inserted = n with the index's entry point and top level, so a build split at a batch boundary of hs_build_schedule -- the prefix
 * built, loaded with room, seeded with (seed, prefix), the rest added here -- holds the bytes of the whole build, and batch_max == 1 is
 * hs_index_add_points(threads = 1).  M, ef_construction and the level multiplier are the file header's.
 * opts->device: -1 (the host twin: the searches on `threads` workers over the host image) or the index's own device (anything else:
 * HS_ERR_INVALID).  On the device the new rows are copied behind the resident fp32 rows (nothing is uploaded twice), the lists are
 * seeded from the host image, the insertion searches and reverse links run there (build_gpu.hip), and only the lists that changed and
 * the new nodes' lists are downloaded (one dense buffer); the host image is updated from them and the device arrays through the same
 * write path as hs_index_add_points (tiles re-tiled when a list outgrows the stride, small structure arrays rebuilt, a filter set made
 * for the old n refused afterwards).  Both paths leave the same bytes for hs_index_save.  Shapes outside the device build (M > 31,
 * ef_construction > 512, a row that does not fit the on-chip memory), an index without resident fp32 rows, and an empty index run the
 * host twin with used_gpu = 0.  Refusals, all before anything changes: those of hs_index_add_points, and HS_ERR_UNSUPPORTED for an
 * index that holds delete marks (the batched insertion has no deleted-element branches; hs_index_add_points takes such an index). */
hs_status hs_index_add_points_batched(hs_index *ix, const float *rows, const uint64_t *labels, size_t count,
                                      const hs_batch_build_opts *opts, hs_batch_build_stats *stats /* nullable */);
/* Diagnostic: what the device path of the last hs_index_add_points_batched brought back beside the new nodes: *lists_downloaded
 * (nullable) old lists that received an id, and the old nodes (internal ids below the element count before the call, ascending)
 * among them whose level-0 or upper list bytes changed -- a full list whose re-prune turns the new id away and keeps its order
 * comes back as it was.  Both empty after a call the host twin served.  ids nullable, at most cap written. */
hs_status hs_debug_batched_add_changed(const hs_index *ix, uint32_t *ids, size_t cap, size_t *count, size_t *lists_downloaded);
/* Host only, no device: hs_hnsw_resume with the rows added in the batched order above, always on the host twin (opts->device is not
 * used; used_gpu = 0) -- what hs_index_add_points_batched leaves for hs_index_save.  Refusals as that call (capacity, existing or
 * repeated label, delete marks), before anything is added; out_path is then not written. */
hs_status hs_hnsw_resume_batched(const char *in_path, int metric, size_t dim, size_t max_elements, const float *rows,
                                 const uint64_t *labels, size_t count, size_t seed, size_t drawn, const hs_batch_build_opts *opts,
                                 const char *out_path, hs_batch_build_stats *stats /* nullable */);
/* Host only, no device: loadIndex(in_path, space, max_elements) with the constructor's allow_replace_deleted, then `n_ops`
 * operations in order, then saveIndex(out_path).  An operation is four 64-bit words {kind, label or new capacity, replace flag,
 * row index into `rows`}: HS_OP_ADD = addPoint(rows + row*dim, label, flag) (update, replacement or append as the reference decides),
 * HS_OP_MARK / HS_OP_UNMARK = markDelete / unmarkDelete(label), HS_OP_RESIZE = resizeIndex(new capacity).  The reference's
 * refusals come back with the statuses of hs_index_upsert_points / hs_index_mark_deleted / hs_index_resize; out_path is then
 * not written. */
enum { HS_OP_ADD = 0, HS_OP_MARK = 1, HS_OP_UNMARK = 2, HS_OP_RESIZE = 3 };
hs_status hs_hnsw_replay(const char *in_path, int metric, size_t dim, size_t max_elements, int allow_replace_deleted,
                         const uint64_t *ops, size_t n_ops, const float *rows, const char *out_path);
/* HierarchicalNSWSlim::convertFromHNSW + saveIndex: hnswalg_slim.h:867-1108, 717-751. */
hs_status hs_convert_slim(const char *hnsw_path, int metric, size_t dim, int threshold_level,
                          float top_degree_percent0, float top_degree_percent, size_t top_degree_M0,
                          size_t low_degree_m0, size_t top_degree_M, size_t low_degree_m, int threads,
                          const char *out_path);
/* The same conversion with the per-list work on HIP device `device` (per-node distances, the by-distance
 * std::sort with libstdc++'s tie order, PruneByHeuristic :836-865, the reverse-edge union :988-1012, the re-prune
 * :1038-1062); histograms, hub thresholds and the final assembly run on `threads` host threads.  The file is byte-identical
 * to hs_convert_slim's.  Shapes outside the device path (degree capacities or budgets above 64 -- a graph built with M > 32 --, a source
 * list above 64 ids, a reverse-edge union beyond 2048 ids)
 * are converted on the CPU; *used_gpu (nullable) says which path ran, *kernel_ms (nullable) the device time. */
hs_status hs_convert_slim_gpu(const char *hnsw_path, int metric, size_t dim, int threshold_level,
                              float top_degree_percent0, float top_degree_percent, size_t top_degree_M0,
                              size_t low_degree_m0, size_t top_degree_M, size_t low_degree_m, int device, int threads,
                              const char *out_path, int *used_gpu, double *kernel_ms);

/* ---- the patch server: convertFromHNSWWithDiff (hnswalg_slim.h:1110-1424, 1478-1751) and genPatch (:1427-1476) -------------
 * The server of the reference's update experiment (hnsw_slim_server_patch.cc:204-296) keeps a vanilla index growing, re-derives
 * its Slim index after every batch and ships the difference; its clients apply it with patchFromStream (hs_index_patch).
 *
 * hs_slim_convert_diff: `slim` is a HS_KIND_SLIM index and `hnsw` a HS_KIND_HNSW index, both loaded with max_elements > their
 * element count (so both hold a host image), of the same metric, dim, maxM and maxM0.  The call re-derives `slim` from `hnsw` --
 * both prunes are hnsw->getNeighborsByHeuristic2 (hnswalg.h:481-523), not PruneByHeuristic -- updates slim's host image and its
 * device arrays in place (one staged upload and one kernel for the changed nodes; count, maxlevel, enterpoint and has_deleted
 * follow `hnsw`, :1113-1118) and returns the changed nodes as a diff object.  slim keeps its own threshold_level.
 * The list passes run on the device when both indexes are on the same device, hnsw holds resident fp32 rows, every degree
 * capacity and budget is at most 32, no source list exceeds 64 ids and no union 2048; otherwise on `threads` host threads with
 * the same bytes.  *used_gpu (nullable) says which, *kernel_ms (nullable) the time from the first
 * kernel to the last -- list, diff and compaction kernels -- which includes the host round trips between them.  On the device path a
 * diff kernel compares the new lists with slim's resident adjacency, rows and labels and compacts the changed ids; the host
 * assembles elements and blobs of the flagged nodes only, and their rows are copied from hnsw's resident array.
 * Where the reference is undefined or timing-dependent this library decides: a re-pruned list holds exactly
 * the entries the heuristic kept, in pop order; the two changed lists are in ascending id; elements beyond the previous count
 * start empty.  A node whose lists come out empty is in neither list (:1340-1343).  Delete marks do not reach Slim elements.
 * Refused before anything changes: HS_ERR_INVALID (null argument, wrong kinds, an index without a host image, metric / dim /
 * capacities that differ, hnsw holding fewer elements than slim), HS_ERR_CAPACITY when hnsw's element count exceeds slim's
 * max_elements (the reference reallocs here; load slim with more room), HS_ERR_UNSUPPORTED when slim has narrow rows and a new
 * row is not representable.  Not while a search on either index is in flight.
 * A failure after these checks (HS_ERR_NOMEM, HS_ERR_DEVICE while the changed nodes are written) is not rolled back: slim's host
 * image is then ahead of its device arrays and the index must be freed and loaded again.
 * A diff object serves until the next hs_slim_convert_diff on the same index; after it the hs_slim_diff_* calls that need the
 * index refuse the older object (HS_ERR_INVALID). */
typedef struct hs_slim_diff hs_slim_diff;
hs_status hs_slim_convert_diff(hs_index *slim, hs_index *hnsw, float top_degree_percent0, float top_degree_percent,
                               size_t top_degree_M0, size_t low_degree_m0, size_t top_degree_M, size_t low_degree_m, int threads,
                               hs_slim_diff **out, int *used_gpu, double *kernel_ms);
/* cur_element_count and the lengths of the two changed lists; n_reprune (nullable): lists that went through the re-prune. */
hs_status hs_slim_diff_info(const hs_slim_diff *d, size_t *count, size_t *n_old, size_t *n_new, size_t *n_reprune);
/* The changed old nodes and the new nodes, ascending (n_old / n_new ids; either pointer may be NULL). */
hs_status hs_slim_diff_ids(const hs_slim_diff *d, uint32_t *old_ids, uint32_t *new_ids);
/* The whole stream of the std::ostream overload (:1384-1422): u64 count, u64 n_old, u64 n_new, the old records (8-byte head),
 * the new records (16-byte head, no rows) -- what hs_index_patch(.., to_add = 0) takes.  `slim` is the index the diff was made
 * on (NULL for a diff of hs_slim_convert_diff_files).  *len receives the size; HS_ERR_CAPACITY when cap is smaller (buf may be
 * NULL with cap 0 to ask). */
hs_status hs_slim_diff_stream(const hs_slim_diff *d, const hs_index *slim, void *buf, size_t cap, size_t *len);
/* One genPatch call (:1427-1476) with the cursors kept in the diff object: records until their sizes reach `limit` bytes, new
 * records with their row when to_add.  Written as the 24-byte header hs_index_patch expects, {u64 count, u64 old_written, u64
 * new_written} of THIS call, then genPatch's record bytes.  As in the reference the record that reaches `limit` is written and
 * its cursor is not advanced, so the next call sends that node again.  *finished = genPatch's return value.  HS_ERR_CAPACITY
 * with the needed *len when cap is too small; the cursors then do not move. */
hs_status hs_slim_diff_next(hs_slim_diff *d, const hs_index *slim, size_t limit, int to_add, void *buf, size_t cap, size_t *len,
                            size_t *old_written, size_t *new_written, int *finished);
void hs_slim_diff_free(hs_slim_diff *d);
/* saveIndex (hnswalg_slim.h:717-751) of the host image of a Slim index loaded with max_elements > its element count, as
 * hs_slim_convert_diff and hs_index_patch left it.  HS_ERR_INVALID for any other index (hs_index_save is the vanilla twin). */
hs_status hs_slim_index_save(const hs_index *slim, const char *path);
/* Host only, no device: the same call on files.  old_slim_path NULL: an empty Slim index with `threshold_level` and the HNSW
 * file's capacities (every node with neighbours is then new); otherwise the Slim file's own threshold_level is kept.  Writes the
 * new Slim file (saveIndex, :717-751) to out_slim_path and, when out_stream_path is given, the whole stream; *out (nullable)
 * receives a diff object that owns its Slim image (pass slim = NULL to hs_slim_diff_stream / hs_slim_diff_next). */
hs_status hs_slim_convert_diff_files(const char *old_slim_path, const char *hnsw_path, int metric, size_t dim, int threshold_level,
                                     float top_degree_percent0, float top_degree_percent, size_t top_degree_M0,
                                     size_t low_degree_m0, size_t top_degree_M, size_t low_degree_m, int threads,
                                     const char *out_slim_path, const char *out_stream_path, hs_slim_diff **out);

/* The graph HNSW-SlimQ is converted FROM: rabitqlib::hnsw::HierarchicalNSW(num_points, dim, total_bits, M, ef_construction,
 * random_seed, metric) + construct() (third_party/rabitqlib/index/hnsw/hnsw.hpp:427-500, 667-1054), as
 * include/strategy/hnsw_slimq_strategy.h:106-121 drives it with M = 32, ef_construction = 128, seed 100.  Edges come from the RAW
 * rows (hnsw.hpp:381-387) in Eigen's inner-product order; heaps order (distance, id) pairs; mult = 1 / ln M.  Only the edges are
 * built here (the RaBitQ records are hs_convert_slimq's job); the file is hnswlib's saveIndex layout (hnswalg.h:748-779), labels ==
 * row index == internal id.  threads == 1 reproduces the reference's serial construct() edge for edge. */
hs_status hs_build_rabitq_hnsw(const float *base, size_t n, size_t dim, int metric, size_t M, size_t ef_construction,
                               size_t seed, int threads, const char *out_path);
/* The same graph from the batched insertion order of hs_build_hnsw_batched: the same schedule (levels from
 * std::default_random_engine(seed) with mult = 1 / ln M), phase A against the graph as the batch found it, the writes of
 * mutually_connect_new_element in ascending id -- with rabitqlib's rules: pair-ordered heaps, Eigen's packet inner product, no
 * second link to a node that already lists the new one.  batch_max == 1 is the serial construct(): the bytes of
 * hs_build_rabitq_hnsw(threads = 1).  Any other schedule writes a graph of its own that does not depend on `threads`, on timing or
 * on where it was built.  device >= 0 builds on that HIP device for M <= 32, max(ef_construction, M) <= 512 and a row that fits the
 * on-chip memory; anything else, and device == -1, builds on the host twin (used_gpu = 0), the same bytes.  Options and stats as
 * hs_build_hnsw_batched; refusals as hs_build_rabitq_hnsw.  Labels are the row index. */
hs_status hs_build_rabitq_hnsw_batched(const float *base, size_t n, size_t dim, int metric, size_t M, size_t ef_construction,
                                       size_t seed, const hs_batch_build_opts *opts, const char *out_path,
                                       hs_batch_build_stats *stats /* nullable */);
/* The distance of that builder alone, for tests: out[i] = raw distance of rows a[i] and b[i] (n_pairs x dim each, host arrays).
 * device == -1: the host recipe; otherwise the wavefront recipe of the build kernels on that HIP device (dim <= 8192).  The two
 * agree bit for bit wherever no NaN arises. */
hs_status hs_debug_rq_raw_dist(const float *a, const float *b, size_t n_pairs, size_t dim, int metric, int device, float *out);
/* HierarchicalNSWSlimQ::convertFromHNSW's graph passes (hnswalg_slimq.h:1546-1762): hs_convert_slim's passes with SlimQ's own
 * PruneByHeuristic as written (:1334-1362 -- the occlusion test reads the row whose id is the LOOP INDEX, :1349) and rabitqlib's
 * raw distance (:1623, :1706).  Writes a Slim-layout file; feed it to hs_convert_slimq for the quantised index. */
hs_status hs_convert_slimq_graph(const char *hnsw_path, int metric, size_t dim, int threshold_level,
                                 float top_degree_percent0, float top_degree_percent, size_t top_degree_M0,
                                 size_t low_degree_m0, size_t top_degree_M, size_t low_degree_m, int threads,
                                 const char *out_path);

/* HierarchicalNSWSlimQ::convertFromHNSW's OUTPUT format + saveIndex (hnswalg_slimq.h:1471-1790, 1161-1216): keeps
 * the graph of an existing HierarchicalNSWSlim file and replaces the fp32 rows by RaBitQ records (cluster id,
 * 1-bit code, {f_add, f_rescale, f_error}); the ex-bits area is zero (no function on the search path reads it).
 * centroids: num_cluster x dim raw vectors; cluster_ids: n ids or NULL (= nearest centroid). */
hs_status hs_convert_slimq(const char *slim_path, int metric, size_t dim, const float *centroids, size_t num_cluster,
                           const uint32_t *cluster_ids, uint64_t flip_seed, int threads, const char *out_path);
/* ---- HierarchicalNSWSlimQ::convertFromHNSW on a HIP device (csrc/convert_slimq.hip) -----------------------------
 * hs_convert_slimq_graph with the list-level work on `device`: raw distances, the by-distance std::sort, SlimQ's PruneByHeuristic,
 * the reverse-edge union and the re-prune; histograms, hub thresholds and the assembly run on `threads` host threads.  The file is
 * byte-identical to hs_convert_slimq_graph's.  Shapes outside the device path (hs_convert_slim_gpu's: capacities or budgets above
 * 64, a source list above 64 ids, a union beyond 2048; and a row that does not fit the kernels' on-chip memory, dim > 8112) are
 * converted on the host; *used_gpu (nullable) says which path ran, *kernel_ms (nullable) the device time. */
hs_status hs_convert_slimq_graph_gpu(const char *hnsw_path, int metric, size_t dim, int threshold_level,
                                     float top_degree_percent0, float top_degree_percent, size_t top_degree_M0,
                                     size_t low_degree_m0, size_t top_degree_M, size_t low_degree_m, int device, int threads,
                                     const char *out_path, int *used_gpu, double *kernel_ms);
/* hs_convert_slimq with the rotation and the 1-bit quantisation of every row on `device`, one wavefront per row; rows are uploaded
 * 256 MiB at a time.  The file is byte-identical to hs_convert_slimq's; refusals as hs_convert_slimq, and HS_ERR_DEVICE without
 * such a device.  *used_gpu / *kernel_ms (nullable) as above. */
hs_status hs_convert_slimq_gpu(const char *slim_path, int metric, size_t dim, const float *centroids, size_t num_cluster,
                               const uint32_t *cluster_ids, uint64_t flip_seed, int device, int threads, const char *out_path,
                               int *used_gpu, double *kernel_ms);
/* Both steps in one call, HNSW file in, SlimQ file out, with no intermediate file: the Slim graph stays in memory and feeds the
 * quantisation.  device == -1: both steps on `threads` host threads; device >= 0: both on that device, each falling back to the
 * host outside its envelope.  Either way the bytes of hs_convert_slimq_graph followed by hs_convert_slimq.  Refusals as those two. */
typedef struct hs_slimq_convert_stats {
  int graph_used_gpu, records_used_gpu;      /* which path each step took */
  double graph_kernel_ms, records_kernel_ms; /* device time of each step's kernels (0 on the host path) */
  double graph_ms, records_ms, total_ms;     /* wall clock: graph passes incl. loading the file; records; the whole call incl. the save */
} hs_slimq_convert_stats;
hs_status hs_convert_hnsw_to_slimq(const char *hnsw_path, int metric, size_t dim, int threshold_level,
                                   float top_degree_percent0, float top_degree_percent, size_t top_degree_M0,
                                   size_t low_degree_m0, size_t top_degree_M, size_t low_degree_m, const float *centroids,
                                   size_t num_cluster, const uint32_t *cluster_ids, uint64_t flip_seed, int device, int threads,
                                   const char *out_path, hs_slimq_convert_stats *stats /* nullable */);
/* The quantiser alone, on explicit flip bytes (4 * padded / 8), for tests: n rows (n x dim) against num_cluster raw centroids;
 * cluster_ids NULL = nearest raw centroid, first minimum.  device == -1: the host recipe; otherwise the kernels of
 * hs_convert_slimq_gpu on that device, bit for bit the same.  out_rotated (nullable): n x padded; out_cluster: n; out_codes:
 * n x padded / 64; out_factors: n x 3. */
hs_status hs_debug_rq_quantize_rows(size_t dim, int metric, const uint8_t *flips, const float *rows, size_t n,
                                    const float *centroids_raw, size_t num_cluster, const uint32_t *cluster_ids, int device,
                                    float *out_rotated, uint32_t *out_cluster, uint64_t *out_codes, float *out_factors);
/* quant::faster_config(padded, 4).t_const (rabitqlib/quantization/rabitq.hpp:27-33) with a seeded generator. */
double hs_rabitq_default_tconst(size_t padded_dim, uint64_t seed);

/* ---- RaBitQ pieces of the HNSW-SlimQ path (CPU; used by the SlimQ harness and query preparation, exposed
 *      so that tests can pin them against the compiled rabitqlib) ------------------------------------- */
/* FhtKacRotator::rotate: rabitqlib/utils/rotator.hpp:370-423.  flips = 4*padded/8 bytes, out = n x padded. */
hs_status hs_rabitq_rotate(size_t dim, const uint8_t *flips, const float *in, size_t n, float *out);
/* one_bit_compact_code<float,uint64_t>: rabitqlib/quantization/rabitq_impl.hpp:75-187.  codes n x padded/64,
 * factors n x {f_add, f_rescale, f_error}. */
hs_status hs_rabitq_quantize_data(size_t padded, int metric, const float *rotated, size_t n, const float *centroid,
                                  uint64_t *codes, float *factors);
/* SplitSingleQuery ctor: rabitqlib/index/query.hpp:112-156.  out3 n x {delta, vl, k1xsumq}; bins n x padded/64*4. */
hs_status hs_rabitq_prepare_query(size_t padded, double t_const, const float *rotated_q, size_t n, float *out3,
                                  uint64_t *bins);
/* split_single_estdist: rabitqlib/index/estimator.hpp:164-188.  out nq x nd x {ip_x0_qr, est_dist, low_dist}. */
hs_status hs_rabitq_estimate(size_t padded, const uint64_t *codes, const float *factors, size_t nd, const float *q3,
                             const uint64_t *bins, const float *g_add, const float *g_error, size_t nq, float *out);

/* ---- a resident SlimQ index from rows or a graph, with no file on the way ------------------------------------
 * hs_graph: an HNSW graph in host memory -- what saveIndex (hnswalg.h:748-779) would write.  hs_build_rabitq_hnsw_batched_mem is
 * hs_build_rabitq_hnsw_batched without its file (same options, refusals and stats; total_ms without a file write);
 * hs_graph_save writes the bytes that call writes; hs_graph_load reads any file of that layout. */
typedef struct hs_graph hs_graph;
hs_status hs_build_rabitq_hnsw_batched_mem(const float *base, size_t n, size_t dim, int metric, size_t M, size_t ef_construction,
                                           size_t seed, const hs_batch_build_opts *opts, hs_graph **out,
                                           hs_batch_build_stats *stats /* nullable */);
hs_status hs_graph_load(const char *path, int metric, size_t dim, hs_graph **out);
hs_status hs_graph_save(const hs_graph *g, const char *path);
/* every output nullable */
hs_status hs_graph_info(const hs_graph *g, uint64_t *n, uint64_t *dim, int *metric, uint64_t *M, uint64_t *ef_construction, int *maxlevel);
void hs_graph_free(hs_graph *g);

/* the arguments of hs_convert_hnsw_to_slimq between `dim` and `device` */
typedef struct hs_slimq_params {
  int threshold_level;
  float top_degree_percent0, top_degree_percent;
  size_t top_degree_M0, low_degree_m0, top_degree_M, low_degree_m;
  const float *centroids;        /* num_cluster x dim raw vectors */
  size_t num_cluster;
  const uint32_t *cluster_ids;   /* n ids or NULL (= nearest centroid) */
  uint64_t flip_seed;
} hs_slimq_params;
/* build + conversion + residency of one hs_slimq_index_from_rows call */
typedef struct hs_slimq_pipeline_stats {
  hs_batch_build_stats build;
  hs_slimq_convert_stats convert;
  double resident_ms;      /* packing, uploads and the tile kernels (and the dataset upload with with_dataset) */
  double tile_kernel_ms;   /* the three kernels of slimq_tiles.hip, first to last */
  double total_ms;
} hs_slimq_pipeline_stats;
/* convertFromHNSW of an in-memory graph.  convert_device: -1 = both steps on `threads` host threads, >= 0 = on that device with the
 * host fallbacks of hs_convert_hnsw_to_slimq.  out_path (nullable): the SlimQ file, byte for byte hs_convert_hnsw_to_slimq's.
 * out_index (nullable): a resident index on `index_device`, its fused tiles gathered on the device (slimq_tiles.hip); with_dataset
 * != 0 also makes the graph's own rows its re-rank dataset (row of internal id i, hnswalg_slimq.h:748), as hs_slimq_set_dataset
 * would.  At least one of the two outputs (HS_ERR_INVALID otherwise).  Refusals are those of hs_convert_hnsw_to_slimq and, with
 * out_index, of hs_index_load (HS_ERR_DEVICE without that device), all before any work: no file is then written.  stats
 * (nullable): total_ms includes whatever outputs were asked for. */
hs_status hs_graph_convert_slimq(const hs_graph *g, const hs_slimq_params *p, int convert_device, int threads, const char *out_path,
                                 int index_device, int with_dataset, hs_index **out_index, hs_slimq_convert_stats *stats);
/* rows in, resident index out: hs_build_rabitq_hnsw_batched_mem + hs_graph_convert_slimq in one call; the graph is freed inside.
 * The build runs on opts->device, the conversion too, and the index lives there (opts->device >= 0: HS_ERR_INVALID otherwise). */
hs_status hs_slimq_index_from_rows(const float *base, size_t n, size_t dim, int metric, size_t M, size_t ef_construction, size_t seed,
                                   const hs_batch_build_opts *opts, const hs_slimq_params *p, int threads, int with_dataset,
                                   hs_index **out_index, hs_slimq_pipeline_stats *stats /* nullable */);
/* saveIndex (hnswalg_slimq.h:1161-1216) of the host image every resident SlimQ index keeps (codes, factors, blobs, labels; no fp32
 * rows).  HS_ERR_INVALID for any other index. */
hs_status hs_slimq_index_save(const hs_index *ix, const char *path);
/* tests: which = 0 rec, 1 ftile, 2 uptile.  *words = the array's length (0: the index has no such array); copied out when
 * cap_words suffices (out may be NULL with cap_words 0 to ask).  stride / row_words (nullable): slots per row and words per slot
 * of it (rec: 1 and rec_words). */
hs_status hs_debug_slimq_arrays(const hs_index *ix, int which, uint32_t *out, size_t cap_words, size_t *words, uint32_t *stride,
                                uint32_t *row_words);
/* the same three arrays from a SlimQ file by the host functions of csrc/slimq_tiles.hpp alone: no device.  fused: what
 * HS_SLIMQ_FUSED would be. */
hs_status hs_debug_slimq_arrays_host(const char *slimq_path, int metric, size_t dim, int fused, int which, uint32_t *out, size_t cap_words,
                                     size_t *words, uint32_t *stride, uint32_t *row_words);

#ifdef __cplusplus
}
#endif
#endif /* HNSW_SLIM_AMD_H */
