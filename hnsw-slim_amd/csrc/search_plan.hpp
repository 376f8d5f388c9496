// search_plan.hpp -- which kernels serve a batch and with what scratch shares, as a pure function of the index's shape, the
// call and the diagnostic knobs.  Host only: no HIP runtime call, no hs_index; the structs are the plain C ones of
// include/hnsw_slim_amd.h (hs_debug_search_plan hands them through), so a plan can be made and tested without a device.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/hnsw_slim_amd.h"

#pragma GCC visibility push(hidden)   // shared between the library's own files, not exported
namespace hs {

// Every diagnostic knob of the C ABI.  diag_from_env() is the only place that reads the environment; diag() is that reading made
// once per process, at first use, and fixed afterwards.
using Diag = hs_plan_diag;
Diag diag_from_env();
const Diag &diag();

using PlanInput = hs_plan_in;
using SearchPlan = hs_plan_out;

static constexpr size_t kLdsPerCU = 160 * 1024;
// Last-resort pass (strict kernel): a few workgroups, each with a small visited hash in LDS and its candidate heap + a large
// tier-2 visited set in its own region of global memory (engine.hpp fb_cand / fb_spill): 24 MiB per stream, any query fits.
static constexpr uint32_t kFbGrid = 32, kFbCand = 32768, kFbSpill = 131072, kFbHash = 2048;
static constexpr uint32_t kLeanMinEf = 64;    // HS_KERNEL=lean: the lean kernel answers from this ef upwards (HS_LEAN_MIN_EF overrides), the fast kernel below
static constexpr uint32_t kSpillSlots = 8192;  // 32 KiB per query of tier-2 visited set
static constexpr uint32_t kCand2Cap = 4096;    // 32 KiB per query of tier-2 candidate heap
static constexpr uint32_t kLogCap = 4096;      // 32 KiB per query: result-set insertion log (tie replay)
static constexpr uint32_t kHopCap = 4096;      // 4 KiB per query: accepted neighbours per expansion (flat start of the fast kernel)
static constexpr uint32_t kParkWords = 2048;   // 8 KiB per query: where the flat kernel parks the head of its visited set during a heap replay
// from this many queries per launch the first pass runs as descent / order / level-0 search (see search_dev_group)
static constexpr size_t kOrderMinQueries = 6144;
// HS_ORDER (diagnostic): 0 = never split, 1 = always, unset = from kOrderMinQueries queries
inline bool split_launch(const Diag &d, size_t nq) { return d.order < 0 ? nq >= kOrderMinQueries : d.order != 0; }

// The name hs_last_kernel reports for a pass-0 kernel family (HS_PLAN_*) reading rows of format `rows` (HS_ROWS_*).
const char *kernel_name(int family, int rows);

// The launch plan of one launch group.  HS_OK, or the status to return with *msg (a string literal) as its text.
hs_status plan_search(const PlanInput &in, SearchPlan &out, const char **msg);

}  // namespace hs
#pragma GCC visibility pop
