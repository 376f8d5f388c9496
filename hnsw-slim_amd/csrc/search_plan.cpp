// search_plan.cpp -- the launch plan of a search batch (search_plan.hpp) and the diagnostic knobs.
#include "search_plan.hpp"

#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "engine.hpp"   // the kernels' own *_lds_bytes / *_supported / flatk_waves_per_cu (host functions of the .hip files)

namespace hs {

Diag diag_from_env() {
  Diag d{};
  const char *kernel = getenv("HS_KERNEL");
  d.kernel = kernel && !strcmp(kernel, "lean") ? HS_PLAN_KERNEL_LEAN : kernel && !strcmp(kernel, "fast") ? HS_PLAN_KERNEL_FAST : HS_PLAN_KERNEL_DEFAULT;
  const char *lean = getenv("HS_LEAN_MIN_EF");
  d.lean_forced = lean != nullptr;
  d.lean_min_ef = lean ? (uint32_t)atoi(lean) : kLeanMinEf;
  d.order = getenv("HS_ORDER") ? atoi(getenv("HS_ORDER")) : -1;               // 0 = never, 1 = always, 2 = the split without the ordering
  d.flat = !(getenv("HS_FLAT") && atoi(getenv("HS_FLAT")) == 0);              // 0: heap path from the first expansion
  d.vis16 = !(getenv("HS_VIS16") && atoi(getenv("HS_VIS16")) == 0);           // 0: the 32-bit form everywhere
  d.flat_waves_per_cu = getenv("HS_FLAT_WAVES_PER_CU") ? atoi(getenv("HS_FLAT_WAVES_PER_CU")) : 0;   // builds with another residency
  const char *zc = getenv("HS_ZERO_COPY");                                    // A/B knobs: "0" = staged, "in" = outputs staged
  d.zero_copy = zc && !strcmp(zc, "0") ? HS_PLAN_ZERO_COPY_OFF : zc && !strcmp(zc, "in") ? HS_PLAN_ZERO_COPY_IN : HS_PLAN_ZERO_COPY_ON;
  d.verbose = getenv("HS_VERBOSE") != nullptr;
  const char *fused = getenv("HS_SLIMQ_FUSED");
  d.slimq_fused = !(fused && fused[0] == '0');
  return d;
}
const Diag &diag() {
  static const Diag d = diag_from_env();
  return d;
}

const char *kernel_name(int family, int rows) {
  static const char *const names[4][3] = {
      {"hs::flat_kernel", "hs::flat_kernel_f16", "hs::flat_kernel_u8"},
      {"hs::lean_kernel", "hs::lean_kernel", "hs::lean_kernel"},   // (no narrow twin: never planned over narrow rows)
      {"hs::fast_kernel", "hs::fast_kernel_f16", "hs::fast_kernel_u8"},
      {"hs::strict_kernel", "hs::strict_kernel_f16", "hs::strict_kernel_u8"},
  };
  return names[family][rows];
}

// The fast kernel's shape table (engine.hpp FastShape): every (metric, dim) with a distance pass compiled for it, the runtime-dim
// shapes for the rest.  A line here and the `case` of the launcher that names the same d16 (beam_search.hip) come and go together:
// a d16 without its case is refused at launch, and tests/test_search_plan_cpu.py holds this table to the instantiations built.
FastShape fast_shape(int metric, uint32_t dim, uint32_t ef, uint32_t k, bool bare) {
  FastShape s{};
  s.d16 = (dim & 15u) ? -1 : 0;
  if (!bare) {   // delete marks / a filter set: the runtime-dim shapes and d = 128 (SIFT) for L2
    if (metric == HS_METRIC_L2 && dim == 128) s.d16 = 8;
  } else if (metric == HS_METRIC_L2) {
    switch (dim) {   // (the runtime-dim kernel is 1.15-1.7x slower: measured at d=64 and on DEEP-10M, d=96)
      case 64: case 96: case 128: case 256: case 512: case 768: case 960: case 1024: s.d16 = (int32_t)(dim / 16); break;   // 96: DEEP, 128: SIFT, 960: GIST
      // GloVe-100-like: the 4-lane recipes with the dim compiled in (the 25 steps unroll without spills; at 200 / 300 the
      // unrolled loads spill 80 / 250 B per lane, so those stay on the runtime-dim kernel)
      case 100: s.d16 = -25; break;
      default: break;
    }
  } else {
    switch (dim) {   // text / image embeddings
      case 512: case 768: case 1024: case 1536: s.d16 = (int32_t)(dim / 16); break;   // 768: COHERE
      case 100: s.d16 = -25; break;   // GloVe-100-angular-like, as for L2
      default: break;
    }
  }
  s.slots = ef <= 64 ? 1 : ef <= 128 ? 2 : ef <= 256 ? 4 : 8;
  s.wb = bare && k == ef;   // nothing is selected at the end (compiled for S <= 2: fast_supported admits ef == k to 128 only)
  return s;
}

namespace {

struct Shape {
  uint32_t ef, cand_cap, cand_cap_fast, hash_slots;
  uint32_t q_hash_slots, q_bits;        // fast kernel: visited-set tier 1 in 16-bit slots (LDS words, id-space width; 0 = not applicable)
  uint32_t l_cand_cap, l_hash_slots;    // lean kernel
  uint32_t fb_cand_cap, fb_hash_slots;  // last-resort pass (one workgroup per CU, whole LDS)
};
// words of scratch per query; beyond ef = 256 (the flat kernel's S = 6, 8 shapes: up to ~3 k accepted neighbours and > 1 k hops per
// query at ef = 512) the insertion and hop logs are twice / four times as long
uint32_t log_cap_for(uint32_t ef) { return ef <= 256 ? kLogCap : 2 * kLogCap; }
uint32_t hop_cap_for(uint32_t ef) { return ef <= 256 ? kHopCap : 4 * kHopCap; }
uint32_t spill_stride_for(uint32_t ef) { return kSpillSlots + 2 * kCand2Cap + 2 * log_cap_for(ef) + hop_cap_for(ef) / 4 + kParkWords; }

hs_status plan_shape(const PlanInput &in, Shape &s, const char **msg) {
  const size_t ef = std::max<size_t>(in.ef, in.k);
  if (ef > (1u << 20)) { *msg = "ef too large"; return HS_ERR_INVALID; }
  s.ef = (uint32_t)ef;
  // LDS share of the candidate heap: must cover essentially every query (peak heap size on the bench data:
  // 2.4 ef median, 4.4 ef + 40 at p99.9) -- tier 2 is a safety net, a few %% of queries living in it already
  // cost 15-40 %% of throughput (profiles/r01_tier2_cost.txt)
  s.cand_cap_fast = in.user_cand_cap ? in.user_cand_cap : (uint32_t)(4.4 * ef + 64);
  s.cand_cap_fast = (s.cand_cap_fast + 1) & ~1u;
  // the strict kernel keeps its whole heap in LDS: cover the observed maximum (4.9 ef + margin)
  s.cand_cap = in.user_cand_cap ? in.user_cand_cap : (uint32_t)((3 * ef + 256) << in.grow_cand);
  s.cand_cap = (s.cand_cap + 1) & ~1u;
  // tier-1 visited set: sized so that most queries never leave LDS (75 % fill); the rest spill to tier 2
  const uint32_t want = (uint32_t)((450 + 5 * ef) * (1.0 + 0.25 * in.grow_hash) / 0.75);
  s.hash_slots = in.user_hash_slots ? (in.user_hash_slots + 63) / 64 * 64 : (want + 63) / 64 * 64;
  // Fast kernel: the same LDS holds twice the ids as 16-bit remainders of a bijective hash, eight to a 16-byte bucket, no
  // probing (csrc/search_common.hpp).  Buckets: a power of two with the expected number of visited ids filling them to
  // 5 of 8 on average (4.5 would double the table at ef=384 for nothing: measured); usable while the id space is at most 16 bits
  // wider than the bucket index.
  {
    const uint32_t n_vis = in.user_hash_slots ? in.user_hash_slots : (uint32_t)((450 + 5 * ef) * (1.0 + 0.25 * in.grow_hash));
    uint32_t nb = 4;
    while (nb * 5.0 < n_vis && nb < (1u << 14)) nb <<= 1;
    uint32_t bbits = 0, idbits = 1;
    while ((1u << bbits) < nb) bbits++;
    while (idbits < 32 && ((uint64_t)1 << idbits) < (uint64_t)std::max<size_t>(in.n, 2)) idbits++;
    const uint32_t B = std::max(idbits, bbits);
    s.q_hash_slots = nb * 4;
    s.q_bits = (in.diag.vis16 && B - bbits <= 16 && B < 32) ? B : 0;
  }
  const uint32_t dim = (uint32_t)in.dim;
  // Lean kernel (large ef): candidate heap ~p99 of its peak size, visited set ~p90 of the distance evaluations at an 87.5 % fill
  // limit (measured on the 1M SIFT-like bench index, ef 32..256); the rest continue in their tier-2 regions.
  {
    uint32_t lc = in.user_cand_cap ? in.user_cand_cap : (uint32_t)((2.5 * ef + 130) * (1u << in.grow_cand));
    s.l_cand_cap = std::max<uint32_t>((lc + 1) & ~1u, 16);
    const uint32_t lh = in.user_hash_slots ? in.user_hash_slots : (uint32_t)((520 + 5 * ef) * (1.0 + 0.25 * in.grow_hash) / 0.875);
    s.l_hash_slots = (lh + 63) / 64 * 64;
  }
  // shrink the first-pass shape if it does not fit one CU at all
  while (strict_lds_bytes(dim, s.ef, s.cand_cap, s.hash_slots) > kLdsPerCU && s.hash_slots > 256) s.hash_slots >>= 1;
  while (strict_lds_bytes(dim, s.ef, s.cand_cap, s.hash_slots) > kLdsPerCU && s.cand_cap > 128) s.cand_cap = (s.cand_cap / 2 + 1) & ~1u;
  if (strict_lds_bytes(dim, s.ef, s.cand_cap, s.hash_slots) > kLdsPerCU) {
    *msg = "ef/dim do not fit the 160 KiB LDS of one CU";
    return HS_ERR_CAPACITY;
  }
  // last resort (see kFbGrid): LDS = query + result array + a kFbHash-slot visited hash; everything else in global memory.
  // (It goes out with every batch and is normally empty; when it asked for 64 KiB -- before that for a whole CU -- it waited 0.56 ms
  // on average for that much LDS to drain behind the other streams' launches, profiles/r03_kernel_stats_pipelined.csv.)
  s.fb_cand_cap = kFbCand;
  s.fb_hash_slots = kFbHash;
  while (strict_lds_bytes(dim, s.ef, 0, s.fb_hash_slots) > kLdsPerCU && s.fb_hash_slots > 256) s.fb_hash_slots >>= 1;
  return HS_OK;
}

// Flat kernel (flat_search.hip): visited-set buckets, the division constants of bucket = h mod nb, and the LDS share of its
// (lazily replayed) candidate heap.  The bucket count takes whatever LDS the wave's residency granule leaves unused: 5 wavefronts
// per SIMD = 20 workgroups per CU = 8 KiB each on the common shapes (flatk_waves_per_cu).
struct FlatPlan { uint32_t nb, mul, sh, vis_bits; bool ok; };
FlatPlan plan_flat(const PlanInput &in, uint32_t ef) {
  FlatPlan f{};
  const uint32_t dim = (uint32_t)in.dim;
  uint32_t idbits = 1;
  while (idbits < 32 && ((uint64_t)1 << idbits) < (uint64_t)std::max<size_t>(in.n, 2)) idbits++;
  f.vis_bits = idbits;
  // expected visited ids per query (distance evaluations, measured on the 1M SIFT-like bench index: 450 + 5 ef), 3.2 per bucket of 7
  uint32_t nb = in.user_hash_slots ? std::max<uint32_t>(in.user_hash_slots / 4, 8) : (uint32_t)((450 + 5.0 * ef) * (1.0 + 0.25 * in.grow_hash) / 3.2);
  nb = std::max<uint32_t>(nb, 8);
  if (!in.user_hash_slots) {
    const size_t total = flatk_lds_bytes(dim, ef, nb);
    const size_t env_waves = (size_t)in.diag.flat_waves_per_cu;
    const size_t max_waves = env_waves ? env_waves : flatk_waves_per_cu(dim, ef);
    size_t waves = std::min<size_t>(max_waves, kLdsPerCU / std::max<size_t>(total, 1));
    // (Until round 3 a launch smaller than the wave slots took fewer, larger shares.  Measured, profiles/r03_small_launch_lds_share_ab.log:
    //  nothing gained on a single small launch -- 1250 SIFT queries 0.705 vs 0.655 ms, 1000 GIST queries 3.420 vs 3.416 ms -- and with
    //  16 such launches in flight the larger shares cap the residency: 416 k vs 520 k q/s.  The share is the full-residency one.)
    if (waves >= 1) {
      const size_t share = std::min<size_t>((kLdsPerCU / waves) & ~size_t(15), 64 * 1024);
      if (share > total) nb += (uint32_t)((share - total) / 16);
    }
  }
  nb = std::min<uint32_t>(nb, 1u << 14);
  // remainders h div nb must fit 15 bits
  while (((uint64_t)1 << idbits) / nb > 32767 && nb < (1u << 16)) nb += nb / 2;
  if (((uint64_t)1 << idbits) / nb > 32767 || idbits > 31) return f;
  uint32_t sh = 0;
  while ((2u << sh) <= nb) sh++;   // floor(log2(nb))
  uint64_t m = (((uint64_t)1 << (32 + sh)) + nb - 1) / nb;
  if (m >> 32) { sh--; m = (((uint64_t)1 << (32 + sh)) + nb - 1) / nb; }
  f.nb = nb; f.mul = (uint32_t)m; f.sh = sh;
  f.ok = flatk_lds_bytes(dim, ef, nb) <= kLdsPerCU;
  return f;
}

}  // namespace

hs_status plan_search(const PlanInput &in, SearchPlan &p, const char **msg) {
  p = SearchPlan{};
  Shape sh;
  hs_status ps = plan_shape(in, sh, msg);
  if (ps != HS_OK) return ps;
  const Diag &dg = in.diag;
  const uint32_t dim = (uint32_t)in.dim, k = (uint32_t)in.k;
  const size_t nq = in.nq;
  // what the kernels' *_supported predicates read of a DevIndex (of the two tile arrays: whether they exist)
  static const uint32_t present[2] = {0, 0};
  DevIndex dev{};
  dev.n = (uint32_t)in.n; dev.dim = dim; dev.maxlevel = in.maxlevel; dev.threshold_level = in.threshold_level;
  dev.has_deleted = in.has_deleted; dev.kind = in.kind;
  dev.tile0 = in.has_tile0 ? present : nullptr;
  dev.uptile = in.has_uptile ? reinterpret_cast<const uint2 *>(present) : nullptr;

  p.ef = sh.ef;
  p.mark_ep = (in.kind == HS_KIND_SLIM && in.mode == HS_MODE_PQ) ? 1 : 0;
  p.spill_stride = spill_stride_for(sh.ef); p.log_cap = log_cap_for(sh.ef); p.hop_cap = hop_cap_for(sh.ef);
  p.flat = dg.flat ? 1u : 0u;
  // A launch that cannot fill the GPU anyway (fewer queries than wavefront slots) lasts as long as its longest query, and
  // LDS is not what limits it: the 16-bit visited set then takes up to 4x the buckets, as far as the queries of this launch
  // still all fit on the chip at once -- the longest queries never see a full bucket.
  if (sh.q_bits && !in.user_hash_slots) {
    const size_t waves_per_cu = std::max<size_t>((nq + 255) / 256, 1);
    const size_t budget = std::min<size_t>(kLdsPerCU / waves_per_cu, 64 * 1024);
    uint32_t bbits = 0;
    while ((1u << bbits) < sh.q_hash_slots / 4) bbits++;
    for (int step = 0; step < 2; step++) {
      const uint32_t bigger = sh.q_hash_slots * 2;
      const size_t lds_fast = fast_lds_bytes(dim, sh.ef, sh.cand_cap_fast, bigger);
      const size_t lds_lean = lean_lds_bytes(dim, sh.ef, sh.l_cand_cap, bigger);
      if (std::max(lds_fast, lds_lean) > budget || bbits + 1 > sh.q_bits) break;
      sh.q_hash_slots = bigger;
      bbits++;
    }
  }
  const bool filt = in.has_filter != 0;   // a filter set: planned as delete marks are (the reference's !bare_bone branches)
  const uint32_t fast_hash = sh.q_bits ? sh.q_hash_slots : sh.hash_slots;
  const bool fast = !in.exact_order && !in.want_raw && fast_supported(dev, sh.ef, k, filt) &&
                    fast_lds_bytes(dim, sh.ef, sh.cand_cap_fast, fast_hash) <= kLdsPerCU;
  // The flat kernel (lazy candidate heap, flat_search.hip) answers every bare index it supports.  The older kernels run where it
  // does not (filters, delete marks, threshold_level > 0, dim % 16 != 0, ef > 512: fast / strict) and when asked for by name:
  // HS_KERNEL=lean|fast for A/B runs and their parity tests (HS_LEAN_MIN_EF=<ef> asks for the lean kernel from that ef upwards),
  // HS_KERNEL=flat forces the flat kernel.  No property of the DATA enters the choice (until round 2 a strided sample of the rows
  // -- "integer-valued?" -- moved the lean / fast threshold).
  const bool lean_asked = dg.lean_forced || dg.kernel == HS_PLAN_KERNEL_LEAN;
  // An index without fp32 rows (hs_index_set_f32_resident): the choice below is what it would be with them, and whichever of flat /
  // fast / strict it names -- the re-run pass too -- is launched as its narrow twin.  The lean kernel (diagnostic, by environment
  // only) has none and is never chosen here: its requests fall through to the fast kernel.
  const bool f32_free = !in.f32_resident;
  const uint32_t lean_hash = sh.q_bits ? sh.q_hash_slots : sh.l_hash_slots;
  const bool lean = lean_asked && !filt && !f32_free && fast && sh.ef >= dg.lean_min_ef && lean_supported(dev, sh.ef, k) &&
                    lean_lds_bytes(dim, sh.ef, sh.l_cand_cap, lean_hash) <= kLdsPerCU;
  const bool flatk_off = dg.kernel == HS_PLAN_KERNEL_LEAN || dg.kernel == HS_PLAN_KERNEL_FAST;
  const FlatPlan fp = plan_flat(in, sh.ef);
  p.fl_nb = fp.nb; p.fl_mul = fp.mul; p.fl_sh = fp.sh; p.fl_bits = fp.vis_bits; p.fl_ok = fp.ok;
  // The flat kernel test-and-marks the ids of one expansion in all lanes at once, every lane reading its bucket before any lane
  // writes (flat_search.hip vis_mark): two lanes holding the same unvisited id would both find it new.  An index with a level-0
  // list that repeats an id (has_dup0, found when the lists are packed) therefore stays with the other kernels, whose
  // compare-and-swap inserts (search_common.hpp) let the first occurrence win and show it to the second.
  const bool distinct0 = !in.has_dup0;
  const bool flatk = !flatk_off && !dg.lean_forced && !filt && fast && fp.ok && distinct0 && flatk_supported(dev, sh.ef, k);

  p.family = flatk ? HS_PLAN_FLAT : lean ? HS_PLAN_LEAN : fast ? HS_PLAN_FAST : HS_PLAN_STRICT;
  // the flat kernel reads the narrow copy wherever the index has one (the same launch plan), the others only when it is all there is
  p.rerun_rows = f32_free ? in.row_fmt : HS_ROWS_F32;
  p.rows = flatk ? in.row_fmt : p.rerun_rows;
  p.name = kernel_name(p.family, p.rows);
  // A launch much larger than what the GPU holds at once (4096 wavefronts of this kernel) ends on the queries that
  // started last; if those are long ones the whole chip waits for them.  The distance of the level-0 entry predicts
  // the number of expansions (rank correlation 0.5 on the bench data), so the descent runs as a launch of its own,
  // the queries are ordered by that distance, farthest first, and the level-0 search takes them in that order.
  p.split = fast && split_launch(dg, nq);
  p.skip_order = p.split && p.family == HS_PLAN_FAST && dg.order == 2;   // diagnostic: the split without the ordering
  // pass 0: every query, one wavefront each.  Flat: a query that exhausts its scratch is left ST_OVERFLOW, one whose logs did not
  // fit ST_HAZARD; lean: a query that exhausts even its tier-2 regions is left ST_OVERFLOW for the re-run pass
  switch (p.family) {
    case HS_PLAN_FLAT:
      p.cand_cap = sh.cand_cap; p.hash_slots = fp.nb * 4; p.vis_bits = fp.vis_bits;
      p.lds_bytes = (uint32_t)flatk_lds_bytes(dim, sh.ef, fp.nb);
      break;
    case HS_PLAN_LEAN:
      p.cand_cap = sh.l_cand_cap; p.hash_slots = lean_hash; p.vis_bits = sh.q_bits; p.hash_fill_shift = 3;
      p.lds_bytes = (uint32_t)lean_lds_bytes(dim, sh.ef, p.cand_cap, p.hash_slots);
      break;
    case HS_PLAN_FAST:
      p.cand_cap = sh.cand_cap_fast; p.hash_slots = fast_hash; p.vis_bits = sh.q_bits;
      p.lds_bytes = (uint32_t)fast_lds_bytes(dim, sh.ef, p.cand_cap, p.hash_slots);
      break;
    default:
      p.cand_cap = sh.cand_cap; p.hash_slots = sh.hash_slots;
      p.lds_bytes = (uint32_t)strict_lds_bytes(dim, sh.ef, p.cand_cap, p.hash_slots);
      break;
  }
  // Re-run pass (normally empty: a launch that scans the statuses and exits): tie queries whose insertion log did not fit
  // (ST_HAZARD) and queries that outgrew their scratch (ST_OVERFLOW) -> strict kernel, a few workgroups, candidate heap and a
  // large tier-2 visited set per workgroup in global memory (kFbGrid).
  p.rerun_select_mask = (1u << ST_OVERFLOW) | (p.family != HS_PLAN_STRICT ? (1u << ST_HAZARD) : 0u);
  p.rerun_cand_cap = sh.fb_cand_cap; p.rerun_hash_slots = sh.fb_hash_slots;
  return HS_OK;
}

}  // namespace hs
