// rq_dist.hpp -- rabitqlib's raw distance, the one every edge of HNSW-SlimQ's base graph is measured with: the host text
// (rabitq_raw_dist, the definition) and the same recipe on a wavefront (rq_dist_pairs, compiled for the device only), which the batched
// build of that graph (build_gpu.hip) is held to bit for bit through hs_debug_rq_raw_dist.
#pragma once
#include <algorithm>

#include "dist_recipe.hpp"
#include "hd.hpp"
#if defined(__HIPCC__)
#include "wave_util.hpp"
#endif

namespace hs {

// raw_dist_func_ = euclidean_sqr / dot_product_dis (rabitqlib/utils/space.hpp:226-240): `(v0 - v1).dot(v0 - v1)` and
// `1 - v0.dot(v1)` through the vendored Eigen's inner product (Eigen/src/Core/InnerProduct.h:113-159) with 16-float packets
// (the AVX-512 build the parity flags pin): four packet accumulators, the first four packets multiplied, every later one
// fused-multiply-added (pmadd = _mm512_fmadd_ps), folded 2+=3, 1+=2, 0+=1, then predux = halves 8, 4, (0+2, 1+3), (0+1)
// (arch/AVX512/PacketMath.h:1456-1461, AVX :1954, SSE :1852-1853); the < 16 tail is a scalar fused chain.  Unlike the Eigen
// reductions on the SEARCH path this one does not depend on pointer alignment: the operands are expressions.
inline float rabitq_raw_dist(Metric metric, const float *a, const float *b, size_t d) {
  const bool l2 = metric == METRIC_L2;
  auto X = [&](size_t k) { return l2 ? a[k] - b[k] : a[k]; };
  auto Y = [&](size_t k) { return l2 ? a[k] - b[k] : b[k]; };
  float res;
  if (d < 16) {
    if (d == 0) return l2 ? 0.f : 1.f;
    res = X(0) * Y(0);
    for (size_t k = 1; k < d; k++) res = __builtin_fmaf(X(k), Y(k), res);
  } else {
    const size_t packet_end = d / 16 * 16, quad_end = d / 64 * 64, np = d / 16, nrem = (packet_end - quad_end) / 16;
    float acc[4][16];
    for (size_t p = 0; p < std::min<size_t>(np, 4); p++)
      for (size_t j = 0; j < 16; j++) acc[p][j] = X(p * 16 + j) * Y(p * 16 + j);
    if (np >= 4) {
      for (size_t k = 64; k < quad_end; k += 64)
        for (size_t p = 0; p < 4; p++)
          for (size_t j = 0; j < 16; j++) acc[p][j] = __builtin_fmaf(X(k + p * 16 + j), Y(k + p * 16 + j), acc[p][j]);
      for (size_t p = 0; p < nrem; p++)
        for (size_t j = 0; j < 16; j++) acc[p][j] = __builtin_fmaf(X(quad_end + p * 16 + j), Y(quad_end + p * 16 + j), acc[p][j]);
      for (size_t j = 0; j < 16; j++) acc[2][j] = acc[2][j] + acc[3][j];
    }
    if (np >= 3)
      for (size_t j = 0; j < 16; j++) acc[1][j] = acc[1][j] + acc[2][j];
    if (np >= 2)
      for (size_t j = 0; j < 16; j++) acc[0][j] = acc[0][j] + acc[1][j];
    float t8[8], t4[4];
    for (size_t j = 0; j < 8; j++) t8[j] = acc[0][j] + acc[0][j + 8];
    for (size_t j = 0; j < 4; j++) t4[j] = t8[j] + t8[j + 4];
    const float u0 = t4[0] + t4[2], u1 = t4[1] + t4[3];
    res = u0 + u1;
    for (size_t k = packet_end; k < d; k++) res = __builtin_fmaf(X(k), Y(k), res);
  }
  return l2 ? res : 1 - res;
}

#if defined(__HIPCC__)
// One term of the recipe: X(k) * Y(k) as a rounded product (first = true) or fused into acc.  L2 squares the rounded difference
// of the two rows, so the value does not depend on which of them is `q`; nor does a product.
template <int METRIC>
__device__ __forceinline__ float rq_term(float q, float x, float acc, bool first) {
  const float X = METRIC == METRIC_L2 ? q - x : q, Y = METRIC == METRIC_L2 ? q - x : x;
  return first ? X * Y : __builtin_fmaf(X, Y, acc);
}

// The recipe on a wavefront, for cnt pairs: pair r is the row qrow(r) (dim floats, LDS or memory) against the row id(r) of vec, into
// out[r] (LDS).  QMEM: the query rows are in memory, and their elements are loaded with the row's, ahead of the terms, so that
// both loads are in flight together; an LDS row is read term by term.  Sixteen lanes per pair: lane j of the group holds element j of the four packet accumulators, so the wavefront
// measures four pairs per pass and a group reads 64 contiguous bytes per packet.  The folds 2+=3, 1+=2, 0+=1 are lane-local.
// predux is a butterfly over the sixteen lanes at distances 8, 4, 2, 1 (rotations within the DPP row: after the step at distance s
// every value repeats with period s, so a rotation by s / 2 reads what an exchange at that distance would); every add is
// commutative, hence lane 0 -- and every other lane -- ends with the bits of t8 / t4 / (0+2, 1+3) / (0+1).  The tail below a
// packet, and dim < 16 altogether, is the scalar fused chain, run by every lane of the group alike.
template <int METRIC, bool QMEM, class QROW, class ID>
__device__ __forceinline__ void rq_dist_pairs(const float *vec, uint32_t dim, QROW qrow, ID id, float *out, uint32_t cnt, int lane) {
  const uint32_t j = (uint32_t)lane & 15u, grp = (uint32_t)lane >> 4;
  const uint32_t np = dim >> 4, packet_end = np << 4, quad_end = (dim >> 6) << 6, nrem = (packet_end - quad_end) >> 4;
  for (uint32_t base = 0; base < cnt; base += 4) {
    const uint32_t r = base + grp;
    const bool act = r < cnt;
    const uint32_t rr = act ? r : base;
    const float *qv = qrow(rr);
    const float *row = vec + (size_t)id(rr) * dim;
    float res;
    if (np == 0) {
      res = rq_term<METRIC>(qv[0], row[0], 0.f, true);
      for (uint32_t k = 1; k < dim; k++) res = rq_term<METRIC>(qv[k], row[k], res, false);
    } else {
      float acc[4] = {0.f, 0.f, 0.f, 0.f};
      {
        float x[4], q[4];
#pragma unroll
        for (uint32_t p = 0; p < 4; p++)
          if (p < np) { x[p] = row[p * 16 + j]; if (QMEM) q[p] = qv[p * 16 + j]; }
#pragma unroll
        for (uint32_t p = 0; p < 4; p++)
          if (p < np) acc[p] = rq_term<METRIC>(QMEM ? q[p] : qv[p * 16 + j], x[p], 0.f, true);
      }
      if (np >= 4) {
        for (uint32_t k = 64; k < quad_end; k += 64) {
          float x[4], q[4];
#pragma unroll
          for (uint32_t p = 0; p < 4; p++) { x[p] = row[k + p * 16 + j]; if (QMEM) q[p] = qv[k + p * 16 + j]; }
#pragma unroll
          for (uint32_t p = 0; p < 4; p++) acc[p] = rq_term<METRIC>(QMEM ? q[p] : qv[k + p * 16 + j], x[p], acc[p], false);
        }
#pragma unroll
        for (uint32_t p = 0; p < 3; p++)
          if (p < nrem) acc[p] = rq_term<METRIC>(qv[quad_end + p * 16 + j], row[quad_end + p * 16 + j], acc[p], false);
        acc[2] = acc[2] + acc[3];
      }
      if (np >= 3) acc[1] = acc[1] + acc[2];
      if (np >= 2) acc[0] = acc[0] + acc[1];
      res = acc[0];
      res = res + dpp_f<0x128>(res);   // row_ror:8
      res = res + dpp_f<0x124>(res);   // row_ror:4
      res = res + dpp_f<0x122>(res);   // row_ror:2
      res = res + dpp_f<0x121>(res);   // row_ror:1
      for (uint32_t k = packet_end; k < dim; k++) res = rq_term<METRIC>(qv[k], row[k], res, false);
    }
    if (act && j == 0) out[r] = METRIC == METRIC_L2 ? res : 1.0f - res;
  }
}

// rabitq_raw_dist of the row `qv` (LDS, dim floats) against rows nid[0..cnt) (LDS) of vec into nd[0..cnt) (LDS), one wavefront.
template <int METRIC>
__device__ __forceinline__ void rq_dists(const float *vec, uint32_t dim, const float *qv, const uint32_t *nid, float *nd, uint32_t cnt, int lane) {
  rq_dist_pairs<METRIC, false>(vec, dim, [=](uint32_t) { return qv; }, [=](uint32_t r) { return nid[r]; }, nd, cnt, lane);
}

// The pairwise sibling: rabitq_raw_dist(row a_first + r, row ids[r].id) for r < cnt into pd[0..cnt) (LDS), for pairs that share
// no query row (HierarchicalNSWSlimQ's PruneByHeuristic measures candidate i against the row whose id is the loop index i).
// IDS: anything with an `.id` member (the sorted (distance, id) pairs).  The caller guarantees a_first + cnt <= n.
template <int METRIC, class IDS>
__device__ __forceinline__ void rq_pair_dists(const float *vec, uint32_t dim, uint32_t a_first, const IDS *ids, float *pd, uint32_t cnt, int lane) {
  rq_dist_pairs<METRIC, true>(vec, dim, [=](uint32_t r) { return vec + (size_t)(a_first + r) * dim; }, [=](uint32_t r) { return ids[r].id; }, pd, cnt, lane);
}
#endif

}  // namespace hs
