// rabitq_rotate.hpp -- the FhtKac rotation (rabitqlib/utils/rotator.hpp:370-423) of one vector in LDS by one wavefront, shared by
// the query preparation (slimq_search.hip) and the data-side quantiser (convert_slimq.hip).  The butterflies are element-wise, so
// the result is the host's (rabitq_host.hpp Rotator::rotate) bit for bit in any lane order.
#pragma once
#include <hip/hip_runtime.h>

#include "slimq_engine.hpp"
#include "wave_util.hpp"

namespace hs {

__device__ __forceinline__ void flip_signs(float *y, const uint8_t *f, uint32_t n, int lane) {
#pragma unroll 1
  for (uint32_t i = lane; i < n; i += 64)
    if ((f[i >> 3] >> (i & 7)) & 1) y[i] = -y[i];
}
// in-place Walsh-Hadamard over n (power of two) floats in LDS, butterfly stages in ascending stride, then * scale
__device__ __forceinline__ void fht_lds(float *y, uint32_t n, float scale, int lane) {
  for (uint32_t h = 1; h < n; h <<= 1) {
    wave_sync();
#pragma unroll 1
    for (uint32_t t = lane; t < n / 2; t += 64) {
      const uint32_t j = ((t / h) * 2 * h) + (t % h);
      const float a = y[j], b = y[j + h];
      y[j] = a + b;
      y[j + h] = a - b;
    }
  }
  wave_sync();
#pragma unroll 1
  for (uint32_t i = lane; i < n; i += 64) y[i] *= scale;
}
__device__ __forceinline__ void rotate_lds(const DevSlimQ &sq, float *y, int lane) {
  const uint32_t P = sq.padded, T = sq.trunc, nb = P / 8;
  if (T == P) {
    for (int r = 0; r < 4; r++) {
      wave_sync();
      flip_signs(y, sq.flips + r * nb, P, lane);
      fht_lds(y, T, sq.fht_scale, lane);
    }
    wave_sync();
    return;
  }
  for (int r = 0; r < 4; r++) {
    wave_sync();
    flip_signs(y, sq.flips + r * nb, P, lane);
    fht_lds((r & 1) ? y + (P - T) : y, T, sq.fht_scale, lane);
    wave_sync();
#pragma unroll 1
    for (uint32_t i = lane; i < P / 2; i += 64) {  // kacs_walk
      const float a = y[i], b = y[i + P / 2];
      y[i] = a + b;
      y[i + P / 2] = a - b;
    }
  }
  wave_sync();
#pragma unroll 1
  for (uint32_t i = lane; i < P; i += 64) y[i] *= 0.25f;
  wave_sync();
}

}  // namespace hs
