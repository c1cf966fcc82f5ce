// How a comparison target is read: element e of a tensor in its stored form (mi355q_compare_pair), dequantized in
// registers. Shared by the comparison metrics (validation.hip), the weight delta of the layer output error
// (layer_error.hip) and its form behind an inserted transformation (hadamard.hip).
#pragma once

#include "common.h"

namespace mi355q {

// Stored integer q of scale entry c, dequantized as NumPy does it.
__device__ __forceinline__ float dequantize_target(const mi355q_compare_pair& p, int32_t q, int64_t c) {
  // NumPy subtracts in the promoted integer type of (q, zero_point) and wraps (int8 - int8 stays int8)
  int32_t d = static_cast<int32_t>(static_cast<uint32_t>(q) - static_cast<uint32_t>(p.zero_point ? p.zero_point[c] : 0));
  if (p.diff_bits == 8) d = static_cast<int8_t>(d);
  else if (p.diff_bits == 16) d = static_cast<int16_t>(d);
  const float s = p.scale[c];
  // int8 / int16 * float32 is a float32 product; int32 * float32 is float64, cast to float32 afterwards
  if (p.diff_bits == 32) return static_cast<float>(static_cast<double>(d) * static_cast<double>(s));
  return static_cast<float>(d) * s;
}

// Element k of a word of packed `bits`-wide integers, element 0 in the low bits, sign-extended.
__device__ __forceinline__ int32_t packed_element(uint32_t word, int bits, int k) {
  return static_cast<int32_t>(word << (32 - bits * (k + 1))) >> (32 - bits);
}

// Target element e as NumPy's get_tensor_data + np.asarray(..., np.float32) sees it.
__device__ __forceinline__ float load_target(const mi355q_compare_pair& p, int64_t e) {
  int32_t q;
  switch (p.target_kind) {
    case MI355Q_CMP_F32: return static_cast<const float*>(p.target)[e];
    case MI355Q_CMP_F16: return static_cast<float>(static_cast<const _Float16*>(p.target)[e]);
    case MI355Q_CMP_BF16: return u2f(static_cast<uint32_t>(static_cast<const uint16_t*>(p.target)[e]) << 16);
    case MI355Q_CMP_I8: q = static_cast<const int8_t*>(p.target)[e]; break;
    case MI355Q_CMP_I16: q = static_cast<const int16_t*>(p.target)[e]; break;
    case MI355Q_CMP_I32: q = static_cast<const int32_t*>(p.target)[e]; break;
    case MI355Q_CMP_I4: q = packed_element(static_cast<const uint8_t*>(p.target)[e >> 1], 4, static_cast<int>(e & 1)); break;
    default: q = packed_element(static_cast<const uint8_t*>(p.target)[e >> 2], 2, static_cast<int>(e & 3)); break;  // I2
  }
  return dequantize_target(p, q, p.channels == 1 ? 0 : (e / p.inner) % p.channels);
}

}  // namespace mi355q
