// The two fixed-point epilogues of the integer execution through to the stored output (include/mi355q.h, "Integer
// execution, through to the stored output"): accumulator + bias, fixed-point multiplier, output zero point, the fused
// activation's integer range. Shared by qfc_out.hip (FULLY_CONNECTED, and CONV_2D on patch rows) and dwconv.hip
// (DEPTHWISE_CONV_2D): one statement, one piece of code. The epilogues read bias, mult, shift, per_channel, zp_y,
// act_min and act_max of OutArgs; the other members are qfc_out.hip's.
#pragma once

#include "common.h"

namespace mi355q {

struct OutArgs {
  const void* xq;          // int8 / int16 [n, d]
  const uint8_t* w;        // [rows, d] stored
  const void* bias;        // int32 / int64 [rows] or null
  const int32_t* mult;     // 1 or rows
  const int32_t* shift;    // 1 or rows
  const int32_t* wsum;     // [rows] (i8: read only when zp_x != 0; i16: the MFMA route)
  void* q;                 // int8 / int16 [n, rows]
  long long n, rows, d;
  int per_channel;         // mult / shift have rows entries
  int zp_x, zp_y;
  int act_min, act_max;
  int kind;
};

// ---------------------------------------------------------------- the fixed-point epilogues
__device__ __forceinline__ int sat32(long long v) {
  return v > 2147483647LL ? 2147483647 : v < -2147483648LL ? static_cast<int>(-2147483648LL) : static_cast<int>(v);
}

// One output channel's constants of the int8 op; the shift is brought into [-31, 30] so that no shift is undefined.
struct Chan8 {
  long long bias;
  int m, left, right;
};

__device__ __forceinline__ Chan8 chan8(const OutArgs& g, long long r) {
  const int c = g.per_channel ? static_cast<int>(r) : 0;
  int s = g.shift[c];
  s = s < -31 ? -31 : s > 30 ? 30 : s;
  return Chan8{g.bias ? static_cast<long long>(static_cast<const int32_t*>(g.bias)[r]) : 0LL, g.mult[c], s > 0 ? s : 0,
               s < 0 ? -s : 0};
}

// clamp(mbqm32(sat32(acc + bias), M, s) + zp_y, act_min, act_max)
__device__ __forceinline__ int8_t output8(int acc, const Chan8& c, const OutArgs& g) {
  const int a = sat32(static_cast<long long>(acc) + c.bias);
  const int v = sat32(static_cast<long long>(a) * (1LL << c.left));
  const long long p = static_cast<long long>(v) * c.m;
  const long long h = (p + (p >= 0 ? (1LL << 30) : 1 - (1LL << 30))) / (1LL << 31);      // truncating division
  const long long mask = (1LL << c.right) - 1;
  const long long r = (h >> c.right) + (((h & mask) > (mask >> 1) + (h < 0 ? 1 : 0)) ? 1 : 0);
  const long long q = r + g.zp_y;
  return static_cast<int8_t>(q < g.act_min ? g.act_min : q > g.act_max ? g.act_max : q);
}

// One output channel's constants of the int16 op: Mr = the multiplier rounded to 15 bits, T = 15 - s in [1, 46].
struct Chan16 {
  long long bias, mr, half;
  int t;
};

__device__ __forceinline__ Chan16 chan16(const OutArgs& g, long long r) {
  const int c = g.per_channel ? static_cast<int>(r) : 0;
  const int m = g.mult[c];
  int s = g.shift[c];
  s = s < -31 ? -31 : s > 14 ? 14 : s;
  long long b = g.bias ? static_cast<const long long*>(g.bias)[r] : 0LL;
  b = b > (1LL << 62) ? (1LL << 62) : b < -(1LL << 62) ? -(1LL << 62) : b;      // (acc + b cannot wrap; a is the same)
  const int t = 15 - s;
  return Chan16{b, m < 0x7FFF0000 ? static_cast<long long>((m + (1 << 15)) >> 16) : 0x7FFFLL, 1LL << (t - 1), t};
}

constexpr long long kA16Max = (1LL << 47) - 1, kA16Min = -(1LL << 47);

// clamp((clamp(acc + bias, -2^47, 2^47 - 1) * Mr + 2^(T - 1)) >> T, act_min, act_max)
__device__ __forceinline__ int16_t output16(long long acc, const Chan16& c, const OutArgs& g) {
  long long a = acc + c.bias;
  a = a > kA16Max ? kA16Max : a < kA16Min ? kA16Min : a;
  const long long r = (a * c.mr + c.half) >> c.t;
  return static_cast<int16_t>(r < g.act_min ? g.act_min : r > g.act_max ? g.act_max : r);
}

}  // namespace mi355q
