// What the token-selection kernels share (sample.hip, spec_verify.hip): the Philox4x32-10
// generator, the order-preserving keys of the logits, the aligned-vector walk over a row at
// any element-aligned address, and the block-wide radix select behind top-k and top-p.  The
// contract these implement is written down in ops/sampling.py.
#pragma once
#include "common.h"

namespace pa {
namespace smp {

typedef unsigned long long u64;

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / 64;
constexpr int kCopies = kWaves;  // histogram copies: one per wave
constexpr float kFix = 1099511627776.f;  // 2^40

// ---------------------------------------------------------------- Philox4x32-10
// first output word for key (seed lo, seed hi) and counter (c0, c1, c2, 0)
__device__ __forceinline__ uint32_t philox_x0(u64 seed, uint32_t c0, uint32_t c1, uint32_t c2 = 0u) {
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  uint32_t x0 = c0, x1 = c1, x2 = c2, x3 = 0u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const u64 p0 = (u64)0xD2511F53u * x0, p1 = (u64)0xCD9E8D57u * x2;
    const uint32_t y0 = (uint32_t)(p1 >> 32) ^ x1 ^ k0, y1 = (uint32_t)p1;
    const uint32_t y2 = (uint32_t)(p0 >> 32) ^ x3 ^ k1, y3 = (uint32_t)p0;
    x0 = y0; x1 = y1; x2 = y2; x3 = y3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return x0;
}

// ---------------------------------------------------------------- element access
// T = u16 (bf16 bits) or float.  Key<T>: order-preserving unsigned key of a logit, 16 bits
// for bf16 and 32 for fp32; NaN counts as -inf and -0 as +0 (the contract is on values).
template <typename T> struct Key;
template <> struct Key<u16> {
  static constexpr int kBits = 16;
  static constexpr int kVec = 8;
  typedef u16x8 vec_t;
  static __device__ __forceinline__ uint32_t key(u16 b) {
    if ((b & 0x7fffu) > 0x7f80u) b = 0xff80u;  // NaN -> -inf
    if (b == 0x8000u) b = 0u;
    return (b & 0x8000u) ? (uint32_t)(u16)~b : (uint32_t)(b | 0x8000u);
  }
  static __device__ __forceinline__ float value(uint32_t k) {
    const u16 b = (k & 0x8000u) ? (u16)(k & 0x7fffu) : (u16)~k;
    return bf2f(b);
  }
};
template <> struct Key<float> {
  static constexpr int kBits = 32;
  static constexpr int kVec = 4;
  typedef f32x4 vec_t;
  static __device__ __forceinline__ uint32_t key(float f) {
    uint32_t b = __float_as_uint(f);
    if ((b & 0x7fffffffu) > 0x7f800000u) b = 0xff800000u;
    if (b == 0x80000000u) b = 0u;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  }
  static __device__ __forceinline__ float value(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
  }
};

// The row as vectors of the 16-byte-aligned address range that contains it: vector jv holds
// the elements i = jv * kVec - off + e.  f(i, key) is called for every i in [0, V) of the
// vector, in index order; a vector that is not wholly inside the row is read by element.
template <typename T, typename F>
__device__ __forceinline__ void visit_vec(const T* row, int off, int V, int jv, F&& f) {
  constexpr int E = Key<T>::kVec;
  const int i0 = jv * E - off;
  if (i0 >= 0 && i0 + E <= V) {
    const typename Key<T>::vec_t v = *reinterpret_cast<const typename Key<T>::vec_t*>(row + i0);
#pragma unroll
    for (int e = 0; e < E; ++e) f(i0 + e, Key<T>::key(v[e]));
  } else {
    for (int e = 0; e < E; ++e) {
      const int i = i0 + e;
      if (i >= 0 && i < V) f(i, Key<T>::key(row[i]));
    }
  }
}

// ---------------------------------------------------------------- block helpers
struct Shared {
  u64 hist[kCopies][256];
  u64 hsum[256];
  u64 wred[kWaves];
  float fred[kWaves];
  u64 bc_above;   // select: weight strictly above the chosen digit's range
  u64 bc_limit;   // select: top_p * (weight of the whole first-level histogram)
  int bc_digit;   // select: the chosen digit
  int found;      // draw: first thread whose inclusive sum passes the target
  int last;       // draw: last index with mass
  int token;
};

__device__ __forceinline__ u64 wave_max_u64(u64 v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const u64 t = __shfl_xor(v, o, 64);
    v = t > v ? t : v;
  }
  return v;
}

// One radix select (see the file comment): the smallest key value t such that the weight
// of the tokens with key > t is below `limit`; tokens below `floor_key` do not take part.
// MASS false: weight 1, limit = k.  MASS true: weight = fixed-point exp((x - xmax) * inv_t),
// limit = top_p * (total weight).  Uniform over the block; ends with the block in step.
template <typename T, bool MASS>
__device__ uint32_t radix_select(Shared& s, const T* row, int off, int V, int nvec, uint32_t floor_key,
                                 u64 limit_count, float top_p, float xmax, float inv_t) {
  constexpr int KB = Key<T>::kBits;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  u64* mine = s.hist[wave];
  uint32_t prefix = 0;
  u64 above = 0, limit = limit_count;
  for (int shift = KB - 8; shift >= 0; shift -= 8) {
    for (int i = tid; i < kCopies * 256; i += kThreads) (&s.hist[0][0])[i] = 0;
    __syncthreads();
    const bool first = shift == KB - 8;
    for (int jv = tid; jv < nvec; jv += kThreads) {
      visit_vec<T>(row, off, V, jv, [&](int, uint32_t k) {
        if (k < floor_key) return;
        if (!first && (k >> (shift + 8)) != prefix) return;
        u64 w = 1;
        if (MASS) w = (u64)(expf((Key<T>::value(k) - xmax) * inv_t) * kFix);
        if (w) atomicAdd(&mine[(k >> shift) & 255u], w);
      });
    }
    __syncthreads();
    if (tid < 256) {
      u64 t = 0;
#pragma unroll 8
      for (int c = 0; c < kCopies; ++c) t += s.hist[c][tid];
      s.hsum[tid] = t;
    }
    __syncthreads();
    if (wave == 0) {
      // lane l owns digits 4l .. 4l+3; sfx = weight of the digits above its four
      u64 h[4], own = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) { h[j] = s.hsum[4 * lane + j]; own += h[j]; }
      u64 inc = own;  // inclusive suffix sum over lanes >= l
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const u64 t = __shfl_down(inc, o, 64);
        if (lane + o < 64) inc += t;
      }
      if (MASS && first) {
        const u64 total = __shfl(inc, 0, 64);
        limit = (u64)((double)top_p * (double)total);
        if (limit < 1) limit = 1;  // the maximum always stays
      }
      // A_d = above + weight of the digits > d, non-increasing in d: the chosen digit is the
      // smallest d with A_d < limit (d = 255 always qualifies: A_255 = above < limit)
      u64 a = above + (inc - own);  // A of digit 4l+3
      int best = 256;
      u64 best_a = 0;
#pragma unroll
      for (int j = 3; j >= 0; --j) {
        if (a < limit) { best = 4 * lane + j; best_a = a; }
        a += h[j];
      }
      int d = best;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const int t = __shfl_xor(d, o, 64);
        d = t < d ? t : d;
      }
      if (d > 255) d = 255;  // unreachable while above < limit; keeps the digit in range
      if (best == d || (lane == 63 && d == 255 && best == 256)) {
        s.bc_digit = d;
        s.bc_above = best == d ? best_a : above;
      }
      if (MASS && first && lane == 0) s.bc_limit = limit;
    }
    __syncthreads();
    prefix = (prefix << 8) | (uint32_t)s.bc_digit;
    above = s.bc_above;
    if (MASS && first) limit = s.bc_limit;
    __syncthreads();
  }
  return prefix;
}

}  // namespace smp
}  // namespace pa
