// What the extend attention kernels share: the launch parameters, the tile geometry, the
// address of a cache row and the conversion of a cache row to bf16.  attn_extend.hip holds the
// kernel with the GQA ratio as a template parameter (1 / 2 / 4 / 8), the merge kernel and the
// entry points; attn_extend_gqa.hip the kernel that takes any ratio up to 16 at run time.
#pragma once
#include "common.h"

namespace ext {

constexpr int kThreads = 256;
constexpr int kBM = 64;  // stacked query rows (token x head of the group) per workgroup
constexpr int kBN = 64;  // keys per tile
constexpr int kMaxSplits = 64;
constexpr int kMaxGroup = 16;  // attn_extend_gqa.hip: the largest Hq / Hk

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

struct Params {
  const pa::u16* q;
  long qsb, qst, qsh;  // element strides of q [B, T, Hq, D] over b, t and head
  const void* kc;
  const void* vc;
  const float* ks;  // e4m3 only: one scale per (slot, kv head)
  const float* vs;
  const int* base_len;  // [B]
  const int* rows;      // [B] q row -> cache row, or null: the identity (paged only)
  const int* table;     // [Bc, max_blocks] (paged only)
  float* ws;            // num_splits > 1: [B*T*Hq, ns, 2] (m, l) then [B*T*Hq, ns, D] acc
  pa::u16* o;
  int B, Bc, T, S_max, Hq, Hk, ns, qtiles;
  int max_blocks, num_blocks, bs_shift;
  float scale_log2;  // scale * log2(e)
};

__device__ __forceinline__ pa::f32x4 mfma16(pa::bf16x8 a, pa::bf16x8 b, pa::f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// The row-address policy: the slot (in units of Hk * D elements, 64-bit) of key `key` of cache
// row cb.  Paged: blk is the key's table entry, which the caller has checked against
// [0, num_blocks) before it dereferences the slot.
template <bool Paged>
__device__ __forceinline__ long cache_slot(const Params& p, int cb, int blk, long key) {
  if constexpr (Paged) return ((long)blk << p.bs_shift) + (key & ((1L << p.bs_shift) - 1));
  else return (long)cb * p.S_max + key;
}

// 8 elements of a cache row as bf16 bits.  e4m3: cvt(code) * scale, exact in bf16.
__device__ __forceinline__ pa::u16x8 row_bf16(const pa::u16x8& r, float) { return r; }
__device__ __forceinline__ pa::u16x8 row_bf16(const u32x2& r, float sc) {
  pa::u16x8 o;
#pragma unroll
  for (int d = 0; d < 2; ++d) {
    const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)r[d], false) * sc;
    const f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)r[d], true) * sc;
    o[4 * d] = pa::f2bf(lo.x);
    o[4 * d + 1] = pa::f2bf(lo.y);
    o[4 * d + 2] = pa::f2bf(hi.x);
    o[4 * d + 3] = pa::f2bf(hi.y);
  }
  return o;
}

// Query tiles of a launch: 64 / g whole tokens per tile (g divides 64: every row of M is live).
inline int query_tiles(int T, int g) { return (int)(((long)T + kBM / g - 1) / (kBM / g)); }

// attn_extend_gqa.hip: the main kernel for any 1 <= Hq / Hk <= kMaxGroup, grid (p.qtiles * p.ns,
// Hk, B) with p.qtiles = query_tiles(T, Hq / Hk).  p.table null: a contiguous cache; p.ks null:
// a bf16 one.  D is 64 or 128.  p.ns > 1: attn_extend_merge_kernel finishes the job.
void launch_extend_gqa(const Params& p, int D, hipStream_t st);

}  // namespace ext
