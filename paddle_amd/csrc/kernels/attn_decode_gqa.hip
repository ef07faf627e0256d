// Split-KV decode attention on the matrix unit for gfx950: one query token per row against
// kv_len[b] cached keys, for any GQA ratio G = Hq / Hk with 1 <= G <= 16.  G is a runtime
// value: the G query heads of a group are one 16-wide MFMA operand (padded with zeros made in
// registers), so the cost per key does not grow with G and there is one instantiation per
// (D in {64, 128}, contiguous | paged, bf16 | e4m3) and none per ratio.
//
// Work split.  Grid (num_splits, Hk, B), four waves.  A split owns an equal chunk of the row's
// own length, rounded up to whole wave tiles of kKT = 32 keys; wave w owns the tiles w, w + 4,
// ... of the chunk.  There is no workgroup barrier in the main loop: the waves meet once at
// the end through LDS, and every split stores its (m, l, acc[D]) per query head with plain
// stores in the workspace layout of pa_attn_decode, which attn_decode_merge_kernel finishes.
// No atomics, flags or spins: the result is bit-identical from run to run.
//
// Arithmetic (v_mfma_f32_16x16x32_bf16, A[row l&15][k 8(l>>4)+j], B[k 8(l>>4)+j][col l&15],
// C[row 4(l>>4)+reg][col l&15]), per wave tile of 32 keys:
//   S^T = K Q^T    A = 16 keys: lane l loads the 16 bytes of key row l & 15 at d = 8 (l >> 4)
//                  + 32 s straight from global memory into the operand register (8 bytes of
//                  e4m3 and one v_cvt_scalef32_pk_bf16_fp8 per pair with the key's scale: the
//                  append's scales are powers of two, so the product is exact in bf16).  B =
//                  the group's query rows, loaded once.  A lane then holds keys 16 c + 4 (l >>
//                  4) + reg, c = 0, 1, of query l & 15: the softmax maximum and sum are in-lane
//                  plus two shuffles.  scale * log2(e) is applied to the fp32 scores.
//   O^T = V^T P^T  B = P rounded to bf16 once, straight from the S^T registers: element j of
//                  lane group h is key 16 (j >> 2) + 4 h + (j & 3) of the tile.  A = V^T in the
//                  same key order: the V tile is staged row-major (bf16; e4m3 dequantised on
//                  the way in) in a wave-private LDS region and read back by two
//                  ds_read_b64_tr_b16 per 16 elements of d -- lane l of a 16-lane group passes
//                  the address of (row l >> 2, columns 4 (l & 3)..+3) of a 4 x 16 block and
//                  receives column l, rows ascending.
// The next tile's K and V loads (and, paged, the table entries of the tile after it) are
// issued before the arithmetic on this tile and stay in flight under it.
//
// One V buffer per wave, not two: the LDS instructions of one wave execute in order, so the
// writes of tile t + 1 queue behind the transposing reads of tile t without a second buffer,
// and the data they write arrives from global memory later than those reads anyway.  A second
// buffer would take 74 KiB of LDS per workgroup at D = 128 (two workgroups per compute unit
// instead of four) and buy no overlap.  Wavefront-scope fences keep the compiler from moving
// the reads across the writes; they emit no instruction.  The pitch of a V row is D + 16
// elements, which spreads the 16 rows of a transposing read over all 64 banks.
//
// Masking.  A key at or beyond the split's end, and a paged key whose table entry is outside
// [0, num_blocks), is never loaded: zeros go to the operand and to LDS and its score becomes
// -inf, so NaN codes, an inf scale or another row's token in such a slot cannot reach 0 * v.
// A wave tile starts at a multiple of 16 keys and a block holds at least 16, so a tile needs
// two table entries, which are wave-uniform.  Every cache offset is computed in 64 bits.
//
// Bit equalities: the address of a cache row and the storage type are compile-time policies
// in front of the same arithmetic, so paged returns the bits of contiguous for the same
// tokens and e4m3 the bits of bf16 over the dequantised cache; a row's result does not depend
// on the other rows.  The bits of attn_decode_kernel (VALU, P in fp32) are not reproduced.
#include <type_traits>

#include "attn_decode_params.h"

using namespace pa;

namespace dec {
namespace gqa {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kKT = 32;  // keys per wave tile: two S^T blocks of 16, one k-step of O^T

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

__device__ __forceinline__ f32x4 mfma16(bf16x8 a, bf16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// 8 elements of a cache row as a bf16 operand.  e4m3: code * scale, exact (see the header).
__device__ __forceinline__ bf16x8 row_bf16(const u16x8& r, float) { return __builtin_bit_cast(bf16x8, r); }
__device__ __forceinline__ bf16x8 row_bf16(const u32x2& r, float sc) {
  bf16x8 o;
#pragma unroll
  for (int d = 0; d < 2; ++d) {
    const bf16x2 lo = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(r[d], sc, false);
    const bf16x2 hi = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(r[d], sc, true);
    o[4 * d] = lo[0];
    o[4 * d + 1] = lo[1];
    o[4 * d + 2] = hi[0];
    o[4 * d + 3] = hi[1];
  }
  return o;
}

// Orders the LDS accesses of the lanes of one wave in the compiler; the hardware keeps them in
// program order by itself.
__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int D, bool Paged, bool F8>
__global__ __launch_bounds__(kThreads) void attn_decode_gqa_kernel(DecodeParams p) {
  constexpr int KS = D / 32;       // k-steps of S^T
  constexpr int DB = D / 16;       // 16-element blocks of d in O^T
  constexpr int CPR = D / 8;       // 8-element chunks per cache row
  constexpr int RPL = 64 / CPR;    // V rows one load instruction of the wave covers
  constexpr int NV = kKT / RPL;    // V loads per lane per tile
  constexpr int VP = D + 16;       // pitch of a V row in LDS (elements)
  constexpr long kStep = (long)kWaves * kKT;  // keys between a wave's consecutive tiles
  using Elt = typename std::conditional<F8, uint8_t, u16>::type;
  using Vec = typename std::conditional<F8, u32x2, u16x8>::type;  // 8 elements of a row
  static_assert(kKT * VP * 2 >= 16 * D * 4, "a wave's V region also holds its 16 x D fp32 partial");
  __shared__ __attribute__((aligned(16))) u16 sV[kWaves][kKT * VP];  // wave-private
  __shared__ float s_ml[kWaves][16][2];

  const int split = blockIdx.x, hk = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lq = lane & 15, lh = lane >> 4;
  const int G = p.Hq / p.Hk;

  int len = p.kv_len[b];
  len = len < 0 ? 0 : (len > p.S_max ? p.S_max : len);
  // this split's key range: equal chunks of the row's own length, whole wave tiles
  int chunk = (len + p.ns - 1) / p.ns;
  chunk = (chunk + kKT - 1) / kKT * kKT;
  const long start = (long)split * chunk;
  const long end = start + chunk < (long)len ? start + chunk : (long)len;

  // B operand of S^T: query head hk * G + lq, zeros for the rows G..15
  bf16x8 qf[KS];
  {
    const u16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
    const u16* qp = p.q + (long)b * p.qsb + (long)(hk * G + (lq < G ? lq : 0)) * p.qsh + lh * 8;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const u16x8 v = lq < G ? *reinterpret_cast<const u16x8*>(qp + 32 * s) : z;
      qf[s] = __builtin_bit_cast(bf16x8, v);
    }
  }

  float m = -INFINITY, l = 0.f;
  f32x4 acc[DB];
#pragma unroll
  for (int db = 0; db < DB; ++db) acc[db] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const long rowe = (long)p.Hk * D;  // elements between consecutive slots
  const Elt* kb = reinterpret_cast<const Elt*>(p.kc) + (long)hk * D + lh * 8;             // + 32 s
  const Elt* vb = reinterpret_cast<const Elt*>(p.vc) + (long)hk * D + (lane % CPR) * 8;
  const int vrow = lane / CPR;  // this lane's V row of a load, + RPL * i
  const int* trow = Paged ? p.table + (long)b * p.max_blocks : nullptr;
  const long bmask = Paged ? (1L << p.bs_shift) - 1 : 0;
  u16* sv = sV[wave];

  Vec kr[2][KS], vr[NV];
  float ksc[2], vsc[NV];
  bool okh[2];  // paged: whether the block of each 16-key half of the loaded tile exists
  int ent[2];   // paged: the table entries of the tile loaded next (wave-uniform)
  // key < end <= S_max <= max_blocks << bs_shift keeps the read inside the row
  auto fetch_entries = [&](long k0) {
    if constexpr (Paged) {
#pragma unroll
      for (int c = 0; c < 2; ++c) ent[c] = k0 + 16 * c < end ? trow[(k0 + 16 * c) >> p.bs_shift] : -1;
    }
  };
  // the slot of a key of half c of the tile at k0, in units of Hk * D elements
  auto slot_of = [&](long key, int c) -> long {
    if constexpr (Paged) return ((long)ent[c] << p.bs_shift) + (key & bmask);
    else return (long)b * p.S_max + key;
  };
  // global -> registers; a key without a slot loads nothing and holds zeros
  auto load_tile = [&](long k0) {
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      okh[c] = !Paged || (unsigned)ent[c] < (unsigned)p.num_blocks;
      const long key = k0 + 16 * c + lq;
      const bool ok = key < end && okh[c];
      const long slot = slot_of(key, c);
      ksc[c] = 0.f;
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        Vec kz;
#pragma unroll
        for (int j = 0; j < (F8 ? 2 : 8); ++j) kz[j] = 0;
        if (ok) kz = *reinterpret_cast<const Vec*>(kb + slot * rowe + 32 * s);
        kr[c][s] = kz;
      }
      if constexpr (F8) {
        if (ok) ksc[c] = p.ks[slot * p.Hk + hk];
      }
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      constexpr int kHalf = NV / 2;  // loads per 16-key half
      const int c = i / kHalf;
      const long key = k0 + vrow + RPL * i;
      const bool ok = key < end && okh[c];
      const long slot = slot_of(key, c);
      Vec vz;
#pragma unroll
      for (int j = 0; j < (F8 ? 2 : 8); ++j) vz[j] = 0;
      vsc[i] = 0.f;
      if (ok) {
        vz = *reinterpret_cast<const Vec*>(vb + slot * rowe);
        if constexpr (F8) vsc[i] = p.vs[slot * p.Hk + hk];
      }
      vr[i] = vz;
    }
  };

  const long first = start + (long)wave * kKT;
  fetch_entries(first);
  if (first < end) load_tile(first);
  fetch_entries(first + kStep);
  for (long k0 = first; k0 < end; k0 += kStep) {
    // this tile out of the load registers: V to LDS, K to operands
    bool oks[2];
    bf16x8 ka[2][KS];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const bf16x8 v8 = row_bf16(vr[i], vsc[i]);
      *reinterpret_cast<u16x8*>(&sv[(vrow + RPL * i) * VP + (lane % CPR) * 8]) = __builtin_bit_cast(u16x8, v8);
    }
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      oks[c] = okh[c];
#pragma unroll
      for (int s = 0; s < KS; ++s) ka[c][s] = row_bf16(kr[c][s], ksc[c]);
    }
    wave_lds_fence();
    if (k0 + kStep < end) {  // in flight under the arithmetic below
      load_tile(k0 + kStep);
      fetch_entries(k0 + 2 * kStep);
    }

    // S^T = K Q^T: s[c][reg] is key k0 + 16 c + 4 lh + reg against query lq
    f32x4 s[2];
    float mt = -INFINITY;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      s[c] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) s[c] = mfma16(ka[c][ks], qf[ks], s[c]);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool vis = k0 + 16 * c + 4 * lh + e < end && oks[c];
        s[c][e] = vis ? s[c][e] * p.scale_log2 : -INFINITY;
        mt = fmaxf(mt, s[c][e]);
      }
    }
    mt = fmaxf(mt, __shfl_xor(mt, 16, 64));
    mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
    const float mn = fmaxf(m, mt);
    const float ms = mn == -INFINITY ? 0.f : mn;  // no key yet: every weight below is exp2(-inf) = 0
    const float alpha = __builtin_amdgcn_exp2f(m - ms);
    float ps = 0.f;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        s[c][e] = __builtin_amdgcn_exp2f(s[c][e] - ms);
        ps += s[c][e];
      }
    }
    ps += __shfl_xor(ps, 16, 64);
    ps += __shfl_xor(ps, 32, 64);
    l = l * alpha + ps;
    m = mn;
    // P rounded to bf16 once: the B operand of the tile's one k-step
    bf16x8 pf;
#pragma unroll
    for (int j = 0; j < 8; ++j) pf[j] = (__bf16)s[j >> 2][j & 3];
    // O^T = V^T P^T: acc[db][reg] is element 16 db + 4 lh + reg of query lq
    const u16* vt = sv + (4 * lh + (lq >> 2)) * VP + 4 * (lq & 3);
#pragma unroll
    for (int db = 0; db < DB; ++db) {
      const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(vt + 16 * db));
      const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(vt + 16 * VP + 16 * db));
      const s16x8 a = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
      acc[db] = mfma16(__builtin_bit_cast(bf16x8, a), pf, acc[db] * alpha);
    }
    wave_lds_fence();
  }

  // the wave's partial into its own region (its V reads are behind it), then the four waves
  // -> this split's partial, plain stores
  float* s_acc = reinterpret_cast<float*>(sv);  // [16][D]
#pragma unroll
  for (int db = 0; db < DB; ++db) *reinterpret_cast<f32x4*>(&s_acc[lq * D + 16 * db + 4 * lh]) = acc[db];
  if (lh == 0) {
    s_ml[wave][lq][0] = m;
    s_ml[wave][lq][1] = l;
  }
  __syncthreads();
  float* ws_ml = p.ws;
  float* ws_acc = p.ws + (long)p.B * p.Hq * p.ns * 2;
  for (int e = tid; e < G * D; e += kThreads) {
    const int g = e / D, d = e % D;
    float mn = s_ml[0][g][0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) mn = fmaxf(mn, s_ml[w][g][0]);
    float ls = 0.f, as = 0.f;
    if (mn != -INFINITY) {
#pragma unroll
      for (int w = 0; w < kWaves; ++w) {
        const float wt = __builtin_amdgcn_exp2f(s_ml[w][g][0] - mn);
        ls += s_ml[w][g][1] * wt;
        as += reinterpret_cast<const float*>(sV[w])[g * D + d] * wt;
      }
    }
    const long slot = ((long)b * p.Hq + hk * G + g) * p.ns + split;
    ws_acc[slot * D + d] = as;
    if (d == 0) {
      ws_ml[slot * 2] = mn;
      ws_ml[slot * 2 + 1] = ls;
    }
  }
}

template <int D>
static void launch(const DecodeParams& p, hipStream_t st) {
  const dim3 grid(p.ns, p.Hk, p.B), block(kThreads);
  const bool f8 = p.ks != nullptr;
  if (p.table != nullptr) {
    if (f8) hipLaunchKernelGGL((attn_decode_gqa_kernel<D, true, true>), grid, block, 0, st, p);
    else hipLaunchKernelGGL((attn_decode_gqa_kernel<D, true, false>), grid, block, 0, st, p);
  } else {
    if (f8) hipLaunchKernelGGL((attn_decode_gqa_kernel<D, false, true>), grid, block, 0, st, p);
    else hipLaunchKernelGGL((attn_decode_gqa_kernel<D, false, false>), grid, block, 0, st, p);
  }
}

}  // namespace gqa

void launch_decode_gqa(const DecodeParams& p, int D, hipStream_t st) {
  if (D == 128) gqa::launch<128>(p, st);
  else gqa::launch<64>(p, st);
}

}  // namespace dec
