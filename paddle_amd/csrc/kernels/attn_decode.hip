// KV-cache decode path for gfx950: cache append (+ rotary at a position offset) and
// split-KV single-token attention.
//
//   pa_kv_append    qkv [B, T, (Hq+2Hk)*D] bf16  ->  q_out [B, T, Hq, D], and k / v written
//                   into k_cache / v_cache [B, S_max, Hk, D] at rows pos[b] + t.  q and k
//                   are rotated (neox half split) at their true positions from the fp32
//                   cos / sin tables; v is copied bit for bit.  Memory bound: 16-byte
//                   loads / stores, table look-ups, no device trig.
//   pa_attn_decode  one query token per row against kv_len[b] cached keys.  Memory-bound
//                   KV read: one workgroup per (row, kv head, split); the Hq/Hk query rows
//                   of a GQA group share every K / V load; K and V go straight from global
//                   memory to registers (16 B per lane); the online softmax runs in fp32.
//                   Each split stores a partial (m, l, acc[D]) with plain stores and a
//                   second kernel merges the splits and writes bf16.
//   pa_kv_append_paged / pa_attn_decode_paged
//                   the same two kernels over a paged cache: k / v pools
//                   [num_blocks, block_size, Hk, D] and an int32 block table
//                   [B, max_blocks] (-1: unassigned) shared by all layers.  Token n of row
//                   b lives at pool[table[b][n / block_size]][n % block_size].  They are
//                   the same kernel bodies with the address of a cache row as a compile-time
//                   policy, so for equal inputs the paged and the contiguous attention
//                   return identical bits.  A table entry outside [0, num_blocks) is never
//                   dereferenced: the append drops the token, the attention masks the key.
//   pa_kv_append_f8 / pa_kv_append_paged_f8 / pa_attn_decode_f8 / pa_attn_decode_paged_f8
//                   the same kernel bodies over an e4m3 cache: the storage type is a second
//                   compile-time policy.  k / v hold one code per element in today's layout
//                   and k_scale / v_scale one power-of-two fp32 scale per (token, kv head),
//                   addressed like the codes.  The append forms the bf16 value the bf16
//                   kernel would store (the shared rotation, one rounding) and quantises it:
//                   amax over the D elements (NaN ignored), scale = 2^e with e the exponent
//                   of amax minus 8, plus one when its mantissa is above 1.75, clamped to
//                   [-100, 100] (1 for a zero vector), code = rne(x / scale) clamped to
//                   +-448, NaN kept.  The attention turns a code into cvt(code) * scale,
//                   which is exact, and then runs the arithmetic of the bf16 kernel in the
//                   same order: for equal q, kv_len and num_splits it returns the bits of
//                   pa_attn_decode over a bf16 cache that holds the dequantised values.
//
// Ordering: the two launches on one stream are the only ordering between workgroups --
// no flags, spins, arrival counters or float atomics, so the result does not depend on
// workgroup placement and is bit-identical from run to run.
//
// Lane layout of the decode kernel: a key row of D bf16 is covered by LG = D/8 adjacent
// lanes (8 elements = one 16-byte load each), so a wave holds KPW = 64/LG keys per load
// and a dot product is reduced over LG lanes only.  Every lane group keeps its own
// online-softmax state over the keys it visits; the groups of a wave are merged by
// shuffles and the four waves through LDS once at the end.
#include <type_traits>

#include "common.h"

using namespace pa;

namespace dec {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kUnroll = 4;  // keys per lane group in flight (2 * kUnroll 16-byte loads per lane)
constexpr int kMaxSplits = 64;
constexpr float kE4M3Max = 448.f;

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

// ------------------------------------------------------------------ kv append
struct AppendParams {
  const u16* qkv;
  long sb, st, sh;  // element strides of the [B, T, Hq+2Hk, D] view of qkv
  const int* pos;
  const float* cosT;
  const float* sinT;
  int max_pos;
  u16* kc;
  u16* vc;
  int S_max;
  u16* q_out;
  int B, T, Hq, Hk, D;
  // paged only: kc / vc are pools [num_blocks, 1 << bs_shift, Hk, D]
  const int* rows;   // [B] input row -> cache row, or null: the identity
  const int* table;  // [Bc, max_blocks]
  int Bc, max_blocks, num_blocks, bs_shift;
  // e4m3 only: kc / vc hold one byte per element, ks / vs one scale per (slot, kv head)
  float* ks;
  float* vs;
};

// The rotation of one lane's two 8-element chunks [a | b] -> [a*c - b*s | b*c + a*s]: one
// piece of code for every storage policy, so what a policy rounds to bf16 is the same.
__device__ __forceinline__ void rope_chunks(const u16x8& va, const u16x8& vb, const float* cosr, const float* sinr,
                                            float (&oa)[8], float (&ob)[8]) {
  float cs[8], sn[8];
  load8(cosr, cs);
  load8(sinr, sn);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float a = bf2f(va[j]), bb = bf2f(vb[j]);
    oa[j] = a * cs[j] - bb * sn[j];
    ob[j] = bb * cs[j] + a * sn[j];
  }
}

// |x| of 8 bf16 as integers (the order of the bits is the order of the values); NaN: 0
__device__ __forceinline__ uint32_t amax_bits8(const u16x8& v, uint32_t am) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const uint32_t a = v[j] & 0x7FFFu;
    am = max(am, a > 0x7F80u ? 0u : a);
  }
  return am;
}

// 8 bf16 times a power of two -> 8 e4m3 codes.  The clamp is two selects, not fminf /
// fmaxf: a NaN fails both comparisons and stays a NaN code.
__device__ __forceinline__ u32x2 quant8_f8(const u16x8& v, float inv) {
  float f[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float x = bf2f(v[j]) * inv;
    x = x > kE4M3Max ? kE4M3Max : x;
    x = x < -kE4M3Max ? -kE4M3Max : x;
    f[j] = x;
  }
  u32x2 w;
#pragma unroll
  for (int d = 0; d < 2; ++d) {
    int c4 = __builtin_amdgcn_cvt_pk_fp8_f32(f[4 * d], f[4 * d + 1], 0, false);
    c4 = __builtin_amdgcn_cvt_pk_fp8_f32(f[4 * d + 2], f[4 * d + 3], c4, true);
    w[d] = (uint32_t)c4;
  }
  return w;
}

// Quantise the vector of D bf16 whose chunks ra (at c * 8) and rb (at half + c * 8) this
// lane holds; the other chunks are in the cpr - 1 neighbouring lanes of its group (cpr a
// power of two, groups aligned: the caller's loop index is c modulo cpr).  Every lane of a
// group gets here or none does.  Two 8-byte stores of codes per lane, the scale from lane 0.
__device__ __forceinline__ void quant_store_f8(const u16x8& ra, const u16x8& rb, int cpr, int c, int half,
                                               uint8_t* codes, float* scale) {
  uint32_t am = amax_bits8(rb, amax_bits8(ra, 0u));
  for (int x = 1; x < cpr; x <<= 1) am = max(am, (uint32_t)__shfl_xor((int)am, x, 64));
  // amax = m * 2^E (m in [1, 2), 7 mantissa bits): 448 = 1.75 * 2^8
  int e = (int)(am >> 7) - 127 - 8 + ((am & 0x7Fu) > 0x60u ? 1 : 0);
  e = e < -100 ? -100 : (e > 100 ? 100 : e);
  if (am == 0u) e = 0;
  const float inv = __uint_as_float((uint32_t)(127 - e) << 23);
  *reinterpret_cast<u32x2*>(codes + c * 8) = quant8_f8(ra, inv);
  *reinterpret_cast<u32x2*>(codes + half + c * 8) = quant8_f8(rb, inv);
  if (c == 0) *scale = __uint_as_float((uint32_t)(127 + e) << 23);
}

template <bool Paged, bool F8>
__global__ __launch_bounds__(256) void kv_append_kernel(AppendParams p) {
  const int half = p.D >> 1;
  const int cpr = half >> 3;  // 8-element chunks per half row
  const int nh = p.Hq + 2 * p.Hk;
  const long total = (long)p.B * p.T * nh * cpr;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i % cpr);
    long r = i / cpr;
    const int h = (int)(r % nh);
    r /= nh;
    const int t = (int)(r % p.T);
    const int b = (int)(r / p.T);
    int cb = b;  // the cache row this input row goes to
    if constexpr (Paged) {
      if (p.rows != nullptr) cb = p.rows[b];
    }
    const bool row_ok = !Paged || (cb >= 0 && cb < p.Bc);
    const long position = row_ok ? (long)p.pos[cb] + t : -1;
    const bool rot = p.cosT != nullptr && h < p.Hq + p.Hk;
    const bool ok = position >= 0 && position < p.S_max && (p.cosT == nullptr || position < p.max_pos);
    u16* dst;
    uint8_t* codes = nullptr;  // e4m3, k / v heads only
    float* scale = nullptr;
    if (h < p.Hq) {
      dst = p.q_out + (((long)b * p.T + t) * p.Hq + h) * p.D;
    } else {
      if (!ok) continue;  // never written: the slot does not exist
      const bool isk = h < p.Hq + p.Hk;
      const int hk = isk ? h - p.Hq : h - p.Hq - p.Hk;
      long slot;  // the token's row in the cache, in units of Hk * D elements
      if constexpr (Paged) {
        // position < S_max <= max_blocks << bs_shift: the table read is in range
        const int blk = p.table[(long)cb * p.max_blocks + (position >> p.bs_shift)];
        if (blk < 0 || blk >= p.num_blocks) continue;  // no block assigned: dropped
        slot = ((long)blk << p.bs_shift) + (position & ((1L << p.bs_shift) - 1));
      } else {
        slot = (long)b * p.S_max + position;
      }
      if constexpr (F8) {
        dst = nullptr;
        codes = reinterpret_cast<uint8_t*>(isk ? p.kc : p.vc) + (slot * p.Hk + hk) * p.D;
        scale = (isk ? p.ks : p.vs) + (slot * p.Hk + hk);
      } else {
        dst = (isk ? p.kc : p.vc) + (slot * p.Hk + hk) * p.D;
      }
    }
    if (!ok) {  // q of a token that has no position: zeros
      const u16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
      *reinterpret_cast<u16x8*>(dst + c * 8) = z;
      *reinterpret_cast<u16x8*>(dst + half + c * 8) = z;
      continue;
    }
    const u16* src = p.qkv + (long)b * p.sb + (long)t * p.st + (long)h * p.sh;
    const u16x8 va = *reinterpret_cast<const u16x8*>(src + c * 8);
    const u16x8 vb = *reinterpret_cast<const u16x8*>(src + half + c * 8);
    if constexpr (F8) {
      if (h >= p.Hq) {  // uniform over the cpr lanes of a vector: (b, t, h) decide every branch above
        u16x8 ra = va, rb = vb;  // the bits the bf16 cache would hold
        if (rot) {
          float oa[8], ob[8];
          rope_chunks(va, vb, p.cosT + position * half + c * 8, p.sinT + position * half + c * 8, oa, ob);
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            ra[j] = f2bf(oa[j]);
            rb[j] = f2bf(ob[j]);
          }
        }
        quant_store_f8(ra, rb, cpr, c, half, codes, scale);
        continue;
      }
    }
    if (!rot) {
      *reinterpret_cast<u16x8*>(dst + c * 8) = va;
      *reinterpret_cast<u16x8*>(dst + half + c * 8) = vb;
      continue;
    }
    float oa[8], ob[8];
    rope_chunks(va, vb, p.cosT + position * half + c * 8, p.sinT + position * half + c * 8, oa, ob);
    store8(dst + c * 8, oa);
    store8(dst + half + c * 8, ob);
  }
}

__global__ void i32_add_kernel(int* x, int n, int inc) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) x[i] += inc;
}

// ------------------------------------------------------------------ decode attention
struct DecodeParams {
  const u16* q;
  long qsb, qsh;  // element strides of q [B, 1, Hq, D] over b and head
  const u16* kc;
  const u16* vc;
  const int* kv_len;
  float* ws;  // [B, Hq, ns, 2] (m, l) then [B, Hq, ns, D] acc
  u16* o;     // [B, 1, Hq, D] contiguous
  int B, S_max, Hq, Hk, ns;
  float scale_log2;  // scale * log2(e): scores live in the log2 domain
  // paged only: kc / vc are pools [num_blocks, 1 << bs_shift, Hk, D]
  const int* table;  // [B, max_blocks]
  int max_blocks, num_blocks, bs_shift;
  // e4m3 only: kc / vc hold one byte per element, ks / vs one scale per (slot, kv head)
  const float* ks;
  const float* vs;
};

// The 8 elements of a key row one lane holds, as floats.  bf16: the bits shifted up.
// e4m3: cvt(code) * scale, exact for the append's power-of-two scales (4 significant bits,
// exponent within [-109, 109]), so the arithmetic downstream sees what a bf16 cache
// holding the dequantised values would give it.
__device__ __forceinline__ void row_floats(const u16x8& r, float, float (&f)[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) f[j] = bf2f(r[j]);
}
__device__ __forceinline__ void row_floats(const u32x2& r, float sc, float (&f)[8]) {
#pragma unroll
  for (int d = 0; d < 2; ++d) {
    const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)r[d], false) * sc;
    const f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)r[d], true) * sc;
    f[4 * d] = lo.x;
    f[4 * d + 1] = lo.y;
    f[4 * d + 2] = hi.x;
    f[4 * d + 3] = hi.y;
  }
}

// merge the online-softmax state (m, l, acc) of another lane group into this one
template <int G>
__device__ __forceinline__ void merge_shfl(float (&m)[G], float (&l)[G], float (&acc)[G][8], int xr) {
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const float mo = __shfl_xor(m[g], xr, 64);
    const float lo = __shfl_xor(l[g], xr, 64);
    const float mn = fmaxf(m[g], mo);
    // both empty (mn = -inf): weights 0, the state stays (m = -inf, l = 0, acc = 0)
    const float wa = mn == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(m[g] - mn);
    const float wb = mn == -INFINITY ? 0.f : __builtin_amdgcn_exp2f(mo - mn);
    l[g] = l[g] * wa + lo * wb;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float ao = __shfl_xor(acc[g][j], xr, 64);
      acc[g][j] = acc[g][j] * wa + ao * wb;
    }
    m[g] = mn;
  }
}

// Paged: the table entry of key n of row b, unchecked (the range check waits until the
// entry is used, so this load needs no wait).  n < end <= S_max <= max_blocks << bs_shift
// keeps the read inside the row; a key at or beyond end reads entry 0 and is never used.
__device__ __forceinline__ int table_entry(const int* trow, long key, long end, int shift) {
  const long idx = key < end ? key >> shift : 0;
  return trow[idx];
}

// Paged = false: keys of row b at kc + (b * S_max + n) * Hk * D.  Paged = true: at
// kc + (table[b][n >> bs_shift] << bs_shift | n & (bs - 1)) * Hk * D.  Everything else --
// the chunking, the lane layout, the order of every floating-point operation -- is shared,
// so the two instantiations return the same bits for the same cached tokens.
//
// F8 = true: a key row is D e4m3 codes and one fp32 scale (ks / vs, indexed like the rows).
// The lane geometry stays -- 8 elements per lane, now one 8-byte load -- and so does every
// fp32 operation after row_floats().  Half the bytes per load means half the bytes in
// flight, so this policy holds R = 2 iterations in registers: the loads of the next iteration
// (the scale loads with them) are issued before the arithmetic on this one and stay in flight
// under it.  The loop starts one iteration early to load the first.  The iterations are
// attended to in the original order.
template <int D, int G, bool Paged, bool F8>
__global__ __launch_bounds__(kThreads) void attn_decode_kernel(DecodeParams p) {
  constexpr int LG = D / 8;          // lanes per key row
  constexpr int KPW = 64 / LG;       // keys per wave per load
  constexpr int WT = KPW * kUnroll;  // keys per wave per iteration
  constexpr int R = F8 ? 2 : 1;      // iterations held in registers
  constexpr int RL = F8 ? 1 : 0;     // how many iterations the loads run ahead of the arithmetic
  using Elt = typename std::conditional<F8, uint8_t, u16>::type;
  using Vec = typename std::conditional<F8, u32x2, u16x8>::type;  // 8 elements of a row
  __shared__ float s_ml[kWaves][G][2];
  __shared__ float s_acc[kWaves][G][D];

  const int split = blockIdx.x, hk = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = lane % LG, grp = lane / LG;

  int len = p.kv_len[b];
  len = len < 0 ? 0 : (len > p.S_max ? p.S_max : len);
  // this split's key range: equal chunks of the row's own length, whole wave tiles
  int chunk = (len + p.ns - 1) / p.ns;
  chunk = (chunk + WT - 1) / WT * WT;
  const long start = (long)split * chunk;
  const long end = start + chunk < (long)len ? start + chunk : (long)len;

  float qf[G][8];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    load8(p.q + (long)b * p.qsb + (long)(hk * G + g) * p.qsh + c * 8, qf[g]);
#pragma unroll
    for (int j = 0; j < 8; ++j) qf[g][j] *= p.scale_log2;
  }
  float m[G], l[G], acc[G][8];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    m[g] = -INFINITY;
    l[g] = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[g][j] = 0.f;
  }

  const long row = (long)p.Hk * D;  // elements between consecutive keys
  const Elt* kc = reinterpret_cast<const Elt*>(p.kc);
  const Elt* vc = reinterpret_cast<const Elt*>(p.vc);
  const Elt *kb, *vb;
  const float *ksb = nullptr, *vsb = nullptr;  // F8: the scales of this kv head, p.Hk floats per key
  if constexpr (Paged) {  // the pool: rows do not own a slab
    kb = kc + (long)hk * D + c * 8;
    vb = vc + (long)hk * D + c * 8;
    if constexpr (F8) {
      ksb = p.ks + hk;
      vsb = p.vs + hk;
    }
  } else {
    kb = kc + (long)b * p.S_max * row + (long)hk * D + c * 8;
    vb = vc + (long)b * p.S_max * row + (long)hk * D + c * 8;
    if constexpr (F8) {
      ksb = p.ks + (long)b * p.S_max * p.Hk + hk;
      vsb = p.vs + (long)b * p.S_max * p.Hk + hk;
    }
  }

  // Paged: the block ids of an iteration's keys are fetched one iteration ahead, so the
  // table look-up (a dependent load in front of each K / V load) is in flight together
  // with the previous iteration's 2 * kUnroll K / V loads and not on the critical path.
  const int* trow = Paged ? p.table + (long)b * p.max_blocks : nullptr;
  const long bmask = Paged ? (1L << p.bs_shift) - 1 : 0;
  constexpr long kStep = (long)kWaves * WT;  // keys between a wave's consecutive iterations
  int blk[kUnroll];  // the entries of the iteration loaded next
  if constexpr (Paged) {
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const long key = start + (long)wave * WT + u * KPW + grp;
      blk[u] = table_entry(trow, key, end, p.bs_shift);
    }
  }

  Vec kr[R][kUnroll], vr[R][kUnroll];  // outside the loop: F8 carries a slot into the next pass
  float ksc[R][kUnroll], vsc[R][kUnroll];
  bool valid[R][kUnroll];
  // One pass loads the iteration at k0 + RL * kStep into slot ld and attends to the iteration
  // at k0 in slot cp.  bf16: the same iteration, the same slot.  F8: the loaded iteration is
  // the next one, the two slots swap roles from pass to pass (R passes unrolled, so the slot
  // numbers are constants and nothing is copied), and the first pass only loads.
  for (long p0 = start + (long)wave * WT - RL * kStep; p0 < end; p0 += R * kStep) {
    if constexpr (F8) {
      if (start + (long)wave * WT >= end) break;  // no key for this wave: nothing to re-read either
    }
#pragma unroll
    for (int ph = 0; ph < R; ++ph) {
      const long k0 = p0 + ph * kStep;  // this pass
      if (ph > 0 && k0 >= end) break;
      const int ld = F8 ? 1 - ph : 0, cp = F8 ? ph : 0;
      int nblk[kUnroll];
      if constexpr (Paged) {
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
          const long key = k0 + (RL + 1) * kStep + u * KPW + grp;
          nblk[u] = table_entry(trow, key, end, p.bs_shift);
        }
      }
      {
        // past the range (F8, the last pass) every lane is masked and re-reads a key of the
        // iteration before; those rows are never attended to
        const long kit = k0 + RL * kStep;
        const long kref = kit < end ? kit : k0;
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
          const long key = kit + u * KPW + grp;
          long kk;
          if constexpr (Paged) {
            // a key whose entry is outside [0, num_blocks) is masked like a key at or beyond
            // end; its lane reads the first slot of the pool, which is always there
            valid[ld][u] = key < end && (unsigned)blk[u] < (unsigned)p.num_blocks;
            kk = valid[ld][u] ? ((long)blk[u] << p.bs_shift) + (key & bmask) : 0;
          } else {
            valid[ld][u] = key < end;
            // slots at or beyond the range are never read: a lane without a key re-reads the
            // iteration's first key (< end) and its score is masked to -inf below, so its
            // weight is exactly 0
            kk = valid[ld][u] ? key : kref;
          }
          kr[ld][u] = *reinterpret_cast<const Vec*>(kb + kk * row);
          vr[ld][u] = *reinterpret_cast<const Vec*>(vb + kk * row);
          if constexpr (F8) {
            ksc[ld][u] = ksb[kk * p.Hk];
            vsc[ld][u] = vsb[kk * p.Hk];
          } else {
            ksc[ld][u] = vsc[ld][u] = 1.f;  // unused
          }
        }
      }
      if constexpr (Paged || F8) {
        // keep all the loads ahead of the arithmetic: without this the scheduler sinks the
        // last one below the first score, where its latency is exposed
        __builtin_amdgcn_sched_barrier(0);
      }
      if (!F8 || k0 >= start + (long)wave * WT) {  // F8, the first pass: slot cp is empty
        if constexpr (Paged) {
          // What the pool's first slot holds (another row's token, inf, NaN) must not reach
          // 0 * v below: clear the v registers of a lane without a key -- and with e4m3 its v
          // scale, since 0 * an inf or NaN scale is not 0.  A mask, not a branch, and after the
          // last load is issued, so all the loads stay in flight.  (Its k needs nothing: the
          // score is replaced by -inf whatever it is.)
#pragma unroll
          for (int u = 0; u < kUnroll; ++u) {
            if constexpr (F8) {
              vr[cp][u] &= (u32x2)(valid[cp][u] ? 0xFFFFFFFFu : 0u);
              vsc[cp][u] = valid[cp][u] ? vsc[cp][u] : 0.f;
            } else {
              vr[cp][u] &= (u16x8)(u16)(valid[cp][u] ? 0xFFFF : 0);
            }
          }
        }
        float s[kUnroll][G];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
          float kf[8];
          row_floats(kr[cp][u], ksc[cp][u], kf);
#pragma unroll
          for (int g = 0; g < G; ++g) {
            float d = 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j) d = fmaf(qf[g][j], kf[j], d);
#pragma unroll
            for (int x = 1; x < LG; x <<= 1) d += __shfl_xor(d, x, 64);
            s[u][g] = valid[cp][u] ? d : -INFINITY;
          }
        }
        float vf[F8 ? kUnroll : 1][8];  // F8: dequantised once, not per query row
        if constexpr (F8) {
#pragma unroll
          for (int u = 0; u < kUnroll; ++u) row_floats(vr[cp][u], vsc[cp][u], vf[u]);
        }
#pragma unroll
        for (int g = 0; g < G; ++g) {
          float mt = s[0][g];
#pragma unroll
          for (int u = 1; u < kUnroll; ++u) mt = fmaxf(mt, s[u][g]);
          const float mn = fmaxf(m[g], mt);
          if (mn == -INFINITY) continue;  // this lane group has seen no key yet
          const float alpha = __builtin_amdgcn_exp2f(m[g] - mn);
          float pw[kUnroll], ps = 0.f;
#pragma unroll
          for (int u = 0; u < kUnroll; ++u) {
            pw[u] = __builtin_amdgcn_exp2f(s[u][g] - mn);
            ps += pw[u];
          }
          l[g] = l[g] * alpha + ps;
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            float a = acc[g][j] * alpha;
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {
              if constexpr (F8) a = fmaf(pw[u], vf[u][j], a);
              else a = fmaf(pw[u], bf2f(vr[cp][u][j]), a);
            }
            acc[g][j] = a;
          }
          m[g] = mn;
        }
      }
      if constexpr (Paged) {
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) blk[u] = nblk[u];
      }
    }
  }

  // lane groups of the wave -> one state (every lane of a group column ends up with it)
#pragma unroll
  for (int xr = LG; xr < 64; xr <<= 1) merge_shfl<G>(m, l, acc, xr);
  if (grp == 0) {
#pragma unroll
    for (int g = 0; g < G; ++g) {
      if (c == 0) {
        s_ml[wave][g][0] = m[g];
        s_ml[wave][g][1] = l[g];
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) s_acc[wave][g][c * 8 + j] = acc[g][j];
    }
  }
  __syncthreads();
  // the four waves -> this split's partial, plain stores
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
        as += s_acc[w][g][d] * wt;
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

// one block per (row, query head), one thread per output element
template <int D>
__global__ __launch_bounds__(D) void attn_decode_merge_kernel(DecodeParams p) {
  const long bh = blockIdx.x;
  const int d = threadIdx.x;
  const float* ws_ml = p.ws + bh * p.ns * 2;
  const float* ws_acc = p.ws + (long)p.B * p.Hq * p.ns * 2 + bh * p.ns * D;
  float mn = -INFINITY;
  for (int s = 0; s < p.ns; ++s) mn = fmaxf(mn, ws_ml[s * 2]);
  float ls = 0.f, as = 0.f;
  if (mn != -INFINITY) {
    for (int s = 0; s < p.ns; ++s) {
      const float wt = __builtin_amdgcn_exp2f(ws_ml[s * 2] - mn);  // empty split: exp2(-inf) = 0
      ls += ws_ml[s * 2 + 1] * wt;
      as += ws_acc[(long)s * D + d] * wt;
    }
  }
  p.o[bh * D + d] = f2bf(ls > 0.f ? as / ls : 0.f);  // kv_len == 0: zeros
}

template <bool Paged>
static void launch_append(const AppendParams& p, bool f8, hipStream_t st) {
  const long items = (long)p.B * p.T * (p.Hq + 2 * p.Hk) * (p.D / 16);
  const dim3 grid(stream_grid(items, 256));
  if (f8) hipLaunchKernelGGL((kv_append_kernel<Paged, true>), grid, dim3(256), 0, st, p);
  else hipLaunchKernelGGL((kv_append_kernel<Paged, false>), grid, dim3(256), 0, st, p);
}

template <int D, bool Paged, bool F8>
static void launch_decode(const DecodeParams& p, hipStream_t st) {
  const dim3 grid(p.ns, p.Hk, p.B);
  switch (p.Hq / p.Hk) {
    case 1: hipLaunchKernelGGL((attn_decode_kernel<D, 1, Paged, F8>), grid, dim3(kThreads), 0, st, p); break;
    case 2: hipLaunchKernelGGL((attn_decode_kernel<D, 2, Paged, F8>), grid, dim3(kThreads), 0, st, p); break;
    case 4: hipLaunchKernelGGL((attn_decode_kernel<D, 4, Paged, F8>), grid, dim3(kThreads), 0, st, p); break;
    default: hipLaunchKernelGGL((attn_decode_kernel<D, 8, Paged, F8>), grid, dim3(kThreads), 0, st, p); break;
  }
  hipLaunchKernelGGL((attn_decode_merge_kernel<D>), dim3(p.B * p.Hq), dim3(D), 0, st, p);
}

}  // namespace dec

// log2 of a paged cache's block size, or -1 when it is not one of 16, 32, 64, 128, 256
static int paged_block_shift(int block_size) {
  for (int s = 4; s <= 8; ++s)
    if (block_size == (1 << s)) return s;
  return -1;
}

// The two appends behind their four entry points.  k_scale null: a bf16 cache.
static int append_contiguous(const void* qkv, const long* strides, const int* pos, const float* cosT,
                             const float* sinT, int max_pos, void* k_cache, void* v_cache, float* k_scale,
                             float* v_scale, int S_max, void* q_out, int B, int T, int Hq, int Hk, int D,
                             hipStream_t st) {
  if (B <= 0 || T <= 0 || Hq <= 0 || Hk <= 0 || D <= 0 || D % 16 || S_max <= 0) return (int)hipErrorInvalidValue;
  if ((cosT == nullptr) != (sinT == nullptr)) return (int)hipErrorInvalidValue;
  for (int i = 0; i < 3; ++i)
    if (strides[i] % 8) return (int)hipErrorInvalidValue;  // 16-byte rows
  dec::AppendParams p;
  p.qkv = (const u16*)qkv;
  p.sb = strides[0]; p.st = strides[1]; p.sh = strides[2];
  p.pos = pos; p.cosT = cosT; p.sinT = sinT; p.max_pos = max_pos;
  p.kc = (u16*)k_cache; p.vc = (u16*)v_cache; p.S_max = S_max; p.q_out = (u16*)q_out;
  p.B = B; p.T = T; p.Hq = Hq; p.Hk = Hk; p.D = D;
  p.rows = nullptr; p.table = nullptr; p.Bc = B; p.max_blocks = 0; p.num_blocks = 0; p.bs_shift = 0;
  p.ks = k_scale; p.vs = v_scale;
  dec::launch_append<false>(p, k_scale != nullptr, st);
  PA_LAUNCH_CHECK();
}

static int append_paged(const void* qkv, const long* strides, const int* pos, const int* rows, const float* cosT,
                        const float* sinT, int max_pos, void* k_pool, void* v_pool, float* k_scale, float* v_scale,
                        const int* table, int max_blocks, int num_blocks, int block_size, int S_max, void* q_out,
                        int B, int Bc, int T, int Hq, int Hk, int D, hipStream_t st) {
  if (B <= 0 || Bc <= 0 || T <= 0 || Hq <= 0 || Hk <= 0 || D <= 0 || D % 16 || S_max <= 0) return (int)hipErrorInvalidValue;
  if ((cosT == nullptr) != (sinT == nullptr)) return (int)hipErrorInvalidValue;
  const int shift = paged_block_shift(block_size);
  if (shift < 0 || num_blocks <= 0 || table == nullptr || (rows == nullptr && B != Bc)) return (int)hipErrorInvalidValue;
  if (max_blocks <= 0 || ((long)max_blocks << shift) < (long)S_max) return (int)hipErrorInvalidValue;  // table covers S_max
  for (int i = 0; i < 3; ++i)
    if (strides[i] % 8) return (int)hipErrorInvalidValue;  // 16-byte rows
  dec::AppendParams p;
  p.qkv = (const u16*)qkv;
  p.sb = strides[0]; p.st = strides[1]; p.sh = strides[2];
  p.pos = pos; p.cosT = cosT; p.sinT = sinT; p.max_pos = max_pos;
  p.kc = (u16*)k_pool; p.vc = (u16*)v_pool; p.S_max = S_max; p.q_out = (u16*)q_out;
  p.B = B; p.T = T; p.Hq = Hq; p.Hk = Hk; p.D = D;
  p.rows = rows; p.table = table; p.Bc = Bc; p.max_blocks = max_blocks; p.num_blocks = num_blocks; p.bs_shift = shift;
  p.ks = k_scale; p.vs = v_scale;
  dec::launch_append<true>(p, k_scale != nullptr, st);
  PA_LAUNCH_CHECK();
}

// strides: element strides of the [B, T, Hq+2Hk, D] view of the packed projection over
// (b, t, head); unit stride on D.  cos / sin null: no rotation.
PA_EXPORT int pa_kv_append(const void* qkv, const long* strides /*3*/, const int* pos, const float* cosT,
                           const float* sinT, int max_pos, void* k_cache, void* v_cache, int S_max, void* q_out,
                           int B, int T, int Hq, int Hk, int D, hipStream_t st) {
  return append_contiguous(qkv, strides, pos, cosT, sinT, max_pos, k_cache, v_cache, nullptr, nullptr, S_max, q_out,
                           B, T, Hq, Hk, D, st);
}

// pa_kv_append into a paged cache: k_pool / v_pool [num_blocks, block_size, Hk, D], table
// [Bc, max_blocks] int32, pos [Bc].  Input row b goes to cache row rows[b] (rows null: b,
// and then B == Bc).  The token at position pos[row] + t lands in block
// table[row][position / block_size]; it is dropped when the position is >= S_max (or past
// the rotary table) or when that entry is outside [0, num_blocks).
PA_EXPORT int pa_kv_append_paged(const void* qkv, const long* strides /*3*/, const int* pos, const int* rows,
                                 const float* cosT, const float* sinT, int max_pos, void* k_pool, void* v_pool,
                                 const int* table, int max_blocks, int num_blocks, int block_size, int S_max,
                                 void* q_out, int B, int Bc, int T, int Hq, int Hk, int D, hipStream_t st) {
  return append_paged(qkv, strides, pos, rows, cosT, sinT, max_pos, k_pool, v_pool, nullptr, nullptr, table,
                      max_blocks, num_blocks, block_size, S_max, q_out, B, Bc, T, Hq, Hk, D, st);
}

// Whether the e4m3 appends take a head size: the D / 16 lanes of a vector reduce its amax
// with shuffles, so they are a power of two inside one wave.
PA_EXPORT int pa_kv_append_f8_ok(int D) {
  if (D <= 0 || D % 16) return 0;
  const int cpr = D / 16;
  return cpr <= 64 && (cpr & (cpr - 1)) == 0;
}

PA_EXPORT int pa_kv_append_paged_f8_ok(int D, int block_size) {
  return pa_kv_append_f8_ok(D) && paged_block_shift(block_size) >= 0;
}

// pa_kv_append into an e4m3 cache: k_codes / v_codes [B, S_max, Hk, D] one byte each,
// k_scale / v_scale [B, S_max, Hk] fp32.  q_out is what pa_kv_append writes; a k / v vector
// is the value pa_kv_append would store, quantised (see the head of the file).
PA_EXPORT int pa_kv_append_f8(const void* qkv, const long* strides /*3*/, const int* pos, const float* cosT,
                              const float* sinT, int max_pos, void* k_codes, void* v_codes, float* k_scale,
                              float* v_scale, int S_max, void* q_out, int B, int T, int Hq, int Hk, int D,
                              hipStream_t st) {
  if (!pa_kv_append_f8_ok(D) || k_scale == nullptr || v_scale == nullptr) return (int)hipErrorInvalidValue;
  return append_contiguous(qkv, strides, pos, cosT, sinT, max_pos, k_codes, v_codes, k_scale, v_scale, S_max, q_out,
                           B, T, Hq, Hk, D, st);
}

// pa_kv_append_paged into an e4m3 pool: codes [num_blocks, block_size, Hk, D], scales
// [num_blocks, block_size, Hk].  A dropped token writes neither.
PA_EXPORT int pa_kv_append_paged_f8(const void* qkv, const long* strides /*3*/, const int* pos, const int* rows,
                                    const float* cosT, const float* sinT, int max_pos, void* k_codes, void* v_codes,
                                    float* k_scale, float* v_scale, const int* table, int max_blocks, int num_blocks,
                                    int block_size, int S_max, void* q_out, int B, int Bc, int T, int Hq, int Hk,
                                    int D, hipStream_t st) {
  if (!pa_kv_append_paged_f8_ok(D, block_size) || k_scale == nullptr || v_scale == nullptr)
    return (int)hipErrorInvalidValue;
  return append_paged(qkv, strides, pos, rows, cosT, sinT, max_pos, k_codes, v_codes, k_scale, v_scale, table,
                      max_blocks, num_blocks, block_size, S_max, q_out, B, Bc, T, Hq, Hk, D, st);
}

// x[i] += inc over n int32 (the cache's per-row lengths), on the stream
PA_EXPORT int pa_i32_add(int* x, int n, int inc, hipStream_t st) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(dec::i32_add_kernel, dim3((n + 255) / 256), dim3(256), 0, st, x, n, inc);
  PA_LAUNCH_CHECK();
}

// Whether pa_attn_decode takes this problem (else the caller runs its reference path).
PA_EXPORT int pa_attn_decode_ok(int B, int S_max, int Hq, int Hk, int D, int num_splits, const long* qstrides /*2*/) {
  if (B <= 0 || B > 65535 || S_max <= 0 || Hq <= 0 || Hk <= 0 || Hk > 65535 || Hq % Hk) return 0;
  if (D != 64 && D != 128) return 0;
  const int g = Hq / Hk;
  if (g != 1 && g != 2 && g != 4 && g != 8) return 0;
  if (num_splits < 1 || num_splits > dec::kMaxSplits) return 0;
  if (qstrides[0] % 8 || qstrides[1] % 8) return 0;
  return 1;
}

// Split count from the launch shape alone (never from kv_len: no host read per step):
// enough workgroups for two per compute unit, at least 256 keys per split.
PA_EXPORT int pa_attn_decode_splits(int B, int Hk, int S_max) {
  long want = (512 + (long)B * Hk - 1) / ((long)B * Hk);
  long cap = S_max / 256;
  if (want > cap) want = cap;
  if (want > dec::kMaxSplits) want = dec::kMaxSplits;
  return want < 1 ? 1 : (int)want;
}

// Whether pa_attn_decode_paged takes this problem: what pa_attn_decode takes, a block size
// of 16..256 (a power of two) and a table that covers S_max.
PA_EXPORT int pa_attn_decode_paged_ok(int B, int S_max, int Hq, int Hk, int D, int num_splits,
                                      const long* qstrides /*2*/, int block_size, int max_blocks, int num_blocks) {
  if (!pa_attn_decode_ok(B, S_max, Hq, Hk, D, num_splits, qstrides)) return 0;
  const int shift = paged_block_shift(block_size);
  if (shift < 0 || num_blocks <= 0 || max_blocks <= 0) return 0;
  if (((long)max_blocks << shift) < (long)S_max) return 0;
  return 1;
}

// The e4m3 kernels take the problems the bf16 ones take.
PA_EXPORT int pa_attn_decode_f8_ok(int B, int S_max, int Hq, int Hk, int D, int num_splits, const long* qstrides /*2*/) {
  return pa_attn_decode_ok(B, S_max, Hq, Hk, D, num_splits, qstrides);
}

PA_EXPORT int pa_attn_decode_paged_f8_ok(int B, int S_max, int Hq, int Hk, int D, int num_splits,
                                         const long* qstrides /*2*/, int block_size, int max_blocks, int num_blocks) {
  return pa_attn_decode_paged_ok(B, S_max, Hq, Hk, D, num_splits, qstrides, block_size, max_blocks, num_blocks);
}

// The two attentions behind their four entry points.  k_scale null: a bf16 cache; table
// null: a contiguous one (the callers have checked the problem).
static int decode_launch(const void* q, const long* qstrides, const void* k, const void* v, const float* k_scale,
                         const float* v_scale, const int* table, int max_blocks, int num_blocks, int block_size,
                         const int* kv_len, void* o, float* ws, int B, int S_max, int Hq, int Hk, int D, float scale,
                         int num_splits, hipStream_t st) {
  dec::DecodeParams p;
  p.q = (const u16*)q; p.qsb = qstrides[0]; p.qsh = qstrides[1];
  p.kc = (const u16*)k; p.vc = (const u16*)v; p.kv_len = kv_len;
  p.ws = ws; p.o = (u16*)o;
  p.B = B; p.S_max = S_max; p.Hq = Hq; p.Hk = Hk; p.ns = num_splits;
  p.scale_log2 = scale * 1.4426950408889634f;
  p.table = table; p.max_blocks = max_blocks; p.num_blocks = num_blocks;
  p.bs_shift = table != nullptr ? paged_block_shift(block_size) : 0;
  p.ks = k_scale; p.vs = v_scale;
  const bool f8 = k_scale != nullptr;
  if (table != nullptr) {
    if (f8) {
      if (D == 128) dec::launch_decode<128, true, true>(p, st);
      else dec::launch_decode<64, true, true>(p, st);
    } else {
      if (D == 128) dec::launch_decode<128, true, false>(p, st);
      else dec::launch_decode<64, true, false>(p, st);
    }
  } else if (f8) {
    if (D == 128) dec::launch_decode<128, false, true>(p, st);
    else dec::launch_decode<64, false, true>(p, st);
  } else {
    if (D == 128) dec::launch_decode<128, false, false>(p, st);
    else dec::launch_decode<64, false, false>(p, st);
  }
  PA_LAUNCH_CHECK();
}

PA_EXPORT int pa_attn_decode(const void* q, const long* qstrides /*2: b, head*/, const void* k_cache,
                             const void* v_cache, const int* kv_len, void* o, float* ws /*B*Hq*num_splits*(D+2)*/, int B, int S_max, int Hq,
                             int Hk, int D, float scale, int num_splits, hipStream_t st) {
  if (!pa_attn_decode_ok(B, S_max, Hq, Hk, D, num_splits, qstrides)) return (int)hipErrorInvalidValue;
  return decode_launch(q, qstrides, k_cache, v_cache, nullptr, nullptr, nullptr, 0, 0, 0, kv_len, o, ws, B, S_max, Hq,
                       Hk, D, scale, num_splits, st);
}

// pa_attn_decode over a paged cache (k_pool / v_pool [num_blocks, block_size, Hk, D],
// table [B, max_blocks] int32): the same bits as pa_attn_decode over a contiguous cache
// that holds the same tokens, for the same kv_len and num_splits.
PA_EXPORT int pa_attn_decode_paged(const void* q, const long* qstrides /*2: b, head*/, const void* k_pool,
                                   const void* v_pool, const int* table, int max_blocks, int num_blocks,
                                   int block_size, const int* kv_len, void* o, float* ws /*B*Hq*num_splits*(D+2)*/,
                                   int B, int S_max, int Hq, int Hk, int D, float scale, int num_splits,
                                   hipStream_t st) {
  if (!pa_attn_decode_paged_ok(B, S_max, Hq, Hk, D, num_splits, qstrides, block_size, max_blocks, num_blocks) ||
      table == nullptr)
    return (int)hipErrorInvalidValue;
  return decode_launch(q, qstrides, k_pool, v_pool, nullptr, nullptr, table, max_blocks, num_blocks, block_size,
                       kv_len, o, ws, B, S_max, Hq, Hk, D, scale, num_splits, st);
}

// pa_attn_decode over an e4m3 cache (k_codes / v_codes [B, S_max, Hk, D] one byte each,
// k_scale / v_scale [B, S_max, Hk] fp32): the bits of pa_attn_decode over a bf16 cache
// that holds codes * scale, for the same q, kv_len and num_splits.
PA_EXPORT int pa_attn_decode_f8(const void* q, const long* qstrides /*2: b, head*/, const void* k_codes,
                                const void* v_codes, const float* k_scale, const float* v_scale, const int* kv_len,
                                void* o, float* ws /*B*Hq*num_splits*(D+2)*/, int B, int S_max, int Hq, int Hk,
                                int D, float scale, int num_splits, hipStream_t st) {
  if (!pa_attn_decode_f8_ok(B, S_max, Hq, Hk, D, num_splits, qstrides) || k_scale == nullptr || v_scale == nullptr)
    return (int)hipErrorInvalidValue;
  return decode_launch(q, qstrides, k_codes, v_codes, k_scale, v_scale, nullptr, 0, 0, 0, kv_len, o, ws, B, S_max,
                       Hq, Hk, D, scale, num_splits, st);
}

// pa_attn_decode_f8 over a paged e4m3 cache (codes [num_blocks, block_size, Hk, D], scales
// [num_blocks, block_size, Hk]): the bits of pa_attn_decode_f8 for the same cached tokens.
PA_EXPORT int pa_attn_decode_paged_f8(const void* q, const long* qstrides /*2: b, head*/, const void* k_codes,
                                      const void* v_codes, const float* k_scale, const float* v_scale,
                                      const int* table, int max_blocks, int num_blocks, int block_size,
                                      const int* kv_len, void* o, float* ws /*B*Hq*num_splits*(D+2)*/, int B,
                                      int S_max, int Hq, int Hk, int D, float scale, int num_splits, hipStream_t st) {
  if (!pa_attn_decode_paged_f8_ok(B, S_max, Hq, Hk, D, num_splits, qstrides, block_size, max_blocks, num_blocks) ||
      table == nullptr || k_scale == nullptr || v_scale == nullptr)
    return (int)hipErrorInvalidValue;
  return decode_launch(q, qstrides, k_codes, v_codes, k_scale, v_scale, table, max_blocks, num_blocks, block_size,
                       kv_len, o, ws, B, S_max, Hq, Hk, D, scale, num_splits, st);
}
