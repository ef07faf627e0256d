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
#include "common.h"

using namespace pa;

namespace dec {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kUnroll = 4;  // keys per lane group in flight (2 * kUnroll 16-byte loads per lane)
constexpr int kMaxSplits = 64;

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
};

template <bool Paged>
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
      dst = (isk ? p.kc : p.vc) + (slot * p.Hk + hk) * p.D;
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
    if (!rot) {
      *reinterpret_cast<u16x8*>(dst + c * 8) = va;
      *reinterpret_cast<u16x8*>(dst + half + c * 8) = vb;
      continue;
    }
    float cs[8], sn[8], oa[8], ob[8];
    load8(p.cosT + position * half + c * 8, cs);
    load8(p.sinT + position * half + c * 8, sn);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float a = bf2f(va[j]), bb = bf2f(vb[j]);
      oa[j] = a * cs[j] - bb * sn[j];
      ob[j] = bb * cs[j] + a * sn[j];
    }
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
};

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
template <int D, int G, bool Paged>
__global__ __launch_bounds__(kThreads) void attn_decode_kernel(DecodeParams p) {
  constexpr int LG = D / 8;          // lanes per key row
  constexpr int KPW = 64 / LG;       // keys per wave per load
  constexpr int WT = KPW * kUnroll;  // keys per wave per iteration
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
  const u16 *kb, *vb;
  if constexpr (Paged) {  // the pool: rows do not own a slab
    kb = p.kc + (long)hk * D + c * 8;
    vb = p.vc + (long)hk * D + c * 8;
  } else {
    kb = p.kc + (long)b * p.S_max * row + (long)hk * D + c * 8;
    vb = p.vc + (long)b * p.S_max * row + (long)hk * D + c * 8;
  }

  // Paged: the block ids of an iteration's keys are fetched one iteration ahead, so the
  // table look-up (a dependent load in front of each K / V load) is in flight together
  // with the previous iteration's 2 * kUnroll K / V loads and not on the critical path.
  const int* trow = Paged ? p.table + (long)b * p.max_blocks : nullptr;
  const long bmask = Paged ? (1L << p.bs_shift) - 1 : 0;
  int blk[kUnroll];
  if constexpr (Paged) {
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const long key = start + (long)wave * WT + u * KPW + grp;
      blk[u] = table_entry(trow, key, end, p.bs_shift);
    }
  }

  for (long k0 = start + (long)wave * WT; k0 < end; k0 += (long)kWaves * WT) {
    u16x8 kr[kUnroll], vr[kUnroll];
    bool valid[kUnroll];
    int nblk[kUnroll];
    if constexpr (Paged) {
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const long key = k0 + (long)kWaves * WT + u * KPW + grp;
        nblk[u] = table_entry(trow, key, end, p.bs_shift);
      }
    }
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const long key = k0 + u * KPW + grp;
      if constexpr (Paged) {
        // a key whose entry is outside [0, num_blocks) is masked like a key at or beyond
        // end; its lane reads the first slot of the pool, which is always there
        valid[u] = key < end && (unsigned)blk[u] < (unsigned)p.num_blocks;
        const long kk = valid[u] ? ((long)blk[u] << p.bs_shift) + (key & bmask) : 0;
        kr[u] = *reinterpret_cast<const u16x8*>(kb + kk * row);
        vr[u] = *reinterpret_cast<const u16x8*>(vb + kk * row);
      } else {
        valid[u] = key < end;
        // slots at or beyond the range are never read: a lane without a key re-reads key k0
        // (k0 < end here) and its score is masked to -inf below, so its weight is exactly 0
        const long kk = valid[u] ? key : k0;
        kr[u] = *reinterpret_cast<const u16x8*>(kb + kk * row);
        vr[u] = *reinterpret_cast<const u16x8*>(vb + kk * row);
      }
    }
    if constexpr (Paged) {
      // keep all 2 * kUnroll loads ahead of the arithmetic: without this the scheduler sinks
      // the last one below the first score, where its latency is exposed
      __builtin_amdgcn_sched_barrier(0);
      // What the pool's first slot holds (another row's token, inf, NaN) must not reach
      // 0 * v below: clear the v registers of a lane without a key.  A mask, not a branch,
      // and after the last load is issued, so all 2 * kUnroll loads stay in flight.  (Its k
      // needs nothing: the score is replaced by -inf whatever it is.)
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) vr[u] &= (u16x8)(u16)(valid[u] ? 0xFFFF : 0);
    }
    float s[kUnroll][G];
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      float kf[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) kf[j] = bf2f(kr[u][j]);
#pragma unroll
      for (int g = 0; g < G; ++g) {
        float d = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) d = fmaf(qf[g][j], kf[j], d);
#pragma unroll
        for (int x = 1; x < LG; x <<= 1) d += __shfl_xor(d, x, 64);
        s[u][g] = valid[u] ? d : -INFINITY;
      }
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
        for (int u = 0; u < kUnroll; ++u) a = fmaf(pw[u], bf2f(vr[u][j]), a);
        acc[g][j] = a;
      }
      m[g] = mn;
    }
    if constexpr (Paged) {
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) blk[u] = nblk[u];
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

template <int D, bool Paged>
static void launch_decode(const DecodeParams& p, hipStream_t st) {
  const dim3 grid(p.ns, p.Hk, p.B);
  switch (p.Hq / p.Hk) {
    case 1: hipLaunchKernelGGL((attn_decode_kernel<D, 1, Paged>), grid, dim3(kThreads), 0, st, p); break;
    case 2: hipLaunchKernelGGL((attn_decode_kernel<D, 2, Paged>), grid, dim3(kThreads), 0, st, p); break;
    case 4: hipLaunchKernelGGL((attn_decode_kernel<D, 4, Paged>), grid, dim3(kThreads), 0, st, p); break;
    default: hipLaunchKernelGGL((attn_decode_kernel<D, 8, Paged>), grid, dim3(kThreads), 0, st, p); break;
  }
  hipLaunchKernelGGL((attn_decode_merge_kernel<D>), dim3(p.B * p.Hq), dim3(D), 0, st, p);
}

}  // namespace dec

// strides: element strides of the [B, T, Hq+2Hk, D] view of the packed projection over
// (b, t, head); unit stride on D.  cos / sin null: no rotation.
PA_EXPORT int pa_kv_append(const void* qkv, const long* strides /*3*/, const int* pos, const float* cosT,
                           const float* sinT, int max_pos, void* k_cache, void* v_cache, int S_max, void* q_out,
                           int B, int T, int Hq, int Hk, int D, hipStream_t st) {
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
  const long items = (long)B * T * (Hq + 2 * Hk) * (D / 16);
  hipLaunchKernelGGL(dec::kv_append_kernel<false>, dim3(stream_grid(items, 256)), dim3(256), 0, st, p);
  PA_LAUNCH_CHECK();
}

// log2 of a paged cache's block size, or -1 when it is not one of 16, 32, 64, 128, 256
static int paged_block_shift(int block_size) {
  for (int s = 4; s <= 8; ++s)
    if (block_size == (1 << s)) return s;
  return -1;
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
  const long items = (long)B * T * (Hq + 2 * Hk) * (D / 16);
  hipLaunchKernelGGL(dec::kv_append_kernel<true>, dim3(stream_grid(items, 256)), dim3(256), 0, st, p);
  PA_LAUNCH_CHECK();
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

PA_EXPORT int pa_attn_decode(const void* q, const long* qstrides /*2: b, head*/, const void* k_cache,
                             const void* v_cache, const int* kv_len, void* o, float* ws /*B*Hq*num_splits*(D+2)*/, int B, int S_max, int Hq,
                             int Hk, int D, float scale, int num_splits, hipStream_t st) {
  if (!pa_attn_decode_ok(B, S_max, Hq, Hk, D, num_splits, qstrides)) return (int)hipErrorInvalidValue;
  dec::DecodeParams p;
  p.q = (const u16*)q; p.qsb = qstrides[0]; p.qsh = qstrides[1];
  p.kc = (const u16*)k_cache; p.vc = (const u16*)v_cache; p.kv_len = kv_len;
  p.ws = ws; p.o = (u16*)o;
  p.B = B; p.S_max = S_max; p.Hq = Hq; p.Hk = Hk; p.ns = num_splits;
  p.scale_log2 = scale * 1.4426950408889634f;
  p.table = nullptr; p.max_blocks = 0; p.num_blocks = 0; p.bs_shift = 0;
  if (D == 128) dec::launch_decode<128, false>(p, st);
  else dec::launch_decode<64, false>(p, st);
  PA_LAUNCH_CHECK();
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
  dec::DecodeParams p;
  p.q = (const u16*)q; p.qsb = qstrides[0]; p.qsh = qstrides[1];
  p.kc = (const u16*)k_pool; p.vc = (const u16*)v_pool; p.kv_len = kv_len;
  p.ws = ws; p.o = (u16*)o;
  p.B = B; p.S_max = S_max; p.Hq = Hq; p.Hk = Hk; p.ns = num_splits;
  p.scale_log2 = scale * 1.4426950408889634f;
  p.table = table; p.max_blocks = max_blocks; p.num_blocks = num_blocks; p.bs_shift = paged_block_shift(block_size);
  if (D == 128) dec::launch_decode<128, true>(p, st);
  else dec::launch_decode<64, true>(p, st);
  PA_LAUNCH_CHECK();
}
