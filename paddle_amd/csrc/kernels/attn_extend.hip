// Multi-token ("extend") attention over the KV cache for gfx950: T >= 1 new query tokens per
// row attend to that row's cached keys plus the chunk itself, causally inside the chunk.
//
//   pa_attn_extend  q [B, T, Hq, D] bf16 against one layer of a cache -- contiguous
//                   [B, S_max, Hk, D] or (table != null) a pool [num_blocks, block_size, Hk, D]
//                   with an int32 block table [Bc, max_blocks]; bf16 elements or
//                   (k_scale != null) e4m3 codes with fp32 scales [.., Hk] addressed like the
//                   codes.  Query t of row b sees the keys n < min(max(base_len[b], 0) + t + 1,
//                   S_max): the chunk's own tokens are already in the cache (pa_kv_append ran
//                   first, the lengths have not advanced).  rows (paged only): q row i reads
//                   cache row rows[i]; base_len is indexed by the q row.  A query without a
//                   visible key gives zeros.  o [B, T, Hq, D] bf16, contiguous.
//
// Tiling.  The G = Hq / Hk query heads of a GQA group and 64 / G consecutive tokens are
// stacked into 64 rows of M; one workgroup of four waves owns (such a query tile, kv head,
// row, split) and every wave 16 of the rows.  Keys are visited in tiles of 64.  A K / V tile
// is loaded from global memory once per workgroup (16-byte loads, 8 bytes of e4m3), held in
// registers under the arithmetic of the tile before it and then written to LDS: K row-major,
// V transposed, both as bf16 -- an e4m3 code becomes cvt(code) * scale, which is exact in
// bf16 by the append's contract, so the arithmetic below does not know the storage type and
// the e4m3 instantiation returns the bits of the bf16 one over the dequantised cache.  Nor
// does it know the layout: the address of a cache row is a compile-time policy, so paged and
// contiguous return the same bits for the same tokens.
//
// Arithmetic (v_mfma_f32_16x16x32_bf16, A[row l&15][k 8(l>>4)+j], B[k 8(l>>4)+j][col l&15],
// C[row 4(l>>4)+reg][col l&15]):
//   S^T = K Q^T    A = K rows from LDS, B = the wave's Q rows (registers, loaded once):
//                  a lane gets its query (l&15) on the lane and 16 keys of the tile in
//                  registers, so the softmax reductions are in-lane plus two shuffles;
//   online softmax fp32, log2 domain, a key masked to -inf when it is at or beyond the
//                  query's own limit, beyond the split, or (paged) has no block;
//   O^T = V^T P^T  B = P rounded to bf16 once, straight from the S^T registers: element j of
//                  lane group h is key 16(2s + (j>>2)) + 4h + (j&3) of k-step s, and the A
//                  operand (two 8-byte reads of a V^T row) follows the same key order.
// A masked key's K and V are never loaded: zeros go to LDS, so a NaN in a slot that no query
// may see cannot reach 0 * v.  Key tiles beyond the query tile's last visible key are not
// visited; a wave skips the tiles beyond its own rows' last key.
//
// Splits: the key range of a query tile is cut into num_splits equal ranges of whole key
// tiles.  num_splits == 1 normalises and writes bf16 directly; otherwise every split stores
// its (m, l, acc[D]) with plain stores and a second kernel merges them.  No atomics, flags or
// spins: two launches on one stream are the only ordering, so the result is bit-identical
// from run to run.  Every cache-row address is computed in 64 bits.
#include <type_traits>

#include "common.h"

using namespace pa;

namespace ext {

constexpr int kThreads = 256;
constexpr int kBM = 64;  // stacked query rows (token x head of the group) per workgroup
constexpr int kBN = 64;  // keys per tile
constexpr int kMaxSplits = 64;

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

struct Params {
  const u16* q;
  long qsb, qst, qsh;  // element strides of q [B, T, Hq, D] over b, t and head
  const void* kc;
  const void* vc;
  const float* ks;  // e4m3 only: one scale per (slot, kv head)
  const float* vs;
  const int* base_len;  // [B]
  const int* rows;      // [B] q row -> cache row, or null: the identity (paged only)
  const int* table;     // [Bc, max_blocks] (paged only)
  float* ws;            // num_splits > 1: [B*T*Hq, ns, 2] (m, l) then [B*T*Hq, ns, D] acc
  u16* o;
  int B, Bc, T, S_max, Hq, Hk, ns, qtiles;
  int max_blocks, num_blocks, bs_shift;
  float scale_log2;  // scale * log2(e)
};

__device__ __forceinline__ f32x4 mfma16(bf16x8 a, bf16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// 8 elements of a cache row as bf16 bits.  e4m3: cvt(code) * scale, exact in bf16.
__device__ __forceinline__ u16x8 row_bf16(const u16x8& r, float) { return r; }
__device__ __forceinline__ u16x8 row_bf16(const u32x2& r, float sc) {
  u16x8 o;
#pragma unroll
  for (int d = 0; d < 2; ++d) {
    const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)r[d], false) * sc;
    const f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)r[d], true) * sc;
    o[4 * d] = f2bf(lo.x);
    o[4 * d + 1] = f2bf(lo.y);
    o[4 * d + 2] = f2bf(hi.x);
    o[4 * d + 3] = f2bf(hi.y);
  }
  return o;
}

template <int D, int G, bool Paged, bool F8>
__global__ __launch_bounds__(kThreads) void attn_extend_kernel(Params p) {
  constexpr int CPR = D / 8;                  // 8-element chunks per cache row
  constexpr int NCH = kBN * CPR / kThreads;   // chunks per thread per key tile
  constexpr int KP = D + 8;                   // pitch of a K row in LDS (elements)
  constexpr int VP = kBN + 4;                 // pitch of a V^T row in LDS (elements; 8-byte rows)
  constexpr int TQ = kBM / G;                 // tokens per query tile
  using Elt = typename std::conditional<F8, uint8_t, u16>::type;
  using Vec = typename std::conditional<F8, u32x2, u16x8>::type;  // 8 elements of a row
  __shared__ __attribute__((aligned(16))) u16 sK[kBN * KP];
  __shared__ __attribute__((aligned(16))) u16 sVt[D * VP];
  __shared__ __attribute__((aligned(16))) uint8_t sOk[kBN];  // paged: whether the key has a block

  const int qt = blockIdx.x % p.qtiles, split = blockIdx.x / p.qtiles;
  const int hk = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lq = lane & 15, lh = lane >> 4;

  int cb = b;  // the cache row
  if constexpr (Paged) {
    if (p.rows != nullptr) cb = p.rows[b];
  }
  const bool row_ok = !Paged || (cb >= 0 && cb < p.Bc);
  if (!row_ok) cb = 0;
  int base = p.base_len[b];
  base = base < 0 ? 0 : base;
  const int t0 = qt * TQ;
  // the limit of query token t: the keys it sees are [0, limit)
  auto limit_of = [&](int t) -> int {
    const long lim = (long)base + t + 1;
    return row_ok ? (int)(lim < (long)p.S_max ? lim : (long)p.S_max) : 0;
  };
  const int t_last = t0 + TQ - 1 < p.T - 1 ? t0 + TQ - 1 : p.T - 1;
  const int len = limit_of(t_last);  // the query tile's last visible key + 1
  // this split's key range: equal chunks of whole key tiles
  int chunk = (len + p.ns - 1) / p.ns;
  chunk = (chunk + kBN - 1) / kBN * kBN;
  const long start = (long)split * chunk;
  const long end = start + chunk < (long)len ? start + chunk : (long)len;

  // this lane's query: stacked row r of the tile -> token t0 + r / G, head hk * G + r % G
  const int r = wave * 16 + lq;
  const int t = t0 + r / G, hq = hk * G + r % G;
  const bool qvalid = t < p.T;
  const int limit_q = qvalid ? limit_of(t) : 0;
  // the last key any row of this wave sees (wave-uniform)
  const int tw_first = t0 + (wave * 16) / G;
  const int tw_last = t0 + (wave * 16 + 15) / G < p.T - 1 ? t0 + (wave * 16 + 15) / G : p.T - 1;
  const int limit_w = tw_first < p.T ? limit_of(tw_last) : 0;

  bf16x8 qf[D / 32];
  {
    const u16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
    const u16* qp = p.q + (long)b * p.qsb + (long)(qvalid ? t : 0) * p.qst + (long)hq * p.qsh + lh * 8;
#pragma unroll
    for (int ks = 0; ks < D / 32; ++ks) {
      const u16x8 v = qvalid ? *reinterpret_cast<const u16x8*>(qp + 32 * ks) : z;
      qf[ks] = __builtin_bit_cast(bf16x8, v);
    }
  }

  float m = -INFINITY, l = 0.f;
  f32x4 acc[D / 16];
#pragma unroll
  for (int db = 0; db < D / 16; ++db) acc[db] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const long rowe = (long)p.Hk * D;  // elements between consecutive slots
  const Elt* kb = reinterpret_cast<const Elt*>(p.kc) + (long)hk * D;
  const Elt* vb = reinterpret_cast<const Elt*>(p.vc) + (long)hk * D;
  const int* trow = Paged ? p.table + (long)cb * p.max_blocks : nullptr;
  const long bmask = Paged ? (1L << p.bs_shift) - 1 : 0;

  Vec kr[NCH], vr[NCH];
  float ksc[NCH], vsc[NCH];
  bool okr[NCH];
  // Paged: the table entries of a tile's keys are fetched one tile ahead of its K / V loads, so
  // the look-up (a dependent load in front of every K / V load) is not on the critical path.
  // key < end <= S_max <= max_blocks << bs_shift keeps the read inside the row.
  int blkn[NCH];
  auto fetch_entries = [&](long k0) {
    if constexpr (Paged) {
#pragma unroll
      for (int i = 0; i < NCH; ++i) {
        const long key = k0 + (i * kThreads + tid) / CPR;
        blkn[i] = key < end ? trow[key >> p.bs_shift] : -1;
      }
    }
  };
  // global -> registers: chunk id = i * kThreads + tid covers (key id / CPR, chunk id % CPR)
  auto load_tile = [&](long k0) {
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int id = i * kThreads + tid;
      const int c = id % CPR;
      const long key = k0 + id / CPR;
      bool ok = key < end;
      long slot;
      if constexpr (Paged) {
        const int blk = blkn[i];  // fetched by the call before this one
        ok = ok && (unsigned)blk < (unsigned)p.num_blocks;  // no block: masked, never dereferenced
        slot = ((long)blk << p.bs_shift) + (key & bmask);
      } else {
        slot = (long)cb * p.S_max + key;
      }
      okr[i] = ok;
      Vec kz, vz;
#pragma unroll
      for (int j = 0; j < (F8 ? 2 : 8); ++j) kz[j] = vz[j] = 0;
      ksc[i] = vsc[i] = 0.f;
      if (ok) {
        kz = *reinterpret_cast<const Vec*>(kb + slot * rowe + c * 8);
        vz = *reinterpret_cast<const Vec*>(vb + slot * rowe + c * 8);
        if constexpr (F8) {
          ksc[i] = p.ks[slot * p.Hk + hk];
          vsc[i] = p.vs[slot * p.Hk + hk];
        }
      }
      kr[i] = kz;
      vr[i] = vz;
    }
    fetch_entries(k0 + kBN);  // of the tile the next call loads
  };
  // registers -> LDS as bf16: K rows, V transposed.  A key without a slot stores zeros.
  auto store_tile = [&]() {
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int id = i * kThreads + tid;
      const int c = id % CPR, kl = id / CPR;
      const u16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
      const u16x8 k8 = okr[i] ? row_bf16(kr[i], ksc[i]) : z;
      const u16x8 v8 = okr[i] ? row_bf16(vr[i], vsc[i]) : z;
      *reinterpret_cast<u16x8*>(&sK[kl * KP + c * 8]) = k8;
#pragma unroll
      for (int j = 0; j < 8; ++j) sVt[(c * 8 + j) * VP + kl] = v8[j];
      if constexpr (Paged) {
        if (c == 0) sOk[kl] = okr[i] ? 1 : 0;
      }
    }
  };

  fetch_entries(start);
  if (start < end) load_tile(start);
  for (long k0 = start; k0 < end; k0 += kBN) {
    __syncthreads();  // the tile before this one has been read
    store_tile();
    __syncthreads();
    if (k0 + kBN < end) load_tile(k0 + kBN);  // in flight under the arithmetic below
    if (k0 >= (long)limit_w) continue;        // none of this wave's rows sees a key of the tile

    // S^T = K Q^T: s[c][reg] is key 16c + 4lh + reg against query lq
    f32x4 s[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      s[c] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < D / 32; ++ks) {
        const u16x8 a = *reinterpret_cast<const u16x8*>(&sK[(16 * c + lq) * KP + 32 * ks + 8 * lh]);
        s[c] = mfma16(__builtin_bit_cast(bf16x8, a), qf[ks], s[c]);
      }
    }
    float mt = -INFINITY;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      uint32_t okw = 0x01010101u;
      if constexpr (Paged) okw = *reinterpret_cast<const uint32_t*>(&sOk[16 * c + 4 * lh]);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const long key = k0 + 16 * c + 4 * lh + e;
        const bool vis = key < (long)limit_q && key < end && ((okw >> (8 * e)) & 1u);
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
    for (int c = 0; c < 4; ++c) {
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
    // P rounded to bf16 once; k-step s2 holds the keys of column blocks 2 s2 and 2 s2 + 1
    bf16x8 pf[2];
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      u16x8 pb;
#pragma unroll
      for (int j = 0; j < 8; ++j) pb[j] = f2bf(s[2 * s2 + (j >> 2)][j & 3]);
      pf[s2] = __builtin_bit_cast(bf16x8, pb);
    }
    // O^T = V^T P^T: acc[db][reg] is element 16 db + 4lh + reg of query lq
#pragma unroll
    for (int db = 0; db < D / 16; ++db) {
      acc[db] *= alpha;
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        const u16* vrow = &sVt[(16 * db + lq) * VP + 32 * s2 + 4 * lh];
        const u16x4 lo = *reinterpret_cast<const u16x4*>(vrow);
        const u16x4 hi = *reinterpret_cast<const u16x4*>(vrow + 16);
        const u16x8 a = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        acc[db] = mfma16(__builtin_bit_cast(bf16x8, a), pf[s2], acc[db]);
      }
    }
  }

  if (!qvalid) return;
  const long row = ((long)b * p.T + t) * p.Hq + hq;
  if (p.ns == 1) {  // one rounding; no visible key: zeros
    u16* op = p.o + row * D + 4 * lh;
#pragma unroll
    for (int db = 0; db < D / 16; ++db) {
      u16x4 w;
#pragma unroll
      for (int e = 0; e < 4; ++e) w[e] = f2bf(l > 0.f ? acc[db][e] / l : 0.f);
      *reinterpret_cast<u16x4*>(op + 16 * db) = w;
    }
    return;
  }
  float* ws_ml = p.ws + (row * p.ns + split) * 2;
  float* ws_acc = p.ws + (long)p.B * p.T * p.Hq * p.ns * 2 + (row * p.ns + split) * D + 4 * lh;
  if (lh == 0) {
    ws_ml[0] = m;
    ws_ml[1] = l;
  }
#pragma unroll
  for (int db = 0; db < D / 16; ++db) *reinterpret_cast<f32x4*>(ws_acc + 16 * db) = acc[db];
}

// one block per (row, token, query head), one thread per output element
template <int D>
__global__ __launch_bounds__(D) void attn_extend_merge_kernel(Params p) {
  const long row = blockIdx.x;
  const int d = threadIdx.x;
  const float* ws_ml = p.ws + row * p.ns * 2;
  const float* ws_acc = p.ws + (long)p.B * p.T * p.Hq * p.ns * 2 + row * p.ns * D;
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
  p.o[row * D + d] = f2bf(ls > 0.f ? as / ls : 0.f);
}

template <int D, bool Paged, bool F8>
static void launch(const Params& p, hipStream_t st) {
  const dim3 grid(p.qtiles * p.ns, p.Hk, p.B);
  switch (p.Hq / p.Hk) {
    case 1: hipLaunchKernelGGL((attn_extend_kernel<D, 1, Paged, F8>), grid, dim3(kThreads), 0, st, p); break;
    case 2: hipLaunchKernelGGL((attn_extend_kernel<D, 2, Paged, F8>), grid, dim3(kThreads), 0, st, p); break;
    case 4: hipLaunchKernelGGL((attn_extend_kernel<D, 4, Paged, F8>), grid, dim3(kThreads), 0, st, p); break;
    default: hipLaunchKernelGGL((attn_extend_kernel<D, 8, Paged, F8>), grid, dim3(kThreads), 0, st, p); break;
  }
  if (p.ns > 1)
    hipLaunchKernelGGL((attn_extend_merge_kernel<D>), dim3((unsigned)((long)p.B * p.T * p.Hq)), dim3(D), 0, st, p);
}

__global__ void i32_add_rows_kernel(int* x, const int* inc, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) x[i] += inc[i];
}

static int block_shift(int block_size) {
  for (int s = 4; s <= 8; ++s)
    if (block_size == (1 << s)) return s;
  return -1;
}

}  // namespace ext

// x[i] += inc[i] over n int32 (the ragged advance of the cache's per-row lengths), on the stream
PA_EXPORT int pa_i32_add_rows(int* x, const int* inc, int n, hipStream_t st) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(ext::i32_add_rows_kernel, dim3((n + 255) / 256), dim3(256), 0, st, x, inc, n);
  PA_LAUNCH_CHECK();
}

// Whether pa_attn_extend takes this problem (else the caller runs its reference path).
// block_size 0: a contiguous cache (max_blocks and num_blocks are ignored).
PA_EXPORT int pa_attn_extend_ok(int B, int T, int S_max, int Hq, int Hk, int D, int num_splits,
                                const long* qstrides /*3: b, t, head*/, int block_size, int max_blocks,
                                int num_blocks) {
  if (B <= 0 || B > 65535 || T <= 0 || S_max <= 0 || Hq <= 0 || Hk <= 0 || Hk > 65535 || Hq % Hk) return 0;
  if (D != 64 && D != 128) return 0;
  const int g = Hq / Hk;
  if (g != 1 && g != 2 && g != 4 && g != 8) return 0;
  if (num_splits < 1 || num_splits > ext::kMaxSplits) return 0;
  if (qstrides[0] % 8 || qstrides[1] % 8 || qstrides[2] % 8) return 0;
  const long qtiles = ((long)T * g + ext::kBM - 1) / ext::kBM;
  if (qtiles * num_splits > 0x7FFFFFFFL || (long)B * T * Hq > 0x7FFFFFFFL) return 0;
  if (block_size != 0) {
    const int shift = ext::block_shift(block_size);
    if (shift < 0 || num_blocks <= 0 || max_blocks <= 0) return 0;
    if (((long)max_blocks << shift) < (long)S_max) return 0;
  }
  return 1;
}

// Split count from the launch shape alone (never from the lengths: no host read): enough
// workgroups for two per compute unit, counting a query tile per 16 tokens, at least 256
// keys per split.  One function for both layouts.  Not tuned by measurement.
PA_EXPORT int pa_attn_extend_splits(int B, int Hk, int T, int S_max) {
  const long wgs = (long)B * Hk * ((T + 15) / 16);
  long want = (512 + wgs - 1) / wgs;
  long cap = S_max / 256;
  if (want > cap) want = cap;
  if (want > ext::kMaxSplits) want = ext::kMaxSplits;
  return want < 1 ? 1 : (int)want;
}

// ws: B * T * Hq * num_splits * (D + 2) floats when num_splits > 1, unused (may be null) otherwise.
// table null: contiguous (rows must be null, Bc is ignored).  k_scale null: a bf16 cache.
PA_EXPORT int pa_attn_extend(const void* q, const long* qstrides /*3: b, t, head*/, const void* k, const void* v,
                             const float* k_scale, const float* v_scale, const int* table, int max_blocks,
                             int num_blocks, int block_size, const int* rows, const int* base_len, void* o,
                             float* ws, int B, int Bc, int T, int S_max, int Hq, int Hk, int D, float scale,
                             int num_splits, hipStream_t st) {
  const bool paged = table != nullptr;
  if (!pa_attn_extend_ok(B, T, S_max, Hq, Hk, D, num_splits, qstrides, paged ? block_size : 0, max_blocks,
                         num_blocks))
    return (int)hipErrorInvalidValue;
  if (paged && block_size == 0) return (int)hipErrorInvalidValue;
  if (!paged && rows != nullptr) return (int)hipErrorInvalidValue;
  if (paged && (Bc <= 0 || (rows == nullptr && B != Bc))) return (int)hipErrorInvalidValue;
  if ((k_scale == nullptr) != (v_scale == nullptr) || base_len == nullptr) return (int)hipErrorInvalidValue;
  if (num_splits > 1 && ws == nullptr) return (int)hipErrorInvalidValue;
  ext::Params p;
  p.q = (const u16*)q; p.qsb = qstrides[0]; p.qst = qstrides[1]; p.qsh = qstrides[2];
  p.kc = k; p.vc = v; p.ks = k_scale; p.vs = v_scale;
  p.base_len = base_len; p.rows = rows; p.table = table;
  p.ws = ws; p.o = (u16*)o;
  p.B = B; p.Bc = paged ? Bc : B; p.T = T; p.S_max = S_max; p.Hq = Hq; p.Hk = Hk; p.ns = num_splits;
  p.qtiles = (int)(((long)T * (Hq / Hk) + ext::kBM - 1) / ext::kBM);
  p.max_blocks = max_blocks; p.num_blocks = num_blocks;
  p.bs_shift = paged ? ext::block_shift(block_size) : 0;
  p.scale_log2 = scale * 1.4426950408889634f;
  const bool f8 = k_scale != nullptr;
  if (paged) {
    if (f8) {
      if (D == 128) ext::launch<128, true, true>(p, st);
      else ext::launch<64, true, true>(p, st);
    } else {
      if (D == 128) ext::launch<128, true, false>(p, st);
      else ext::launch<64, true, false>(p, st);
    }
  } else if (f8) {
    if (D == 128) ext::launch<128, false, true>(p, st);
    else ext::launch<64, false, true>(p, st);
  } else {
    if (D == 128) ext::launch<128, false, false>(p, st);
    else ext::launch<64, false, false>(p, st);
  }
  PA_LAUNCH_CHECK();
}
