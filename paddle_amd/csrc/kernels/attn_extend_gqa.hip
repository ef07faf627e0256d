// Multi-token ("extend") attention over the KV cache for gfx950 at any GQA ratio G = Hq / Hk
// with 1 <= G <= 16: the kernel behind pa_attn_extend for 5, 7 and 9..16 query heads per KV
// head, and behind pa_attn_extend_gqa for every ratio.  The contract is pa_attn_extend's (the
// header of attn_extend.hip): visibility n < min(max(base_len[b], 0) + t + 1, S_max), zeros
// for a query without a visible key, a masked key never loaded, a table entry outside
// [0, num_blocks) never dereferenced, 64-bit cache addresses, plain stores only.
//
// G is a run-time value: one instantiation per (D in {64, 128}, contiguous | paged, bf16 |
// e4m3) and none per ratio.
//
// Query tile.  A workgroup of four waves owns 64 stacked rows of M for one (query tile, kv
// head, row, split).  A tile holds TQ = 64 / G (integer division) consecutive tokens times the
// G heads of the group: row r < TQ * G is token t0 + r / G, head hk * G + r % G, on lane r % 16
// of wave r / 16; r / G and r % G are computed once per lane.  When G does not divide 64 the
// rows r >= TQ * G are dead (4 at G = 5, 1 at 7 and 9, 12 at 13): zeros in Q, no part in the
// wave's skip limit, no store.  r / G of a dead row is TQ, the first token of the *next* tile,
// so liveness is r < TQ * G and never t < T alone.  A token's heads may sit in two waves (G =
// 5: token 3 has heads 0, 1 in wave 0 and 2..4 in wave 1), so the wave's skip limit is that of
// the token of its last live row, not of a token boundary.
//
// Keys are visited in tiles of 64.  A K / V tile is loaded from global memory once per
// workgroup (16-byte loads, 8 bytes of e4m3), held in registers under the arithmetic of the
// tile before it and then written to LDS as bf16, both row-major with 16-byte stores: K with a
// pitch of D + 8 elements, V with D + 16.  Paged: the table entries of a tile are fetched one
// tile ahead of its loads.
//
// Arithmetic (v_mfma_f32_16x16x32_bf16, A[row l&15][k 8(l>>4)+j], B[k 8(l>>4)+j][col l&15],
// C[row 4(l>>4)+reg][col l&15]):
//   S^T = K Q^T    A = K rows from LDS, B = the wave's Q rows (registers, loaded once);
//   online softmax fp32, log2 domain, in-lane plus two shuffles per reduction;
//   O^T = V^T P^T  B = P rounded to bf16 once, straight from the S^T registers: element j of
//                  lane group h is key 16 (2 s + (j >> 2)) + 4 h + (j & 3) of k-step s.  A = V^T
//                  in the same key order, by two ds_read_b64_tr_b16 per 16 elements of d: lane
//                  l of a 16-lane group passes the address of (key row l >> 2, columns
//                  4 (l & 3)..+3) of a 4 x 16 block of V and receives column l, rows ascending.
// The operand contents and their order are those of attn_extend_kernel (which stores V
// transposed with 2-byte LDS stores instead), and so are the tile geometry and the split
// arithmetic: where G divides 64 this kernel returns that kernel's bits.
#include <type_traits>

#include "attn_extend_params.h"

using namespace pa;

namespace ext {
namespace gqa {

typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

template <int D, bool Paged, bool F8>
__global__ __launch_bounds__(kThreads) void attn_extend_gqa_kernel(Params p) {
  constexpr int CPR = D / 8;                 // 8-element chunks per cache row
  constexpr int NCH = kBN * CPR / kThreads;  // chunks per thread per key tile
  constexpr int KP = D + 8;                  // pitch of a K row in LDS (elements)
  constexpr int VP = D + 16;                 // pitch of a V row: a transposing read's 16 rows on all banks
  using Elt = typename std::conditional<F8, uint8_t, u16>::type;
  using Vec = typename std::conditional<F8, u32x2, u16x8>::type;  // 8 elements of a row
  __shared__ __attribute__((aligned(16))) u16 sK[kBN * KP];
  __shared__ __attribute__((aligned(16))) u16 sV[kBN * VP];
  __shared__ __attribute__((aligned(16))) uint8_t sOk[kBN];  // paged: whether the key has a block

  const int qt = blockIdx.x % p.qtiles, split = blockIdx.x / p.qtiles;
  const int hk = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lq = lane & 15, lh = lane >> 4;
  const int G = p.Hq / p.Hk;
  const int TQ = kBM / G;     // tokens per query tile
  const int live = TQ * G;    // live rows of M

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

  // this lane's query: stacked row r of the tile
  const int r = wave * 16 + lq;
  const int rt = r / G;
  const int t = t0 + rt, hq = hk * G + (r - rt * G);
  const bool qvalid = r < live && t < p.T;
  const int limit_q = qvalid ? limit_of(t) : 0;
  // the last key any live row of this wave sees (wave-uniform): from its first and last live rows
  const int rw_last = wave * 16 + 15 < live - 1 ? wave * 16 + 15 : live - 1;
  const int tw_first = t0 + (wave * 16) / G;
  const int tw_last = t0 + rw_last / G < p.T - 1 ? t0 + rw_last / G : p.T - 1;
  const int limit_w = wave * 16 < live && tw_first < p.T ? limit_of(tw_last) : 0;

  bf16x8 qf[D / 32];
  {
    const u16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
    const u16* qp = p.q + (long)b * p.qsb + (long)(qvalid ? t : 0) * p.qst + (long)(qvalid ? hq : 0) * p.qsh + lh * 8;
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

  Vec kr[NCH], vr[NCH];
  float ksc[NCH], vsc[NCH];
  bool okr[NCH];
  // Paged: the table entries of a tile's keys, fetched one tile ahead of its K / V loads.
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
      const int blk = Paged ? blkn[i] : 0;  // fetched by the call before this one
      if constexpr (Paged) ok = ok && (unsigned)blk < (unsigned)p.num_blocks;  // no block: masked, never dereferenced
      const long slot = cache_slot<Paged>(p, cb, blk, key);
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
  // registers -> LDS as bf16, K and V rows alike.  A key without a slot stores zeros.
  auto store_tile = [&]() {
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int id = i * kThreads + tid;
      const int c = id % CPR, kl = id / CPR;
      const u16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
      *reinterpret_cast<u16x8*>(&sK[kl * KP + c * 8]) = okr[i] ? row_bf16(kr[i], ksc[i]) : z;
      *reinterpret_cast<u16x8*>(&sV[kl * VP + c * 8]) = okr[i] ? row_bf16(vr[i], vsc[i]) : z;
      if constexpr (Paged) {
        if (c == 0) sOk[kl] = okr[i] ? 1 : 0;
      }
    }
  };

  // this lane's corner of a transposing read: key row 4 lh + (lq >> 2), columns 4 (lq & 3)..+3
  const u16* vt = sV + (4 * lh + (lq >> 2)) * VP + 4 * (lq & 3);

  fetch_entries(start);
  if (start < end) load_tile(start);
  for (long k0 = start; k0 < end; k0 += kBN) {
    __syncthreads();  // the tile before this one has been read
    store_tile();
    __syncthreads();
    if (k0 + kBN < end) load_tile(k0 + kBN);  // in flight under the arithmetic below
    if (k0 >= (long)limit_w) continue;        // none of this wave's live rows sees a key of the tile

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
        const u16* vp = vt + 32 * s2 * VP + 16 * db;
        const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)vp);
        const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(vp + 16 * VP));
        const s16x8 a = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
        acc[db] = mfma16(__builtin_bit_cast(bf16x8, a), pf[s2], acc[db]);
      }
    }
  }

  if (!qvalid) return;  // a dead row or a token past the chunk stores nothing
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

template <int D>
static void launch(const Params& p, hipStream_t st) {
  const dim3 grid(p.qtiles * p.ns, p.Hk, p.B), block(kThreads);
  const bool f8 = p.ks != nullptr;
  if (p.table != nullptr) {
    if (f8) hipLaunchKernelGGL((attn_extend_gqa_kernel<D, true, true>), grid, block, 0, st, p);
    else hipLaunchKernelGGL((attn_extend_gqa_kernel<D, true, false>), grid, block, 0, st, p);
  } else {
    if (f8) hipLaunchKernelGGL((attn_extend_gqa_kernel<D, false, true>), grid, block, 0, st, p);
    else hipLaunchKernelGGL((attn_extend_gqa_kernel<D, false, false>), grid, block, 0, st, p);
  }
}

}  // namespace gqa

void launch_extend_gqa(const Params& p, int D, hipStream_t st) {
  if (D == 128) gqa::launch<128>(p, st);
  else gqa::launch<64>(p, st);
}

}  // namespace ext
