// MoE FFN for decode steps on gfx950: y[M, H] = sum_j w[t, j] * down[e_tj](swiglu(x_t . gate_up[e_tj])),
// 1 <= M <= 16 rows, E <= 256 experts, top-k <= 16, bf16 operands, fp32 accumulation.
//
// The same bandwidth problem as gemm_skinny.hip with one twist: only the experts the rows
// picked are streamed, each once per product for the whole call, however many rows chose it.
// Four launches on one stream, nothing else orders them (no atomics on global memory, no
// flags, no spins, no compaction pass):
//
//   route    one workgroup per row: fp32 logits x . gate_w [H, E] in a summation order fixed
//            by (H, E), NaN -> -inf, k rounds of arg-max (equal logits: the lower expert
//            wins; an expert is taken once, so the k indices are distinct and in range for
//            any input), weights = softmax over the selected logits (renorm) or the
//            full-softmax probabilities.
//   gate|up  grid (128-column tiles of 2I, K slices, min(E, M k) slots).  Every workgroup
//            derives its expert from idx alone: slot s is the s-th smallest distinct expert
//            id, its rows are the (row, choice) pairs with that id in ascending pair order;
//            workgroups of unused slots exit.  The main loop is gemm_skinny.hip's MN-major
//            one (a lane owns 8 adjacent columns, 16-byte weight loads, the next step's rows
//            in flight, A staged in LDS) on the slot's rows of x, instantiated for 1, 2, 4, 8
//            or 16 accumulator rows and picked per workgroup from the slot's row count, so a
//            call of 16 rows that spreads over 50 experts does the arithmetic of ~2 rows per
//            expert, not of 16.  fp32 partials go to the workspace [slice][pair][2I] with
//            plain stores.  gate_up keeps the model's [gate | up] column layout.
//   down     the same grid over H.  While it stages its A operand it sums the gate|up
//            partials in slice order, applies SwiGLU in fp32 and rounds a to bf16 (the first
//            of the two roundings).  Partials [slice][pair][H].
//   combine  sums the down partials over slices, then over j ascending with the weights, and
//            rounds once (the second rounding).
//
// Determinism and invariance: the K terms of one output element are added per lane in
// ascending K, then the fixed shuffle tree, then waves 0..3, then slices in order -- whatever
// the accumulator-row count, the slot or the other rows of the call.  Row t of an M-row call
// equals the 1-row call on that row bit for bit, in idx, w and y, and two runs give the same
// bits.  Split counts come from (H, I) alone (pa_moe_decode_splits).
//
// All offsets are 64-bit: the stacked gate_up of ernie-moe-21b-a3b is 1.0 GB per layer.
#include "common.h"

using namespace pa;

namespace moedec {

constexpr int kThreads = 256;
constexpr int kWaves = 4;
constexpr int kMaxRows = 16;
constexpr int kMaxExperts = 256;
constexpr int kMaxTopK = 16;
constexpr int kMaxSplits = 64;
constexpr int kTileN = 128;    // columns per workgroup
constexpr int kStepK = 128;    // K rows per workgroup step: 4 waves x 4 lane groups x 8 rows
constexpr int kChunkK = 1024;  // K values of A staged in LDS at a time (8 steps)

typedef float f32x2 __attribute__((ext_vector_type(2)));

// ------------------------------------------------------------------ route
constexpr int kRouteThreads = 1024;
constexpr int kRouteAcc = 8;  // independent accumulators (and loads in flight) per thread

struct RouteParams {
  const u16* x;
  long ldx;
  const float* gw;  // [H, E]
  int* idx;         // [M, k]
  float* w;         // [M, k]
  int M, H, E, k, renorm;
};

// better(a, b): candidate a = (value, expert) beats b; expert < 0 is "no candidate"
__device__ __forceinline__ bool route_better(float av, int ai, float bv, int bi) {
  if (ai < 0) return false;
  if (bi < 0) return true;
  return av > bv || (av == bv && ai < bi);
}

__global__ __launch_bounds__(kRouteThreads) void route_kernel(RouteParams p) {
  __shared__ float s_part[kRouteThreads];
  __shared__ float s_logit[kMaxExperts];
  __shared__ float s_exp[kMaxExperts];
  __shared__ float s_sel_l[kMaxTopK];
  __shared__ int s_sel_i[kMaxTopK];

  const int t = blockIdx.x, tid = threadIdx.x;
  int EP = 1;
  while (EP < p.E) EP <<= 1;
  const int nsl = kRouteThreads / EP;  // H slices; thread = (slice, expert)
  const int e = tid & (EP - 1), sl = tid / EP;
  const int hs = ((p.H + nsl - 1) / nsl + kRouteAcc - 1) / kRouteAcc * kRouteAcc;
  const int h0 = sl * hs;
  const int h1 = h0 + hs < p.H ? h0 + hs : p.H;

  float acc[kRouteAcc];
#pragma unroll
  for (int i = 0; i < kRouteAcc; ++i) acc[i] = 0.f;
  if (e < p.E) {
    const u16* xr = p.x + (long)t * p.ldx;
    const float* g = p.gw + e;
    int h = h0;
#pragma unroll 2
    for (; h + kRouteAcc <= h1; h += kRouteAcc) {
#pragma unroll
      for (int i = 0; i < kRouteAcc; ++i) acc[i] = fmaf(bf2f(xr[h + i]), g[(long)(h + i) * p.E], acc[i]);
    }
#pragma unroll
    for (int i = 0; i < kRouteAcc; ++i)
      if (h + i < h1) acc[i] = fmaf(bf2f(xr[h + i]), g[(long)(h + i) * p.E], acc[i]);
  }
  s_part[tid] = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
  __syncthreads();
  if (tid < kMaxExperts) {
    float v = -INFINITY;
    if (tid < p.E) {
      v = s_part[tid];
      for (int s = 1; s < nsl; ++s) v = v + s_part[s * EP + tid];
      if (v != v) v = -INFINITY;  // NaN counts as -inf
    }
    s_logit[tid] = v;
  }
  __syncthreads();
  // k rounds of arg-max over the experts not taken yet, on wave 0
  const int lane = tid & 63;
  float lv[4];
  bool open[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    lv[c] = s_logit[lane + 64 * c];
    open[c] = lane + 64 * c < p.E;
  }
  for (int j = 0; tid < 64 && j < p.k; ++j) {
    float bv = 0.f;
    int bi = -1;
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (open[c] && route_better(lv[c], lane + 64 * c, bv, bi)) {
        bv = lv[c];
        bi = lane + 64 * c;
      }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, 64);
      const int oi = __shfl_xor(bi, o, 64);
      if (route_better(ov, oi, bv, bi)) {
        bv = ov;
        bi = oi;
      }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (bi == lane + 64 * c) open[c] = false;
    if (lane == 0) {
      s_sel_i[j] = bi;
      s_sel_l[j] = bv;
    }
  }
  __syncthreads();

  const float mx = s_sel_l[0];  // the largest logit of the row
  if (!p.renorm) {
    if (tid < p.E) s_exp[tid] = expf(s_logit[tid] - mx);
    __syncthreads();
  }
  if (tid < p.k) {
    float den = 0.f;
    if (p.renorm) {
      for (int j = 0; j < p.k; ++j) den = den + expf(s_sel_l[j] - mx);
    } else {
      for (int i = 0; i < p.E; ++i) den = den + s_exp[i];
    }
    p.idx[(long)t * p.k + tid] = s_sel_i[tid];
    p.w[(long)t * p.k + tid] = expf(s_sel_l[tid] - mx) / den;
  }
}

// ------------------------------------------------------------------ expert GEMMs
struct Params {
  const u16* x;       // gate|up: activations [M, ldx]
  long ldx;
  const u16* b;       // gate_up [E, H, 2I] or down [E, I, H]
  const int* idx;     // [P] expert of each (row, choice) pair
  const float* wsin;  // down: the gate|up partials [sin][P][2K]
  float* wsout;       // [splits][P][N]
  int P, k, E;
  int N, K;  // per-expert product: B is [K, N]
  int splits, ks;
  int sin;
};

#pragma clang fp contract(off)
__device__ __forceinline__ float swiglu_val(float g, float u) {
  return g / (1.f + __expf(-g)) * u;
}
#pragma clang fp contract(fast)

// Slot -> expert and its pairs, from idx alone.  Returns the slot's pair count (0: unused
// slot); s_rows[0 .. n) are the pair indices in ascending order.  Ids outside [0, E) belong
// to no slot.  A row picks an expert at most once, so a slot has at most M <= 16 pairs.
__device__ __forceinline__ int resolve_slot(const Params& p, int slot, int* s_rows, int& expert) {
  __shared__ unsigned long long s_mask[4];
  __shared__ unsigned long long s_ball[kWaves];
  __shared__ int s_e;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid < 4) s_mask[tid] = 0ull;
  if (tid == 0) s_e = -1;
  __syncthreads();
  const int v = tid < p.P ? p.idx[tid] : -1;
  if ((unsigned)v < (unsigned)p.E) atomicOr(&s_mask[v >> 6], 1ull << (v & 63));  // LDS
  __syncthreads();
  if (tid < p.E) {
    const unsigned long long m = s_mask[tid >> 6];
    int rank = __popcll(m & ((1ull << (tid & 63)) - 1ull));
    for (int i = 0; i < (tid >> 6); ++i) rank += __popcll(s_mask[i]);
    if (((m >> (tid & 63)) & 1ull) && rank == slot) s_e = tid;
  }
  __syncthreads();
  expert = __builtin_amdgcn_readfirstlane(s_e);  // uniform: the weight base stays in scalar registers
  if (expert < 0) return 0;
  const bool match = v == expert;
  const unsigned long long ball = __ballot(match);
  if (lane == 0) s_ball[wave] = ball;
  __syncthreads();
  int pos = __popcll(ball & ((1ull << lane) - 1ull)), n = 0;
  for (int i = 0; i < kWaves; ++i) {
    const int c = __popcll(s_ball[i]);
    if (i < wave) pos += c;
    n += c;
  }
  if (match && pos < kMaxRows) s_rows[pos] = tid;
  __syncthreads();
  return __builtin_amdgcn_readfirstlane(n < kMaxRows ? n : kMaxRows);
}

template <int CW> struct WVec;
template <> struct WVec<8> { typedef u16x8 type; };
template <> struct WVec<4> { typedef u16x4 type; };

// One K slice of one expert's product on the slot's `nr` <= MT rows, over the 16 * CW columns
// from `cbase`: a lane owns CW adjacent columns.  CW = 8 (16-byte loads) covers the 128-column
// tile in one pass; 16 accumulator rows take CW = 4 and two passes over the tile's halves, so
// that accumulators, weights in flight and the prefetch fit the register file without scratch
// (every weight byte is still loaded once).  `reuse_a`: the second pass; where the slice fits
// one chunk of A, the chunk the first pass staged is still in s_a and is not staged again.  The
// K order of an output element is the same for every MT and CW.
template <int MT, int CW, bool DOWN>
__device__ __forceinline__ void tile_body(const Params& p, const u16* __restrict__ bexp, const int* s_rows, int nr,
                                          u16* sA, float* s_red, int cbase, bool reuse_a) {
  typedef typename WVec<CW>::type wvec;
  constexpr int J = CW / 2;       // f32x2 accumulators per row
  constexpr int TW = 16 * CW;     // columns per pass
  constexpr int MH = MT < 8 ? MT : 8;  // accumulator rows per pass over a step
  // sA: A chunk [MT][kChunkK] bf16; s_red: the wave sums [4][MT][TW] fp32

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int cg = lane & 15, kg = lane >> 4;
  const int col = cbase + cg * CW;
  const bool col_ok = col < p.N;
  const int split = blockIdx.y;
  const long kbeg = (long)split * p.ks;
  long kend = kbeg + p.ks;
  if (kend > p.K) kend = p.K;
  const int nsteps = kend > kbeg ? (int)((kend - kbeg + kStepK - 1) / kStepK) : 0;

  f32x2 acc[MT][J];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int j = 0; j < J; ++j) acc[m][j] = f32x2{0.f, 0.f};

  const u16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  wvec zerow;
#pragma unroll
  for (int j = 0; j < CW; ++j) zerow[j] = 0;
  const u16* bcol = bexp + col;
  const long ldb = p.N;
  const int koff = wave * 32 + kg * 8;  // this lane's first K row inside a step

  wvec wc[8];
  {
    const long k0 = kbeg + koff;
    const bool v = col_ok && k0 < kend;
#pragma unroll
    for (int r = 0; r < 8; ++r) wc[r] = v ? *reinterpret_cast<const wvec*>(bcol + (k0 + r) * ldb) : zerow;
  }

#pragma unroll 1
  for (int s = 0; s < nsteps; ++s) {
    if ((s & 7) == 0 && !(reuse_a && nsteps <= 8)) {  // next chunk of A -> LDS; rows >= nr and K values >= kend: zeros
      __syncthreads();
      const long a0 = kbeg + (long)s * kStepK;
      for (int it = tid; it < MT * (kChunkK / 8); it += kThreads) {
        const int m = it / (kChunkK / 8), k8 = it % (kChunkK / 8);
        const long k = a0 + k8 * 8;
        u16x8 v = zero8;
        if (m < nr && k < kend) {
          const long pair = s_rows[m];
          if (!DOWN) {
            v = *reinterpret_cast<const u16x8*>(p.x + (pair / p.k) * p.ldx + k);
          } else {
            // a = bf16(silu(g) * u) from the gate|up partials, summed in slice order
            const long row = 2l * p.K;
            const float* src = p.wsin + pair * row + k;
            float g[8], u[8], o[8];
            load8(src, g);
            load8(src + p.K, u);
            for (int q = 1; q < p.sin; ++q) {
              float tg[8], tu[8];
              load8(src + (long)q * p.P * row, tg);
              load8(src + (long)q * p.P * row + p.K, tu);
#pragma unroll
              for (int j = 0; j < 8; ++j) {
                g[j] = g[j] + tg[j];
                u[j] = u[j] + tu[j];
              }
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = swiglu_val(g[j], u[j]);
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = f2bf(o[j]);
          }
        }
        *reinterpret_cast<u16x8*>(sA + m * kChunkK + k8 * 8) = v;
      }
      __syncthreads();
    }
    // the next step's weight rows are in flight while this step's are consumed
    wvec wn[8];
    {
      const long k0 = kbeg + (long)(s + 1) * kStepK + koff;
      const bool v = col_ok && k0 < kend;
#pragma unroll
      for (int r = 0; r < 8; ++r) wn[r] = v ? *reinterpret_cast<const wvec*>(bcol + (k0 + r) * ldb) : zerow;
    }
    const u16* sa = sA + (s & 7) * kStepK + koff;
#pragma unroll
    for (int mh = 0; mh < MT; mh += MH) {
      u16x8 av[MH];
#pragma unroll
      for (int m = 0; m < MH; ++m) av[m] = *reinterpret_cast<const u16x8*>(sa + (mh + m) * kChunkK);
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        f32x2 wf[J];
#pragma unroll
        for (int j = 0; j < J; ++j) wf[j] = f32x2{bf2f(wc[r][2 * j]), bf2f(wc[r][2 * j + 1])};
#pragma unroll
        for (int m = 0; m < MH; ++m) {
          const float a = bf2f(av[m][r]);
          const f32x2 a2 = {a, a};
#pragma unroll
          for (int j = 0; j < J; ++j) acc[mh + m][j] = __builtin_elementwise_fma(a2, wf[j], acc[mh + m][j]);
        }
      }
    }
#pragma unroll
    for (int r = 0; r < 8; ++r) wc[r] = wn[r];
  }

  // the four lane groups of a wave -> one sum (fixed tree: xor 16, then xor 32)
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int j = 0; j < J; ++j) {
      f32x2 v = acc[m][j];
      v.x += __shfl_xor(v.x, 16, 64);
      v.y += __shfl_xor(v.y, 16, 64);
      v.x += __shfl_xor(v.x, 32, 64);
      v.y += __shfl_xor(v.y, 32, 64);
      acc[m][j] = v;
    }
  __syncthreads();  // every thread is done with the previous pass's sums in s_red
  if (kg == 0) {
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      float* d = s_red + (wave * MT + m) * TW + cg * CW;
#pragma unroll
      for (int j = 0; j < J; j += 2)
        *reinterpret_cast<f32x4*>(d + 2 * j) = f32x4{acc[m][j].x, acc[m][j].y, acc[m][j + 1].x, acc[m][j + 1].y};
    }
  }
  __syncthreads();

  // waves 0..3 in order -> the sums, stored as this slice's partial of the pair's row
  for (int it = tid; it < nr * (TW / 8); it += kThreads) {
    const int m = it / (TW / 8), c0 = (it % (TW / 8)) * 8;
    const int n = cbase + c0;
    if (n >= p.N) continue;
    float o[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float v = s_red[(0 * MT + m) * TW + c0 + j];
#pragma unroll
      for (int w = 1; w < kWaves; ++w) v = v + s_red[(w * MT + m) * TW + c0 + j];
      o[j] = v;
    }
    store8(p.wsout + ((long)split * p.P + s_rows[m]) * p.N + n, o);
  }
}

template <bool DOWN>
__global__ __launch_bounds__(kThreads, 2) void ffn_kernel(Params p) {
  __shared__ __attribute__((aligned(16))) u16 s_a[kMaxRows * kChunkK];  // 32 KiB
  __shared__ __attribute__((aligned(16))) float s_red[kWaves * 1024];   // MT * TW <= 1024: 16 KiB
  __shared__ int s_rows[kMaxRows];
  int expert;
  const int nr = resolve_slot(p, blockIdx.z, s_rows, expert);
  if (nr == 0) return;
  const u16* bexp = p.b + (long)expert * p.K * p.N;
  const int cbase = blockIdx.x * kTileN;
  if (nr <= 1) tile_body<1, 8, DOWN>(p, bexp, s_rows, nr, s_a, s_red, cbase, false);
  else if (nr <= 2) tile_body<2, 8, DOWN>(p, bexp, s_rows, nr, s_a, s_red, cbase, false);
  else if (nr <= 4) tile_body<4, 8, DOWN>(p, bexp, s_rows, nr, s_a, s_red, cbase, false);
  else if (nr <= 8) tile_body<8, 8, DOWN>(p, bexp, s_rows, nr, s_a, s_red, cbase, false);
  else {
#pragma unroll 1
    for (int half = 0; half < 2; ++half) tile_body<16, 4, DOWN>(p, bexp, s_rows, nr, s_a, s_red, cbase + half * 64, half == 1);
  }
}

// ------------------------------------------------------------------ combine
struct CombineParams {
  const float* ws;  // [splits][P][H]
  const float* w;   // [M, k]
  u16* y;
  long ldy;
  int M, k, H, P, splits;
};

#pragma clang fp contract(off)
// 8 outputs per thread: partials in slice order, then j ascending with the weights, one rounding
__global__ __launch_bounds__(256) void combine_kernel(CombineParams p) {
  const int h8 = p.H / 8;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)p.M * h8) return;
  const int t = (int)(i / h8), h0 = (int)(i % h8) * 8;
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
  for (int c = 0; c < p.k; ++c) {
    const long pair = (long)t * p.k + c;
    const float* src = p.ws + pair * p.H + h0;
    float v[8];
    load8(src, v);
    for (int s = 1; s < p.splits; ++s) {
      float tv[8];
      load8(src + (long)s * p.P * p.H, tv);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = v[j] + tv[j];
    }
    const float wc = p.w[pair];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = acc[j] + wc * v[j];
  }
  store8(p.y + (long)t * p.ldy + h0, acc);
}
#pragma clang fp contract(fast)

static int slice_rows(int K, int splits) { return ((K / 8 + splits - 1) / splits) * 8; }

}  // namespace moedec

// Whether the kernels take this problem.  Sizes, element strides and addresses only: nothing
// is dereferenced.  x [M, ldx] bf16, gate_w [H, E] fp32, gate_up [E, H, 2I], down [E, I, H] bf16
// (contiguous).
PA_EXPORT int pa_moe_decode_ok(int M, int H, int I, int E, int k, long ldx, const void* x, const void* gate_w,
                               const void* gate_up, const void* down) {
  using namespace moedec;
  if (M < 1 || M > kMaxRows || H < 8 || H % 8 || I < 8 || I % 8) return 0;
  if (E < 1 || E > kMaxExperts || k < 1 || k > kMaxTopK || k > E) return 0;
  if (H > (1 << 20) || I > (1 << 20) || ldx < H || ldx % 8) return 0;
  if (x == nullptr || ((uintptr_t)x & 15) || gate_w == nullptr || ((uintptr_t)gate_w & 3)) return 0;
  if (gate_up == nullptr || ((uintptr_t)gate_up & 15) || down == nullptr || ((uintptr_t)down & 15)) return 0;
  return 1;
}

// Whether pa_moe_decode_route takes this problem (sizes, strides and addresses only).
PA_EXPORT int pa_moe_decode_route_ok(int M, int H, int E, int k, long ldx, const void* x, const void* gate_w) {
  using namespace moedec;
  if (M < 1 || M > kMaxRows || H < 1 || H > (1 << 20) || E < 1 || E > kMaxExperts || k < 1 || k > kMaxTopK || k > E)
    return 0;
  if (ldx < H || x == nullptr || ((uintptr_t)x & 1) || gate_w == nullptr || ((uintptr_t)gate_w & 3)) return 0;
  return 1;
}

// K slices of the gate|up (which 0: [H, 2I] per expert) and the down (which 1: [I, H]) product:
// a function of H and I alone, never of M, k or the routing.  The smallest power of two that
// gives a single expert's product at least 80 (tile, slice) workgroups -- with the usual
// top-k of 6..8 a one-row call then fills the 256 CUs about twice --, slices of at least 256
// K rows.
PA_EXPORT int pa_moe_decode_splits(int which, int H, int I) {
  if (H < 8 || I < 8) return 1;
  const long N = which ? H : 2l * I, K = which ? I : H;
  const long tiles = (N + moedec::kTileN - 1) / moedec::kTileN;
  long want = 1;
  while (want * tiles < 80 && want * 2 <= K / 256 && want * 2 <= moedec::kMaxSplits) want *= 2;
  return (int)want;
}

// fp32 workspace elements of pa_moe_decode_ffn: both products' partials
PA_EXPORT int pa_moe_decode_ws_floats(int M, int H, int I, int k, int splits_gu, int splits_dn) {
  const long n = (long)M * k * (2l * I * splits_gu + (long)H * splits_dn);
  return n > 0x7FFFFFFFl ? -1 : (int)n;
}

// idx [M, k] int32, w [M, k] fp32 from x [M, ldx] bf16 and gate_w [H, E] fp32.  One launch.
PA_EXPORT int pa_moe_decode_route(const void* x, long ldx, const void* gate_w, void* idx, void* w, int M, int H,
                                  int E, int k, int renorm, hipStream_t st) {
  using namespace moedec;
  if (!pa_moe_decode_route_ok(M, H, E, k, ldx, x, gate_w) || idx == nullptr || w == nullptr ||
      ((uintptr_t)idx & 3) || ((uintptr_t)w & 3))
    return (int)hipErrorInvalidValue;
  RouteParams p;
  p.x = (const u16*)x; p.ldx = ldx; p.gw = (const float*)gate_w; p.idx = (int*)idx; p.w = (float*)w;
  p.M = M; p.H = H; p.E = E; p.k = k; p.renorm = renorm;
  hipLaunchKernelGGL(route_kernel, dim3(M), dim3(kRouteThreads), 0, st, p);
  PA_LAUNCH_CHECK();
}

// y [M, ldy] bf16 from x, the stacked expert weights and the routing (idx, w) of
// pa_moe_decode_route.  ws: pa_moe_decode_ws_floats floats.  Three launches; the grid is a
// function of M, k, E, H, I and the split counts.  A refused problem returns
// hipErrorInvalidValue and launches nothing.  No host synchronisation, no host read of device
// memory: capturable into a HIP graph.
PA_EXPORT int pa_moe_decode_ffn(const void* x, long ldx, const void* gate_up, const void* down, const void* idx,
                                const void* w, float* ws, void* y, long ldy, int M, int H, int I, int E, int k,
                                int splits_gu, int splits_dn, hipStream_t st) {
  using namespace moedec;
  if (!pa_moe_decode_ok(M, H, I, E, k, ldx, x, w, gate_up, down)) return (int)hipErrorInvalidValue;
  if (splits_gu < 1 || splits_gu > kMaxSplits || splits_dn < 1 || splits_dn > kMaxSplits) return (int)hipErrorInvalidValue;
  if (idx == nullptr || ((uintptr_t)idx & 3) || ws == nullptr || ((uintptr_t)ws & 15) || y == nullptr ||
      ((uintptr_t)y & 15) || ldy < H || ldy % 8)
    return (int)hipErrorInvalidValue;
  if (pa_moe_decode_ws_floats(M, H, I, k, splits_gu, splits_dn) < 0) return (int)hipErrorInvalidValue;
  const int P = M * k;
  const int slots = P < E ? P : E;
  float* ws_gu = ws;
  float* ws_dn = ws + (long)splits_gu * P * 2l * I;

  Params g;
  g.x = (const u16*)x; g.ldx = ldx; g.b = (const u16*)gate_up; g.idx = (const int*)idx; g.wsin = nullptr;
  g.wsout = ws_gu; g.P = P; g.k = k; g.E = E; g.N = 2 * I; g.K = H; g.splits = splits_gu;
  g.ks = slice_rows(H, splits_gu); g.sin = 0;
  hipLaunchKernelGGL((ffn_kernel<false>), dim3((g.N + kTileN - 1) / kTileN, splits_gu, slots), dim3(kThreads), 0, st,
                     g);
  Params d = g;
  d.b = (const u16*)down; d.wsin = ws_gu; d.wsout = ws_dn; d.N = H; d.K = I; d.splits = splits_dn;
  d.ks = slice_rows(I, splits_dn); d.sin = splits_gu;
  hipLaunchKernelGGL((ffn_kernel<true>), dim3((d.N + kTileN - 1) / kTileN, splits_dn, slots), dim3(kThreads), 0, st,
                     d);
  CombineParams c;
  c.ws = ws_dn; c.w = (const float*)w; c.y = (u16*)y; c.ldy = ldy; c.M = M; c.k = k; c.H = H; c.P = P;
  c.splits = splits_dn;
  const long items = (long)M * (H / 8);
  hipLaunchKernelGGL(combine_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st, c);
  PA_LAUNCH_CHECK();
}
