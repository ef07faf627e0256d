// MoE FFN for decode steps over FP8 (OCP e4m3) expert weights on gfx950:
//
//   y[M, H] = sum_j w[t, j] * down[e_tj](swiglu(x_t . gate_up[e_tj])),   stacks = codes * scale
//
// 1 <= M <= 16 rows, E <= 256 experts, top-k <= 16, bf16 activations, e4m3 codes [E, K, N] with
// one fp32 scale per (expert, output column) [E, N], fp32 accumulation.  moe_decode.hip's expert
// selection on gemm_skinny_f8.hip's streaming: only the experts the rows picked are read, each
// byte once per product for the whole call, and the bytes are half of the bf16 stacks'.
//
// Three launches after moe_decode.hip's route launch, on one stream, nothing else orders them (no
// atomics on global memory, no flags, no spins, no compaction pass):
//
//   gate|up  grid (column tiles of 2I, K slices, min(E, M k) slots).  A workgroup derives its
//            expert from idx alone (slot s = the s-th smallest distinct expert id, its rows = the
//            (row, choice) pairs with that id in ascending pair order); workgroups of unused
//            slots exit.  Raw fp32 partials of x . codes go to the workspace [slice][pair][2I]
//            with plain stores: the scales stay out of the main loop.
//   down     the same grid over H.  While it stages its A operand it sums the gate|up partials
//            in slice order, multiplies the gate and up sums by gate_up_scale[e, col] and
//            [e, I + col], applies SwiGLU in fp32 and rounds a to bf16 (the first rounding).
//   combine  sums the down partials over slices, multiplies by down_scale[idx[pair], h], then
//            accumulates over j ascending with the weights and rounds once (the second).
//
// Main loop.  A lane's 16-byte load holds 16 adjacent columns of one weight row: 16 columns and
// MT x 16 fp32 accumulators per lane, v_cvt_pk_f32_fp8 (exact) and v_pk_fma_f32 on float2.
// 16 lanes span a tile of 256 columns; the 4 lane groups of a wave times the four waves take
// different K rows, 8 consecutive rows per lane and step: 128 K rows per workgroup step.  One
// geometry: a 128-column tile (8 lanes, 256 K rows per step) was measured against it and lost
// by 5 to 21 % at every row count with the same slices, and is not kept
// (profiles/moe_decode_fp8_bench.md).  Accumulator rows are picked per workgroup from the
// slot's row count: 1, 2, 4, 8 or 16.  The weight rows a lane needs next are in flight while the
// current ones are consumed: 8 rows ahead up to 4 accumulator rows, 4 rows ahead at 8 and 16,
// where the 128 accumulators leave fewer registers.  A 16-row slot does not read the weight
// twice: it narrows the lane's span to 8 columns (8-byte loads of 8 codes) and makes two passes
// over the halves of the tile, with A staged once where the slice fits a chunk.
//
// Registers (two workgroups per compute unit: 256 per lane): 130 / 150 / 174 / 204 / 208 VGPRs
// for the gate|up kernel at 1 / 2 / 4 / 8 / 16 accumulator rows and 116 / 134 / 170 / 213 / 211
// for the down kernel, each instantiation compiled alone; a kernel holds all five and takes their
// maximum (208 and 213).  No scratch.  That rests on one thing outside the main loop: see the
// empty asm after the shuffle tree.
//
// Determinism and invariance: the K terms of an output element are added per lane in ascending
// K, then the fixed shuffle tree (xor CL, .., xor 32), then waves 0..3, then slices in order --
// whatever the accumulator-row count, the column span, the slot or the other rows.  Row t of an
// M-row call equals the 1-row call bit for bit, and two runs give the same bits.  Split counts
// come from (H, I) alone (pa_moe_decode_f8_splits).
//
// Covered: H and I multiples of 16 (every code row 16-byte aligned), contiguous stacks.  All
// offsets are 64-bit; nothing outside the operands is read or written.
//
// pa_fp8w_dequant_experts: out[n, K, N] bf16 = q[sel[n]] * scale[sel[n]] (or every expert in
// order), one launch with the expert on a grid axis, 16-byte loads and stores.
#include "common.h"

using namespace pa;

namespace moedec_f8 {

constexpr int kThreads = 256;
constexpr int kWaves = 4;
constexpr int kMaxRows = 16;
constexpr int kMaxExperts = 256;
constexpr int kMaxTopK = 16;
constexpr int kMaxSplits = 64;
constexpr int kChunkK = 1024;  // K values of A staged in LDS at a time
constexpr int kCL = 16;           // lanes across a column tile
constexpr int kTile = kCL * 16;   // 256 columns
constexpr int kRedFloats = 2048;  // MT * columns per pass <= 2048

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef uint8_t u8;

struct Params {
  const u16* x;        // gate|up: activations [M, ldx]
  long ldx;
  const u8* b;         // codes: gate_up [E, H, 2I] or down [E, I, H]
  const float* scin;   // down: gate_up_scale [E, 2K]
  const int* idx;      // [P] expert of each (row, choice) pair
  const float* wsin;   // down: the gate|up partials [sin][P][2K]
  float* wsout;        // [splits][P][N]
  int P, k, E;
  int N, K;  // per-expert product: B is [K, N]
  int splits, ks;
  int sin;
};

#pragma clang fp contract(off)
// scale, then SwiGLU, on the summed accumulators
__device__ __forceinline__ float swiglu_scaled(float g, float sg, float u, float su) {
  g = g * sg;
  u = u * su;
  return g / (1.f + __expf(-g)) * u;
}
#pragma clang fp contract(fast)

// Slot -> expert and its pairs, from idx alone (moe_decode.hip's rule).  Returns the slot's pair
// count (0: unused slot); s_rows[0 .. n) are the pair indices in ascending order.  Ids outside
// [0, E) belong to no slot.  A row picks an expert at most once: at most M <= 16 pairs.
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
template <> struct WVec<16> { typedef u32x4 type; };
template <> struct WVec<8> { typedef u32x2 type; };
template <int R> struct U16V;
template <> struct U16V<8> { typedef u16x8 type; };
template <> struct U16V<4> { typedef u16x4 type; };

// One K slice of one expert's product on the slot's `nr` <= MT rows, over the CL * CW columns
// from `cbase`: a lane owns CW adjacent columns.  CW = 16 (16-byte loads) covers the tile in one
// pass; 16 accumulator rows take CW = 8 and two passes over the tile's halves, so that
// accumulators, weights in flight and the prefetch fit the register file without scratch (every
// weight byte is still loaded once).  `reuse_a`: the second pass; where the slice fits one
// chunk of A, the chunk the first pass staged is still in sA and is not staged again.  The K
// order of an output element is the same for every MT and CW.
template <int MT, int CW, int CL, bool DOWN>
__device__ __forceinline__ void tile_body(const Params& p, const u8* __restrict__ bexp, const float* scexp,
                                          const int* s_rows, int nr, u16* sA, float* s_red, int cbase, bool reuse_a) {
  typedef typename WVec<CW>::type wvec;
  constexpr int ND = CW / 4;                // dwords per weight load
  constexpr int J = CW / 2;                 // f32x2 accumulators per row
  constexpr int PW = CL * CW;               // columns per pass
  constexpr int KG = 64 / CL;               // lane groups of a wave over K
  constexpr int STEP = kWaves * KG * 8;     // K rows per workgroup step
  constexpr int SPC = kChunkK / STEP;       // steps per chunk of A
  constexpr int RH = MT <= 4 ? 8 : 4;       // weight rows fetched (and consumed) at a time
  constexpr int NH = 8 / RH;                // ticks per step
  constexpr int MH = MT < 8 ? MT : 8;       // accumulator rows per pass over a tick
  typedef typename U16V<RH>::type avec;
  static_assert(MT * PW <= kRedFloats, "s_red");
  // sA: A chunk [MT][kChunkK] bf16; s_red: the tile's sums [MT][PW] fp32

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int cg = lane % CL, kg = lane / CL;
  const int col = cbase + cg * CW;
  const bool col_ok = col < p.N;  // N is a multiple of 16 and col of CW: the whole span is inside
  const int split = blockIdx.y;
  const long kbeg = (long)split * p.ks;
  long kend = kbeg + p.ks;
  if (kend > p.K) kend = p.K;
  const int nsteps = kend > kbeg ? (int)((kend - kbeg + STEP - 1) / STEP) : 0;
  const int nticks = nsteps * NH;

  f32x2 acc[MT][J];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int j = 0; j < J; ++j) acc[m][j] = f32x2{0.f, 0.f};

  const u16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  wvec zerow;
#pragma unroll
  for (int d = 0; d < ND; ++d) zerow[d] = 0u;
  const u8* bcol = bexp + col;
  const long ldb = p.N;
  const int koff = wave * (KG * 8) + kg * 8;  // this lane's first K row inside a step

  // the RH weight rows of tick t (rows at or past kend, and columns past N: zeros, not read; K,
  // the slice length and a lane's row offset are multiples of 8, so the rows of a tick are
  // inside the slice together or not at all)
  auto fetch = [&](int t, wvec (&w)[RH]) {
    const long k0 = kbeg + (long)(t / NH) * STEP + koff + (t % NH) * RH;
    const bool v = col_ok && k0 < kend;
#pragma unroll
    for (int r = 0; r < RH; ++r) w[r] = v ? *reinterpret_cast<const wvec*>(bcol + (k0 + r) * ldb) : zerow;
  };

  wvec wc[RH];
  fetch(0, wc);

#pragma unroll 1
  for (int t = 0; t < nticks; ++t) {
    const int s = t / NH;
    if (t % (SPC * NH) == 0 && !(reuse_a && nsteps <= SPC)) {  // next chunk of A -> LDS; rows >= nr, K >= kend: zeros
      __syncthreads();
      const long a0 = kbeg + (long)s * STEP;
      for (int it = tid; it < MT * (kChunkK / 8); it += kThreads) {
        const int m = it / (kChunkK / 8), k8 = it % (kChunkK / 8);
        const long k = a0 + k8 * 8;
        u16x8 v = zero8;
        if (m < nr && k < kend) {
          const long pair = s_rows[m];
          if (!DOWN) {
            v = *reinterpret_cast<const u16x8*>(p.x + (pair / p.k) * p.ldx + k);
          } else {
            // a = bf16(silu(sg g) * (su u)) from the gate|up partials, summed in slice order
            const long row = 2l * p.K;
            const float* src = p.wsin + pair * row + k;
            float g[8], u[8], sg[8], su[8], o[8];
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
            load8(scexp + k, sg);
            load8(scexp + p.K + k, su);
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = swiglu_scaled(g[j], sg[j], u[j], su[j]);
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = f2bf(o[j]);
          }
        }
        *reinterpret_cast<u16x8*>(sA + m * kChunkK + k8 * 8) = v;
      }
      __syncthreads();
    }
    wvec wn[RH];
    fetch(t + 1, wn);  // in flight while wc is consumed
    const u16* sa = sA + (s % SPC) * STEP + koff + (t % NH) * RH;
#pragma unroll
    for (int mh = 0; mh < MT; mh += MH) {
      avec av[MH];
#pragma unroll
      for (int m = 0; m < MH; ++m) av[m] = *reinterpret_cast<const avec*>(sa + (mh + m) * kChunkK);
#pragma unroll
      for (int r = 0; r < RH; ++r) {
        f32x2 wf[J];
#pragma unroll
        for (int d = 0; d < ND; ++d) {
          wf[2 * d] = __builtin_amdgcn_cvt_pk_f32_fp8(wc[r][d], false);
          wf[2 * d + 1] = __builtin_amdgcn_cvt_pk_f32_fp8(wc[r][d], true);
        }
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
    for (int r = 0; r < RH; ++r) wc[r] = wn[r];
  }

  // the lane groups of a wave -> one sum (fixed tree: xor CL, 2 CL, .., 32).  The empty asm pins
  // each sum here: otherwise the last add of every tree is sunk into the kg == 0 branch below,
  // both of its operands stay live across the barrier, and 128 accumulators become 256 registers.
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int j = 0; j < J; ++j) {
      f32x2 v = acc[m][j];
#pragma unroll
      for (int o = CL; o < 64; o *= 2) {
        v.x += __shfl_xor(v.x, o, 64);
        v.y += __shfl_xor(v.y, o, 64);
      }
      asm volatile("" : "+v"(v));
      acc[m][j] = v;
    }
  // waves 0..3 in order -> the tile's sums, accumulated in place: ((w0 + w1) + w2) + w3
  __syncthreads();  // every thread is done with the previous pass's sums in s_red
#pragma unroll 1
  for (int w = 0; w < kWaves; ++w) {
    if (wave == w && kg == 0) {
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        float* d = s_red + m * PW + cg * CW;
#pragma unroll
        for (int j = 0; j < J; j += 2) {
          f32x4 v = f32x4{acc[m][j].x, acc[m][j].y, acc[m][j + 1].x, acc[m][j + 1].y};
          if (w > 0) v = *reinterpret_cast<const f32x4*>(d + 2 * j) + v;
          *reinterpret_cast<f32x4*>(d + 2 * j) = v;
        }
      }
    }
    __syncthreads();
  }

  // stored as this slice's partial of the pair's row
  for (int it = tid; it < nr * (PW / 8); it += kThreads) {
    const int m = it / (PW / 8), c0 = (it % (PW / 8)) * 8;
    const int n = cbase + c0;
    if (n >= p.N) continue;
    float o[8];
    load8(s_red + m * PW + c0, o);
    store8(p.wsout + ((long)split * p.P + s_rows[m]) * p.N + n, o);
  }
}

template <bool DOWN>
__global__ __launch_bounds__(kThreads, 2) void ffn_kernel(Params p) {
  __shared__ __attribute__((aligned(16))) u16 s_a[kMaxRows * kChunkK];  // 32 KiB
  __shared__ __attribute__((aligned(16))) float s_red[kRedFloats];      // 8 KiB
  __shared__ int s_rows[kMaxRows];
  int expert;
  const int nr = resolve_slot(p, blockIdx.z, s_rows, expert);
  if (nr == 0) return;
  const u8* bexp = p.b + (long)expert * p.K * p.N;
  const float* scexp = DOWN ? p.scin + (long)expert * 2l * p.K : nullptr;
  constexpr int CL = kCL;
  const int cbase = blockIdx.x * kTile;
  if (nr <= 1) tile_body<1, 16, CL, DOWN>(p, bexp, scexp, s_rows, nr, s_a, s_red, cbase, false);
  else if (nr <= 2) tile_body<2, 16, CL, DOWN>(p, bexp, scexp, s_rows, nr, s_a, s_red, cbase, false);
  else if (nr <= 4) tile_body<4, 16, CL, DOWN>(p, bexp, scexp, s_rows, nr, s_a, s_red, cbase, false);
  else if (nr <= 8) tile_body<8, 16, CL, DOWN>(p, bexp, scexp, s_rows, nr, s_a, s_red, cbase, false);
  else {
#pragma unroll 1
    for (int half = 0; half < 2; ++half)
      tile_body<16, 8, CL, DOWN>(p, bexp, scexp, s_rows, nr, s_a, s_red, cbase + half * (CL * 8), half == 1);
  }
}

// ------------------------------------------------------------------ combine
struct CombineParams {
  const float* ws;     // [splits][P][H]
  const float* w;      // [M, k]
  const float* scale;  // down_scale [E, H]
  const int* idx;      // [P]
  u16* y;
  long ldy;
  int M, k, H, P, E, splits;
};

#pragma clang fp contract(off)
// 8 outputs per thread: partials in slice order, the scale, then j ascending with the weights,
// one rounding
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
    const int e = p.idx[pair];
    if ((unsigned)e >= (unsigned)p.E) continue;  // no slot computed it, and there is no scale to read
    const float* src = p.ws + pair * p.H + h0;
    float v[8], sc[8];
    load8(src, v);
    for (int s = 1; s < p.splits; ++s) {
      float tv[8];
      load8(src + (long)s * p.P * p.H, tv);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = v[j] + tv[j];
    }
    load8(p.scale + (long)e * p.H + h0, sc);
    const float wc = p.w[pair];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = acc[j] + wc * (v[j] * sc[j]);
  }
  store8(p.y + (long)t * p.ldy + h0, acc);
}
#pragma clang fp contract(fast)

static int slice_rows(int K, int splits) { return ((K / 8 + splits - 1) / splits) * 8; }

// ------------------------------------------------------------------ stack dequantiser
// one item = 16 adjacent columns of one row of one expert: a 16-byte load, two 16-byte stores
__global__ __launch_bounds__(256) void dequant_experts_kernel(const u8* q, const float* scale, const long* sel,
                                                              u16* out, long E, long K, long N) {
  const long e = sel ? sel[blockIdx.y] : (long)blockIdx.y;
  if (e < 0 || e >= E) return;  // an index outside the stack reads nothing
  q += e * K * N;
  scale += e * N;
  out += (long)blockIdx.y * K * N;
  const long per_row = N / 16, items = K * per_row;
  for (long it = (long)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += (long)gridDim.x * blockDim.x) {
    const long k = it / per_row, n = (it % per_row) * 16;
    const u32x4 w = *reinterpret_cast<const u32x4*>(q + k * N + n);
    float lo8[8], hi8[8], s0[8], s1[8];
    load8(scale + n, s0);
    load8(scale + n + 8, s1);
#pragma unroll
    for (int d = 0; d < 2; ++d) {
      const f32x2 a = __builtin_amdgcn_cvt_pk_f32_fp8(w[d], false), b = __builtin_amdgcn_cvt_pk_f32_fp8(w[d], true);
      const f32x2 c = __builtin_amdgcn_cvt_pk_f32_fp8(w[2 + d], false), f = __builtin_amdgcn_cvt_pk_f32_fp8(w[2 + d], true);
      lo8[4 * d] = a.x; lo8[4 * d + 1] = a.y; lo8[4 * d + 2] = b.x; lo8[4 * d + 3] = b.y;
      hi8[4 * d] = c.x; hi8[4 * d + 1] = c.y; hi8[4 * d + 2] = f.x; hi8[4 * d + 3] = f.y;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      lo8[j] = lo8[j] * s0[j];
      hi8[j] = hi8[j] * s1[j];
    }
    store8(out + k * N + n, lo8);
    store8(out + k * N + n + 8, hi8);
  }
}

}  // namespace moedec_f8

// Whether the kernels take this problem.  Sizes, element strides and addresses only: nothing
// is dereferenced.  x [M, ldx] bf16, gate_w [H, E] fp32, codes gate_up [E, H, 2I] / down
// [E, I, H] e4m3 and scales [E, 2I] / [E, H] fp32 (all contiguous).
PA_EXPORT int pa_moe_decode_f8_ok(int M, int H, int I, int E, int k, long ldx, const void* x, const void* gate_w,
                                  const void* gate_up_q, const void* gate_up_scale, const void* down_q,
                                  const void* down_scale) {
  using namespace moedec_f8;
  if (M < 1 || M > kMaxRows || H < 16 || H % 16 || I < 16 || I % 16) return 0;
  if (E < 1 || E > kMaxExperts || k < 1 || k > kMaxTopK || k > E) return 0;
  if (H > (1 << 20) || I > (1 << 20) || ldx < H || ldx % 8) return 0;
  if (x == nullptr || ((uintptr_t)x & 15) || gate_w == nullptr || ((uintptr_t)gate_w & 3)) return 0;
  if (gate_up_q == nullptr || ((uintptr_t)gate_up_q & 15) || down_q == nullptr || ((uintptr_t)down_q & 15)) return 0;
  if (gate_up_scale == nullptr || ((uintptr_t)gate_up_scale & 15) || down_scale == nullptr ||
      ((uintptr_t)down_scale & 15))
    return 0;
  return 1;
}

// K slices of the gate|up (which 0: [H, 2I] per expert) and the down (which 1: [I, H]) product:
// a function of H and I alone, never of M, k or the routing.  The smallest power of two that
// gives a single expert's product at least 40 (tile, slice) workgroups, with slices of at least
// 512 K rows.  Half the bf16 kernel's 80 workgroups and twice its 256 rows: a 256-column tile of
// codes holds the bytes of its 128-column tile, and every slice pays the slot resolution, the
// staging of A and a round trip of fp32 partials.  Measured at one shape only, H 2560, I 1536,
// where it gives (4, 2): as fast as (4, 4) at one row and 2 to 8 % faster from two rows on;
// (2, 2) is 6 % slower at one row, (1, 1) 36 % (profiles/moe_decode_fp8_bench.md).
PA_EXPORT int pa_moe_decode_f8_splits(int which, int H, int I) {
  constexpr long kMinSlice = 512;
  if (H < 16 || I < 16) return 1;
  const long N = which ? H : 2l * I, K = which ? I : H;
  const long tiles = (N + moedec_f8::kTile - 1) / moedec_f8::kTile;
  long want = 1;
  while (want * tiles < 40 && want * 2 <= K / kMinSlice && want * 2 <= moedec_f8::kMaxSplits) want *= 2;
  return (int)want;
}

// fp32 workspace elements of pa_moe_decode_ffn_f8: both products' partials
PA_EXPORT int pa_moe_decode_f8_ws_floats(int M, int H, int I, int k, int splits_gu, int splits_dn) {
  const long n = (long)M * k * (2l * I * splits_gu + (long)H * splits_dn);
  return n > 0x7FFFFFFFl ? -1 : (int)n;
}

// y [M, ldy] bf16 from x, the e4m3 expert stacks with their scales and the routing (idx, w) of
// pa_moe_decode_route.  ws: pa_moe_decode_f8_ws_floats floats.  Three launches; the grid is a
// function of M, k, E, H, I and the split counts.  A refused problem returns
// hipErrorInvalidValue and launches nothing.  No host synchronisation, no host read of device
// memory: capturable into a HIP graph.
PA_EXPORT int pa_moe_decode_ffn_f8(const void* x, long ldx, const void* gate_up_q, const void* gate_up_scale,
                                   const void* down_q, const void* down_scale, const void* idx, const void* w,
                                   float* ws, void* y, long ldy, int M, int H, int I, int E, int k, int splits_gu,
                                   int splits_dn, hipStream_t st) {
  using namespace moedec_f8;
  if (!pa_moe_decode_f8_ok(M, H, I, E, k, ldx, x, w, gate_up_q, gate_up_scale, down_q, down_scale))
    return (int)hipErrorInvalidValue;
  if (splits_gu < 1 || splits_gu > kMaxSplits || splits_dn < 1 || splits_dn > kMaxSplits) return (int)hipErrorInvalidValue;
  if (idx == nullptr || ((uintptr_t)idx & 3) || ws == nullptr || ((uintptr_t)ws & 15) || y == nullptr ||
      ((uintptr_t)y & 15) || ldy < H || ldy % 8)
    return (int)hipErrorInvalidValue;
  if (pa_moe_decode_f8_ws_floats(M, H, I, k, splits_gu, splits_dn) < 0) return (int)hipErrorInvalidValue;
  const int P = M * k;
  const int slots = P < E ? P : E;
  float* ws_gu = ws;
  float* ws_dn = ws + (long)splits_gu * P * 2l * I;

  Params g;
  g.x = (const u16*)x; g.ldx = ldx; g.b = (const u8*)gate_up_q; g.scin = nullptr; g.idx = (const int*)idx;
  g.wsin = nullptr; g.wsout = ws_gu; g.P = P; g.k = k; g.E = E; g.N = 2 * I; g.K = H; g.splits = splits_gu;
  g.ks = slice_rows(H, splits_gu); g.sin = 0;
  Params d = g;
  d.b = (const u8*)down_q; d.scin = (const float*)gate_up_scale; d.wsin = ws_gu; d.wsout = ws_dn; d.N = H; d.K = I;
  d.splits = splits_dn; d.ks = slice_rows(I, splits_dn); d.sin = splits_gu;
  hipLaunchKernelGGL(ffn_kernel<false>, dim3((g.N + kTile - 1) / kTile, g.splits, slots), dim3(kThreads), 0, st, g);
  hipLaunchKernelGGL(ffn_kernel<true>, dim3((d.N + kTile - 1) / kTile, d.splits, slots), dim3(kThreads), 0, st, d);
  CombineParams c;
  c.ws = ws_dn; c.w = (const float*)w; c.scale = (const float*)down_scale; c.idx = (const int*)idx; c.y = (u16*)y;
  c.ldy = ldy; c.M = M; c.k = k; c.H = H; c.P = P; c.E = E; c.splits = splits_dn;
  const long items = (long)M * (H / 8);
  hipLaunchKernelGGL(combine_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st, c);
  PA_LAUNCH_CHECK();
}

// out [n, K, N] bf16 = q [E, K, N] e4m3 * scale [E, N], for the n experts sel[0 .. n) (int64
// on the device; null: n = E, every expert in order).  N % 16 == 0, contiguous, 16-byte aligned.
PA_EXPORT int pa_fp8w_dequant_experts(const void* q, const void* scale, const void* sel, void* out, long n, long E,
                                      long K, long N, hipStream_t st) {
  if (n < 1 || n > 65535 || E < 1 || K < 1 || N < 16 || N % 16 || q == nullptr || scale == nullptr || out == nullptr ||
      ((uintptr_t)q & 15) || ((uintptr_t)out & 15) || ((uintptr_t)scale & 15) || ((uintptr_t)sel & 7) ||
      (sel == nullptr && n != E))
    return (int)hipErrorInvalidValue;
  const long items = K * (N / 16);
  long gx = (items + 255) / 256;
  if (gx > 1024) gx = 1024;
  hipLaunchKernelGGL(moedec_f8::dequant_experts_kernel, dim3((unsigned)gx, (unsigned)n), dim3(256), 0, st,
                     (const moedec_f8::u8*)q, (const float*)scale, (const long*)sel, (u16*)out, E, K, N);
  PA_LAUNCH_CHECK();
}
