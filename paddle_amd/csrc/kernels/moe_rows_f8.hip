// Weight-only e4m3 ragged grouped expert GEMMs for more rows than moe_decode_f8.hip covers
// (gfx950): the SwiGLU expert MLP of an MoE layer over Fp8ExpertWeights as they are stored,
//
//   a[r, c] = bf16(silu(g) * u),  g = gs[e, c]     * sum_h x[r, h] * gq[e, h, c]
//                                 u = gs[e, I + c] * sum_h x[r, h] * gq[e, h, I + c]
//   y[r, n] = bf16(ds[e, n] * sum_i a[r, i] * dq[e, i, n])
//
// for the rows r in [offs[e], offs[e + 1]) of the expert-sorted x [R, ldx] bf16.  gq [E, H, 2I]
// and dq [E, I, H] are e4m3 codes, gs [E, 2I] and ds [E, H] fp32 power-of-two scales, applied to
// the summed fp32 accumulator (exact).  No dequantised image of a weight is written or read, no
// second layout of the codes is kept, and h = x . gate_up never reaches memory.
//
// Two launches of one kernel template, no workspace: gate|up + SwiGLU (K = H), then down (K = I).
//
// Tiling.  256 threads, four waves.  A workgroup owns kTileM = 32 rows of one expert -- two
// 16-row MFMA tiles that share every converted B fragment; the second costs nothing when the
// tile holds at most 16 rows, the common case of a decode step (2..12 rows per expert) -- and
// kTileN = 128 columns of B, two 16-column strips per wave.  In the down product these are 128
// adjacent columns of H.  In the gate|up product they are 64 gate columns c0.. and the matching
// up columns I + c0..: a wave's first strip is gate, its second the same columns of up, so a
// lane holds g and u of the same output element and SwiGLU happens in registers.
//
// Ragged groups without a host read.  grid.y = min(E, R) + R / 32, an upper bound of
// sum_e ceil(count_e / 32) that needs R and E only.  Every workgroup loads offs (E <= 256: one
// entry per thread, clamped to [0, R] and to ascending order), scans ceil(count / 32) over the
// 256 threads (wave shuffles and four LDS words) and takes the (expert, row tile) whose range
// holds blockIdx.y; past the last tile it exits.  Rows of the tile beyond the expert's last row
// are zeros made in registers and are never stored.  No atomics, flags or spins.
//
// Operand path.  The codes are N-contiguous, the MFMA B operand wants 8 consecutive k per lane.
// A step is kStepK = 128 k: the 128 x 128 code bytes arrive by four global_load_dwordx4 per
// thread (a row of the tile is one 128-byte run, or two of 64 for gate|up) one step ahead of
// their use, are written to LDS as stored, double-buffered (row stride 144 bytes: the 16 rows
// x 16 bytes that half a wave's transposed read touches fall into 64 different banks), and are
// read back with the byte transpose ds_read_b64_tr_b8: in each block of 16 lanes, lane l gives
// the address of the 8 bytes at (row l / 2, columns 8 (l % 2)..+7) of an 8 k x 16 column tile
// and receives column l, k ascending.  Block kb reads rows 8 kb.., so one read is the whole B
// operand (32 k x 16 columns) of one v_mfma_f32_16x16x32_bf16; its two dwords become eight bf16
// by four v_cvt_scalef32_pk_bf16_fp8 at scale 1.0 (exact).  The rows of x / a go through LDS
// once per chunk of kChunkK = 512 k (32 rows x 520 bf16; the 16-byte pad spreads the 16 rows
// of a ds_read_b128 over the banks), shared by the four waves.  One barrier per step, one
// more per chunk.
//
// Arithmetic.  Per output element two fp32 accumulators, the 32-k MFMA steps of even and odd
// index in ascending k, added once at the end, times the scale; SwiGLU as g / (1 + exp(-g)) * u
// in fp32; one rounding per product.  The order is fixed by (K, tile constants) alone and an
// MFMA output element is a function of its A row and its B column only: a row's bits do not
// depend on R, on the counts, on its position in its tile or on the other rows, and two runs
// give the same bits.  Equal bits to moe_decode_f8.hip or to dequant + bf16 are not promised.
//
// Covered: H and I multiples of 16, 1 <= E <= 256, R >= 1 with min(E, R) + R / 32 <= 65535, any
// counts (zero-count experts included), 16-byte aligned operands, ldx a multiple of 8.  All
// offsets are 64-bit.  k from K on and columns from N on are never loaded (zero codes stand in
// for them), rows outside the expert's range are neither loaded nor stored.
//
// None of the tile constants (32 rows, 128 columns, 128-k steps, one step ahead, two
// accumulators, the 64 + 64 split of gate|up) has been timed against an alternative;
// profiles/moe_rows_fp8_bench.md has the measurements against dequant + the bf16 grouped GEMM.
#include "common.h"

using namespace pa;

namespace moe_rows_f8 {

constexpr int kThreads = 256;
constexpr int kWaves = 4;
constexpr int kStrips = 2;      // 16-column strips per wave
constexpr int kRowTiles = 2;    // 16-row MFMA tiles per workgroup
constexpr int kTileM = kRowTiles * 16;
constexpr int kTileN = kWaves * kStrips * 16;  // B columns per workgroup
constexpr int kStepK = 128;     // k per staged tile of codes
constexpr int kChunkK = 512;    // k of the rows staged in LDS at a time
constexpr int kRowPad = 8;      // bf16 elements of padding per LDS row of A
constexpr int kBRow = kTileN + 16;  // LDS row stride of the codes, bytes
constexpr int kMaxExperts = 256;
constexpr int kLoads = kStepK * (kTileN / 16) / kThreads;  // 16-byte loads per thread and step
static_assert(kChunkK % kStepK == 0 && kLoads * kThreads == kStepK * kTileN / 16, "tile constants");
static_assert(kMaxExperts <= kThreads, "one offs entry per thread");

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef int i32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef uint8_t u8;
typedef __attribute__((address_space(3))) i32x2 lds_i32x2;

struct Params {
  const u16* x;        // rows [R, ldx]
  const u8* q;         // codes [E, K, N]
  const float* scale;  // [E, N]
  const int* offs;     // [E + 1]
  u16* out;            // [R, ldo]
  long ldx, ldo;
  int R, K, N, E;
};

#pragma clang fp contract(off)
__device__ __forceinline__ float swiglu_val(float g, float u) {
  return g / (1.f + __expf(-g)) * u;
}

// eight e4m3 codes (k ascending from the low byte of w[0]) -> eight bf16, exact
__device__ __forceinline__ bf16x8 cvt8(i32x2 w) {
  const bf16x2 p0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((uint32_t)w[0], 1.f, false);
  const bf16x2 p1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((uint32_t)w[0], 1.f, true);
  const bf16x2 p2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((uint32_t)w[1], 1.f, false);
  const bf16x2 p3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((uint32_t)w[1], 1.f, true);
  bf16x8 r;
  r[0] = p0[0]; r[1] = p0[1]; r[2] = p1[0]; r[3] = p1[1];
  r[4] = p2[0]; r[5] = p2[1]; r[6] = p3[0]; r[7] = p3[1];
  return r;
}

template <bool SWIGLU>
__global__ __launch_bounds__(kThreads, 2) void rows_kernel(Params p) {
  constexpr int ROW = kChunkK + kRowPad;  // LDS row stride of A, bf16 elements
  __shared__ __attribute__((aligned(16))) u16 sA[kTileM * ROW];
  __shared__ __attribute__((aligned(16))) u8 sB[2][kStepK * kBRow];
  __shared__ int sScan[kWaves];
  __shared__ int sSel[2];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = lane & 15, kb = lane >> 4;  // B: column and k-slot; A: row c of a tile and k-slot

  // ---- which (expert, row tile) is blockIdx.y: a scan of ceil(count / 32) over the experts
  int o0 = 0, tiles = 0;
  if (tid < p.E) {
    int a = p.offs[tid], b = p.offs[tid + 1];
    a = a < 0 ? 0 : (a > p.R ? p.R : a);
    b = b < a ? a : (b > p.R ? p.R : b);
    o0 = a;
    tiles = (b - a + kTileM - 1) / kTileM;
  }
  int inc = tiles;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int v = __shfl_up(inc, d, 64);
    if (lane >= d) inc += v;
  }
  if (lane == 63) sScan[wave] = inc;
  if (tid == 0) sSel[0] = -1;
  __syncthreads();
  for (int w = 0; w < wave; ++w) inc += sScan[w];
  const int slot = blockIdx.y;
  if (slot >= inc - tiles && slot < inc) {  // at most one thread: the ranges are disjoint
    sSel[0] = tid;
    sSel[1] = o0 + (slot - (inc - tiles)) * kTileM;
  }
  __syncthreads();
  const int e = sSel[0];
  if (e < 0) return;  // past the last tile (uniform)
  const int row0 = sSel[1];
  int o1 = p.offs[e + 1];
  o1 = o1 > p.R ? p.R : o1;
  const int rows = o1 - row0 < kTileM ? o1 - row0 : kTileM;  // 1..32 by construction
  const int rt = (rows + 15) >> 4;

  const int K = p.K, N = p.N;
  const int nsteps = (K + kStepK - 1) / kStepK;
  const int c0 = blockIdx.x * (SWIGLU ? kTileN / 2 : kTileN);  // first gate column / first column
  const u8* qe = p.q + (long)e * K * N;
  const u16* arow = p.x + (long)row0 * p.ldx;

  // the thread's 16-byte pieces of a step: row (tid >> 3) + 32 i, piece tid & 7 of the 128 bytes
  const int pc = tid & 7, pr = tid >> 3;
  int gcol;  // global column of the piece
  bool cvalid;
  if (SWIGLU) {
    const int half = N >> 1;
    gcol = c0 + 16 * (pc & 3);
    cvalid = gcol < half;
    if (pc >= 4) gcol += half;
  } else {
    gcol = c0 + 16 * pc;
    cvalid = gcol < N;
  }
  const u32x4 zero4 = {0u, 0u, 0u, 0u};
  const u16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  auto fetch = [&](int t, u32x4 (&w)[kLoads]) {
#pragma unroll
    for (int i = 0; i < kLoads; ++i) {
      const int k = t * kStepK + pr + 32 * i;
      w[i] = (cvalid && k < K) ? *reinterpret_cast<const u32x4*>(qe + (long)k * N + gcol) : zero4;
    }
  };

  // LDS byte column of the wave's strip s, and whether the strip holds columns of B
  int scol[kStrips];
  bool svalid[kStrips];
#pragma unroll
  for (int s = 0; s < kStrips; ++s) {
    scol[s] = SWIGLU ? 64 * s + 16 * wave : 32 * wave + 16 * s;
    svalid[s] = SWIGLU ? (c0 + 16 * wave < (N >> 1)) : (c0 + scol[s] < N);
  }
  // transposed read: lane l of a 16-lane block points at (row l / 2, bytes 8 (l % 2)..) of the block's 8 k
  const int troff = (8 * kb + (c >> 1)) * kBRow + 8 * (c & 1);

  f32x4 acc[kRowTiles][kStrips][2];
#pragma unroll
  for (int r = 0; r < kRowTiles; ++r)
#pragma unroll
    for (int s = 0; s < kStrips; ++s) acc[r][s][0] = acc[r][s][1] = f32x4{0.f, 0.f, 0.f, 0.f};

  u32x4 wq[kLoads];
  fetch(0, wq);
#pragma unroll 1
  for (int t = 0; t < nsteps; ++t) {
    constexpr int kPer = kChunkK / kStepK;
    if (t % kPer == 0) {
      // next chunk of the rows -> LDS (k >= K: zeros; rows past the expert's last are not staged)
      if (t > 0) __syncthreads();  // every wave is done with the previous chunk
      const long a0 = (long)t * kStepK;
      for (int it = tid; it < rows * (kChunkK / 8); it += kThreads) {
        const int m = it / (kChunkK / 8), k8 = it % (kChunkK / 8);
        const long k = a0 + k8 * 8;
        u16x8 v = zero8;
        if (k < K) v = *reinterpret_cast<const u16x8*>(arow + (long)m * p.ldx + k);
        *reinterpret_cast<u16x8*>(sA + m * ROW + k8 * 8) = v;
      }
    }
    // the codes of step t -> the buffer that step t - 2 read (the barrier of step t - 1 is behind)
    u8* sb = sB[t & 1];
#pragma unroll
    for (int i = 0; i < kLoads; ++i) *reinterpret_cast<u32x4*>(sb + (pr + 32 * i) * kBRow + 16 * pc) = wq[i];
    __syncthreads();
    if (t + 1 < nsteps) fetch(t + 1, wq);  // in flight while step t is consumed

    const u16* sa = sA + c * ROW + (t % kPer) * kStepK + kb * 8;
#pragma unroll
    for (int kk = 0; kk < kStepK / 32; ++kk) {
      if (t * kStepK + kk * 32 < K) {  // uniform
        bf16x8 bv[kStrips];
#pragma unroll
        for (int s = 0; s < kStrips; ++s) {
          const u8* ad = sb + kk * 32 * kBRow + troff + scol[s];
          bv[s] = cvt8(__builtin_amdgcn_ds_read_tr8_b64_v2i32((lds_i32x2*)ad));
        }
#pragma unroll
        for (int r = 0; r < kRowTiles; ++r) {
          if (r < rt) {  // uniform: a tile without rows costs nothing
            u16x8 av = zero8;
            if (r * 16 + c < rows) av = *reinterpret_cast<const u16x8*>(sa + r * 16 * ROW + kk * 32);
#pragma unroll
            for (int s = 0; s < kStrips; ++s)
              acc[r][s][kk & 1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, av), bv[s],
                                                                          acc[r][s][kk & 1], 0, 0, 0);
          }
        }
      }
    }
  }

  // lane (c, kb) holds rows 16 r + 4 kb .. + 3 of column c of each of the wave's strips
  const float* sc = p.scale + (long)e * N;
  u16* orow = p.out + (long)row0 * p.ldo;
#pragma unroll
  for (int r = 0; r < kRowTiles; ++r) {
    if (r < rt) {
      if (SWIGLU) {
        if (svalid[0]) {
          const int col = c0 + 16 * wave + c;
          const float gs = sc[col], us = sc[(N >> 1) + col];
          const f32x4 g = (acc[r][0][0] + acc[r][0][1]) * gs, u = (acc[r][1][0] + acc[r][1][1]) * us;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int m = r * 16 + kb * 4 + i;
            if (m < rows) orow[(long)m * p.ldo + col] = f2bf(swiglu_val(g[i], u[i]));
          }
        }
      } else {
#pragma unroll
        for (int s = 0; s < kStrips; ++s) {
          if (svalid[s]) {
            const int col = c0 + scol[s] + c;
            const f32x4 v = (acc[r][s][0] + acc[r][s][1]) * sc[col];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const int m = r * 16 + kb * 4 + i;
              if (m < rows) orow[(long)m * p.ldo + col] = f2bf(v[i]);
            }
          }
        }
      }
    }
  }
}

static int row_tile_bound(int R, int E) { return (E < R ? E : R) + R / kTileM; }

}  // namespace moe_rows_f8

// Tile constants the Python side and the tests size their cases by: 0 rows per workgroup,
// 1 k of the rows staged at a time, 2 B columns per workgroup, 3 k per step.
PA_EXPORT int pa_moe_rows_f8_const(int which) {
  using namespace moe_rows_f8;
  return which == 0 ? kTileM : which == 1 ? kChunkK : which == 2 ? kTileN : which == 3 ? kStepK : -1;
}

// Whether pa_moe_rows_f8 takes this problem.  Sizes, the row stride of x (bf16 elements) and
// addresses only: nothing is dereferenced.
PA_EXPORT int pa_moe_rows_f8_ok(int R, int H, int I, int E, long ldx, const void* x, const void* gate_up_q,
                                const void* gate_up_scale, const void* down_q, const void* down_scale,
                                const void* offs, const void* a, const void* y) {
  if (R < 1 || H < 16 || H % 16 || I < 16 || I % 16 || E < 1 || E > moe_rows_f8::kMaxExperts) return 0;
  if (H > (1 << 24) || I > (1 << 24) || moe_rows_f8::row_tile_bound(R, E) > 65535) return 0;
  if (ldx < H || ldx % 8) return 0;
  const void* ps[] = {x, gate_up_q, gate_up_scale, down_q, down_scale, a, y};
  for (const void* q : ps)
    if (q == nullptr || ((uintptr_t)q & 15)) return 0;
  if (offs == nullptr || ((uintptr_t)offs & 3)) return 0;
  return 1;
}

// y [R, H] bf16 = down(swiglu(gate_up(x))) per expert range of offs [E + 1] (int32, on the
// device); a [R, I] bf16 is the rounded SwiGLU output, written by the first launch and read by
// the second (both contiguous).  A refused problem returns hipErrorInvalidValue and launches
// nothing.  No host synchronisation, no host read of device memory.
PA_EXPORT int pa_moe_rows_f8(const void* x, long ldx, const void* gate_up_q, const void* gate_up_scale,
                             const void* down_q, const void* down_scale, const void* offs, void* a, void* y, int R,
                             int H, int I, int E, hipStream_t st) {
  using namespace moe_rows_f8;
  if (!pa_moe_rows_f8_ok(R, H, I, E, ldx, x, gate_up_q, gate_up_scale, down_q, down_scale, offs, a, y))
    return (int)hipErrorInvalidValue;
  const unsigned gy = (unsigned)row_tile_bound(R, E);
  Params p;
  p.offs = (const int*)offs; p.R = R; p.E = E;
  p.x = (const u16*)x; p.ldx = ldx; p.q = (const u8*)gate_up_q; p.scale = (const float*)gate_up_scale;
  p.out = (u16*)a; p.ldo = I; p.K = H; p.N = 2 * I;
  hipLaunchKernelGGL(rows_kernel<true>, dim3((I + kTileN / 2 - 1) / (kTileN / 2), gy), dim3(kThreads), 0, st, p);
  p.x = (const u16*)a; p.ldx = I; p.q = (const u8*)down_q; p.scale = (const float*)down_scale;
  p.out = (u16*)y; p.ldo = H; p.K = I; p.N = H;
  hipLaunchKernelGGL(rows_kernel<false>, dim3((H + kTileN - 1) / kTileN, gy), dim3(kThreads), 0, st, p);
  PA_LAUNCH_CHECK();
}
