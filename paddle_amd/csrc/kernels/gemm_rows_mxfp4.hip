// MXFP4 weight GEMM for 1..256 rows on the packed image of gemm_skinny_mxfp4.hip (gfx950):
//
//   C[M, nout] bf16 = epilogue(sum_k A[m, k] * dq[k, n]),   dq[k, n] = e2m1(code[k, n]) * 2^(e8m0[k / 32, n] - 127)
//
// A [M, lda] bf16, 1 <= M <= 256; the weight is the Mxfp4Weight image and its e8m0 scales,
// unchanged (layout: gemm_skinny_mxfp4.hip / ops/skinny_mxfp4.py): no second copy, no repacking.
// The sibling feeds one converted B fragment to one MFMA whatever M is and leaves the matrix
// pipe idle; here the fragment feeds one MFMA per 16-row tile of A, so the load and the
// conversion of a weight dword are paid once per up to 64 rows.
//
// Geometry.  256 threads.  Workgroup (bx, s, by) owns rows 64 by .. 64 by + 63 (four 16-row A
// tiles), the kStrips * 4 = 8 strips of 16 columns from 8 bx on (128 columns) and K slice s (a
// multiple of 128 k).  Wave w owns strips 8 bx + 2 w and + 1.  The weight is read once per
// 64-row tile, from L2 for the tiles after the first.  A lane does the sibling's
// global_load_dwordx4 per strip and 128-k step, kAhead = 4 steps (8 KiB per wave) in flight, and
// one v_cvt_scalef32_pk_bf16_fp4 conversion per dword, strip and step; the converted dword j is
// the B operand of one v_mfma_f32_16x16x32_bf16 per row tile.  The rows of A are staged in LDS
// in chunks of 512 k (64 rows x 520 bf16 = 65 KiB; the row stride is padded by 16 bytes so that
// the 16 rows of a ds_read_b128 fall into different banks), shared by the four waves; an A
// fragment read once from LDS feeds the MFMAs of the wave's two strips.  Row tiles that lie
// wholly at or beyond M issue no LDS reads and no MFMAs (a uniform branch); rows M .. of the
// last partial tile are zeros made in registers and are never staged.  The accumulators of a
// wave are [4 row tiles][2 strips][4 dwords] f32x4 = 128 registers.
//
// Arithmetic: the sibling's, per output element -- four accumulators, one per dword j of a step,
// every step of the slice in ascending k, (acc0 + acc1) + (acc2 + acc3) at the end, slices of
// ceil(KT / splits) tiles, the same fp32 epilogue expressions under fp contract(off).  An MFMA
// output element is a function of its A row and its B column only, so a row's result depends on
// (N, K, num_splits, its x row) only -- not on M, on its position or on the other rows -- and for
// equal num_splits it is the sibling's result bit for bit.
//
// Split-K: raw fp32 partials [splits, M, N] with plain stores, a second kernel adds them in
// slice order, applies the epilogue and rounds once.  No atomics, flags or spins.
//
// Epilogues: 0 none, 1 + bias[N], 2 gelu_tanh(. + bias), 3 SwiGLU over gate|up interleaved in
// 16-column blocks (output [M, N/2]).
//
// All offsets are 64-bit; nothing outside the operands is read or written: rows of A from M on,
// k from K on and columns from N on are never loaded.
//
// Parameters: two strips per wave, four row tiles, the 512-k chunk, four steps in flight and the
// split rule are the starting values; no alternative has been timed against them yet
// (profiles/mxfp4_rows_bench.md has the measurements against dequant + ops.linear, from which
// ops/rows_mxfp4.py takes ROUTED_ROWS = 128).  Resource remarks for gfx950: 213 VGPRs (210 for the
// split-K form), no AGPRs, 66,560 bytes of LDS, no scratch, two waves per SIMD.
#include "common.h"

using namespace pa;

namespace rows_mx4 {

constexpr int kThreads = 256;
constexpr int kWaves = 4;
constexpr int kStrips = 2;     // 16-column strips per wave: an A fragment read from LDS feeds kStrips MFMAs
constexpr int kRowTiles = 4;   // 16-row A tiles per workgroup
constexpr int kTileM = kRowTiles * 16;
constexpr int kTileN = kWaves * kStrips * 16;
constexpr int kMaxRows = 256;
constexpr int kMaxSplits = 1024;
constexpr int kStepK = 128;    // k per weight tile = per wave step
constexpr int kChunkK = 512;   // k of A staged in LDS at a time
constexpr int kRowPad = 8;     // bf16 elements of padding per LDS row of A
constexpr int kAhead = 4;      // weight steps in flight per wave = steps per chunk of A
constexpr int kTileBytes = 1024;
constexpr unsigned long kLimit = 0xFFFFFF00ul;  // bytes per operand, as pa_gemm_skinny_mxfp4_ok
static_assert(kAhead * kStepK == kChunkK, "a chunk of A is refilled once per kAhead steps");

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef uint8_t u8;

struct Params {
  const u16* a;
  const u8* b;      // packed image
  const u8* scale;  // e8m0 [K / 32, N]
  u16* c;
  float* ws;         // [splits, M, N] raw fp32 partials (splits > 1)
  const void* bias;  // [N] or null
  long lda, ldc;
  int M, N, K;
  int KT;           // 128-k tiles over K (the last one may be partial)
  int splits, kts;  // kts: tiles per slice
  int epi, bias_f32;
};

// ------------------------------------------------------------------ epilogues (the sibling's expressions)
#pragma clang fp contract(off)
__device__ __forceinline__ float bias_at(const Params& p, int n) {
  return p.bias_f32 ? ((const float*)p.bias)[n] : bf2f(((const u16*)p.bias)[n]);
}
__device__ __forceinline__ float gelu_tanh(float z) {
  const float u = 0.7978845608028654f * (z + 0.044715f * z * z * z);
  const float t = 1.f - 2.f / (1.f + __expf(2.f * u));
  return 0.5f * z * (1.f + t);
}
__device__ __forceinline__ float epi_col(const Params& p, float v, int n) {
  if (p.epi >= 1) v = v + bias_at(p, n);
  if (p.epi == 2) v = gelu_tanh(v);
  return v;
}
__device__ __forceinline__ float swiglu_val(float g, float u) {
  return g / (1.f + __expf(-g)) * u;
}

__device__ __forceinline__ float e8m0_to_f32(uint32_t e) {
  return __uint_as_float(e << 23);
}

// the eight codes of one dword -> eight bf16 values times the scale (low nibble first)
__device__ __forceinline__ bf16x8 cvt8(uint32_t w, float sc) {
  const bf16x2 p0 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, sc, 0);
  const bf16x2 p1 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, sc, 1);
  const bf16x2 p2 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, sc, 2);
  const bf16x2 p3 = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, sc, 3);
  bf16x8 r;
  r[0] = p0[0]; r[1] = p0[1]; r[2] = p1[0]; r[3] = p1[1];
  r[4] = p2[0]; r[5] = p2[1]; r[6] = p3[0]; r[7] = p3[1];
  return r;
}

// ------------------------------------------------------------------ main kernel
template <bool DIRECT>
__global__ __launch_bounds__(kThreads, 2) void rows_kernel(Params p) {
  constexpr int ROW = kChunkK + kRowPad;  // LDS row stride of A, bf16 elements
  // the A chunk [64][ROW] bf16 during the K loop, the workgroup's [64][128] fp32 sums after it
  __shared__ __attribute__((aligned(16))) u16 sA[kTileM * ROW];
  static_assert(sizeof(u16) * kTileM * ROW >= sizeof(float) * kTileM * kTileN, "sC lives in sA");
  float* sC = reinterpret_cast<float*>(sA);

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = lane & 15, kb = lane >> 4;  // B: column and k-slot; A: row c of a tile and k-slot
  const int split = blockIdx.y;
  const int row0 = blockIdx.z * kTileM;
  const int rows = p.M - row0 < kTileM ? p.M - row0 : kTileM;  // >= 1: the grid has ceil(M / 64) row tiles
  const int rt = (rows + 15) >> 4;                             // 16-row tiles that hold a row
  const int kt0 = split * p.kts;
  int kt1 = kt0 + p.kts;
  if (kt1 > p.KT) kt1 = p.KT;
  const int nsteps = kt1 > kt0 ? kt1 - kt0 : 0;  // the same for the four waves
  const int groups = p.K / 32;

  const u32x4 zero4 = {0u, 0u, 0u, 0u};
  const u16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  const int strip0 = (blockIdx.x * kWaves + wave) * kStrips;
  const u16* arow = p.a + (long)row0 * p.lda;

  // the weight of step t (tile kt0 + t) of the wave's strip s and its scale byte; a step past
  // the slice, a strip past N and a group past K (the last tile may be partial) are not read
  auto fetch = [&](int t, int s, u32x4& w, uint32_t& e) {
    const int strip = strip0 + s;
    const int kt = kt0 + t;
    const int g = kt * 4 + kb;
    const bool v = strip * 16 < p.N && t < nsteps && g < groups;
    w = v ? *reinterpret_cast<const u32x4*>(p.b + (long)strip * p.K * 8 + (long)kt * kTileBytes + lane * 16) : zero4;
    e = v ? (uint32_t)p.scale[(long)g * p.N + strip * 16 + c] : 127u;
  };

  u32x4 wq[kAhead][kStrips];
  uint32_t eq[kAhead][kStrips];
#pragma unroll
  for (int i = 0; i < kAhead; ++i)
#pragma unroll
    for (int s = 0; s < kStrips; ++s) fetch(i, s, wq[i][s], eq[i][s]);

  f32x4 acc[kRowTiles][kStrips][4];
#pragma unroll
  for (int r = 0; r < kRowTiles; ++r)
#pragma unroll
    for (int s = 0; s < kStrips; ++s)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[r][s][j] = f32x4{0.f, 0.f, 0.f, 0.f};

#pragma unroll 1
  for (int t0 = 0; t0 < nsteps; t0 += kAhead) {
    // next chunk of A -> LDS; k >= K are zeros, rows >= M are not staged
    __syncthreads();
    {
      const long a0 = (long)(kt0 + t0) * kStepK;
      for (int it = tid; it < rows * (kChunkK / 8); it += kThreads) {
        const int m = it / (kChunkK / 8), k8 = it % (kChunkK / 8);
        const long k = a0 + k8 * 8;
        u16x8 v = zero8;
        if (k < p.K) v = *reinterpret_cast<const u16x8*>(arow + (long)m * p.lda + k);
        *reinterpret_cast<u16x8*>(sA + m * ROW + k8 * 8) = v;
      }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kAhead; ++i) {
      const int t = t0 + i;  // uniform over the workgroup
      if (t < nsteps) {
        u32x4 w[kStrips];
        float sc[kStrips];
#pragma unroll
        for (int s = 0; s < kStrips; ++s) {
          w[s] = wq[i][s];
          sc[s] = e8m0_to_f32(eq[i][s]);
          fetch(t + kAhead, s, wq[i][s], eq[i][s]);  // in flight while w is consumed
        }
        const u16* sa = sA + c * ROW + i * kStepK + kb * 32;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          bf16x8 bv[kStrips];
#pragma unroll
          for (int s = 0; s < kStrips; ++s) bv[s] = cvt8(w[s][j], sc[s]);
#pragma unroll
          for (int r = 0; r < kRowTiles; ++r) {
            if (r < rt) {  // uniform: a tile wholly beyond M costs nothing
              u16x8 av = zero8;  // rows M .. of the last tile: zeros made here
              if (r * 16 + c < rows) av = *reinterpret_cast<const u16x8*>(sa + r * 16 * ROW + j * 8);
#pragma unroll
              for (int s = 0; s < kStrips; ++s)
                acc[r][s][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, av), bv[s],
                                                                       acc[r][s][j], 0, 0, 0);
            }
          }
        }
      }
    }
  }

  // lane (c, kb) holds rows 16 r + 4 kb .. + 3 of column c of each of the wave's strips
  __syncthreads();  // the last chunk of A has been read by every wave: sC takes its place
#pragma unroll
  for (int r = 0; r < kRowTiles; ++r) {
    if (r < rt) {
#pragma unroll
      for (int s = 0; s < kStrips; ++s) {
        const f32x4 sum = (acc[r][s][0] + acc[r][s][1]) + (acc[r][s][2] + acc[r][s][3]);
#pragma unroll
        for (int i = 0; i < 4; ++i) sC[(r * 16 + kb * 4 + i) * kTileN + (wave * kStrips + s) * 16 + c] = sum[i];
      }
    }
  }
  __syncthreads();

  const int n0 = blockIdx.x * kTileN;
  if (!DIRECT) {
    for (int it = tid; it < rows * (kTileN / 8); it += kThreads) {
      const int m = it / (kTileN / 8), c0 = (it % (kTileN / 8)) * 8;
      const int n = n0 + c0;
      if (n >= p.N) continue;
      float o[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = sC[m * kTileN + c0 + j];
      store8(p.ws + ((long)split * p.M + row0 + m) * p.N + n, o);
    }
  } else if (p.epi == 3) {
    // 8 outputs per item: block b of 32 columns holds gate 0..15 | up 16..31
    for (int it = tid; it < rows * (kTileN / 16); it += kThreads) {
      const int m = it / (kTileN / 16), og = it % (kTileN / 16);
      const int gc = (og >> 1) * 32 + (og & 1) * 8;  // gate columns inside the workgroup's 128
      if (n0 + gc >= p.N) continue;
      float o[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = swiglu_val(sC[m * kTileN + gc + j], sC[m * kTileN + gc + 16 + j]);
      store8(p.c + (long)(row0 + m) * p.ldc + blockIdx.x * (kTileN / 2) + og * 8, o);
    }
  } else {
    for (int it = tid; it < rows * (kTileN / 8); it += kThreads) {
      const int m = it / (kTileN / 8), c0 = (it % (kTileN / 8)) * 8;
      const int n = n0 + c0;
      if (n >= p.N) continue;
      float o[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = epi_col(p, sC[m * kTileN + c0 + j], n + j);
      store8(p.c + (long)(row0 + m) * p.ldc + n, o);
    }
  }
}

// ------------------------------------------------------------------ split-K sum + epilogue
// one thread per output element: partials added in slice order, epilogue in fp32, one rounding
__global__ __launch_bounds__(256) void rows_sum_kernel(Params p) {
  const int nout = p.epi == 3 ? p.N / 2 : p.N;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)p.M * nout) return;
  const int m = (int)(i / nout), o = (int)(i % nout);
  const long slab = (long)p.M * p.N;
  const float* src = p.ws + (long)m * p.N;
  float r;
  if (p.epi == 3) {
    const int gc = (o >> 4) * 32 + (o & 15);
    float g = src[gc], u = src[gc + 16];
    for (int s = 1; s < p.splits; ++s) {
      g = g + src[s * slab + gc];
      u = u + src[s * slab + gc + 16];
    }
    r = swiglu_val(g, u);
  } else {
    float v = src[o];
    for (int s = 1; s < p.splits; ++s) v = v + src[s * slab + o];
    r = epi_col(p, v, o);
  }
  p.c[(long)m * p.ldc + o] = f2bf(r);
}

}  // namespace rows_mx4

// Whether pa_gemm_rows_mxfp4 takes this problem.  Sizes, strides (lda, ldc in bf16 elements) and
// addresses only: nothing is dereferenced.  The sibling's conditions with M up to 256, and a
// partial slab that 32-bit element counts can index.
PA_EXPORT int pa_gemm_rows_mxfp4_ok(int M, int N, int K, long lda, long ldc, int epi, int num_splits, const void* a,
                                    const void* b, const void* c, const void* bias, const void* scale) {
  using rows_mx4::kLimit;
  if (M < 1 || M > rows_mx4::kMaxRows || N < 16 || N % 16 || K < 32 || K % 32) return 0;
  if (epi < 0 || epi > 3 || num_splits < 1 || num_splits > rows_mx4::kMaxSplits) return 0;
  if ((epi == 1 || epi == 2) && bias == nullptr) return 0;
  if (epi == 3 && N % 32) return 0;
  const int nout = epi == 3 ? N / 2 : N;
  if (a == nullptr || b == nullptr || c == nullptr || scale == nullptr) return 0;
  if (((uintptr_t)a & 15) || ((uintptr_t)b & 15) || ((uintptr_t)c & 15)) return 0;
  if (lda < K || lda % 8 || ldc < nout || ldc % 8) return 0;
  if ((unsigned long)M * (unsigned long)lda * 2 >= kLimit || (unsigned long)M * (unsigned long)ldc * 2 >= kLimit ||
      (unsigned long)K * 8ul * (unsigned long)(N / 16) >= kLimit)
    return 0;
  if ((long)num_splits * M * N > 0x7FFFFFFFl) return 0;
  if (bias != nullptr && ((uintptr_t)bias & 3)) return 0;
  return 1;
}

// Split count from N and K alone (never from M: the summation order of an output element must
// not depend on the batch).  The partial slab is splits * M * N * 4 bytes, written and read
// once: at 256 rows every slice costs about as much traffic as 4096 k of the weight, so K is cut
// far less than for the sibling -- the largest power of two that keeps workgroups of the first
// 64-row tile (128 columns each) times splits at or below 512 (two resident workgroups on each
// of 256 compute units), with slices of at least 512 k (one chunk of A), at most 8.
PA_EXPORT int pa_gemm_rows_mxfp4_splits(int N, int K) {
  if (N < 1 || K < 32) return 1;
  const long wgs = ((long)N + rows_mx4::kTileN - 1) / rows_mx4::kTileN;
  long want = 1;
  while (want * 2 * wgs <= 512) want *= 2;
  while (want > 1 && want > K / rows_mx4::kChunkK) want /= 2;
  if (want > 8) want = 8;
  return want < 1 ? 1 : (int)want;
}

// fp32 workspace elements pa_gemm_rows_mxfp4 needs (none for a single slice)
PA_EXPORT int pa_gemm_rows_mxfp4_ws_floats(int M, int N, int splits) {
  return splits > 1 ? splits * M * N : 0;
}

// C [M, ldc] bf16 = epilogue(A [M, lda] . dq [K, N]).  ws: pa_gemm_rows_mxfp4_ws_floats(M, N,
// num_splits) floats.  A refused problem returns hipErrorInvalidValue and launches nothing.  No
// host synchronisation, no host read of device memory: capturable into a HIP graph.
PA_EXPORT int pa_gemm_rows_mxfp4(const void* a, const void* b, const void* scale, void* c, const void* bias,
                                 int bias_f32, float* ws, int M, int N, int K, long lda, long ldc, int epi,
                                 int num_splits, hipStream_t st) {
  if (!pa_gemm_rows_mxfp4_ok(M, N, K, lda, ldc, epi, num_splits, a, b, c, bias, scale))
    return (int)hipErrorInvalidValue;
  if (num_splits > 1 && ws == nullptr) return (int)hipErrorInvalidValue;
  rows_mx4::Params p;
  p.a = (const u16*)a; p.b = (const rows_mx4::u8*)b; p.scale = (const rows_mx4::u8*)scale;
  p.c = (u16*)c; p.ws = num_splits > 1 ? ws : nullptr; p.bias = bias;
  p.lda = lda; p.ldc = ldc;
  p.M = M; p.N = N; p.K = K;
  p.KT = (K + 127) / 128;
  p.splits = num_splits;
  p.kts = (p.KT + num_splits - 1) / num_splits;
  p.epi = epi; p.bias_f32 = bias_f32;
  const dim3 grid((N + rows_mx4::kTileN - 1) / rows_mx4::kTileN, num_splits,
                  (M + rows_mx4::kTileM - 1) / rows_mx4::kTileM);
  if (num_splits == 1) {
    hipLaunchKernelGGL(rows_mx4::rows_kernel<true>, grid, dim3(rows_mx4::kThreads), 0, st, p);
  } else {
    hipLaunchKernelGGL(rows_mx4::rows_kernel<false>, grid, dim3(rows_mx4::kThreads), 0, st, p);
    const long outs = (long)M * (epi == 3 ? N / 2 : N);
    hipLaunchKernelGGL(rows_mx4::rows_sum_kernel, dim3((unsigned)((outs + 255) / 256)), dim3(256), 0, st, p);
  }
  PA_LAUNCH_CHECK();
}
