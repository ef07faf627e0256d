// Weight-only e4m3 GEMM for 1..256 rows on an Fp8Weight as it is stored (gfx950):
//
//   C[M, nout] bf16 = epilogue(scale[n] * sum_k A[m, k] * e4m3(q[k, n]))
//
// A [M, lda] bf16, 1 <= M <= 256; q [K, ldq] e4m3 codes, N-contiguous, and scale [N] fp32 are the
// Fp8Weight's buffers, unchanged: no repacked second image of the codes is kept and no
// dequantised image is written.  gemm_skinny_f8.hip stops at 16 rows (fp32 FMAs, the matrix
// pipe idle); beyond it a product used to write a bf16 image of the whole weight and read it
// back.  Here a weight byte is read once per up to 64 rows and feeds the MFMAs directly.
//
// Geometry.  256 threads, four waves.  Workgroup (bx, by, s) owns rows 64 by .. 64 by + 63 (four
// 16-row A tiles), columns 128 bx .. + 127 (two 16-column strips per wave: wave w owns columns
// 32 w .. 32 w + 31 of the tile) and K slice s, a multiple of 128 k.  One converted B fragment
// feeds up to four v_mfma_f32_16x16x32_bf16, one per row tile; row tiles that lie wholly at or
// beyond M issue no LDS reads and no MFMAs (a uniform branch), and rows M .. of the last partial
// tile are zeros made in registers and are never staged.  The weight is read once per 64-row
// tile, from L2 for the tiles after the first.
//
// B operand path (that of moe_rows_f8.hip).  The codes are N-contiguous, the MFMA B operand wants
// 8 consecutive k per lane.  A step is kStepK = 128 k: the 128 x 128 code bytes arrive by four
// global_load_dwordx4 per thread (a row of the tile is one 128-byte run) one step ahead of their
// use, are written to LDS as stored, double-buffered (row stride 144 bytes: the 16 rows x 16
// bytes that half a wave's transposed read touches fall into 64 different banks), and are read
// back with the byte transpose ds_read_b64_tr_b8: in each block of 16 lanes, lane l gives the
// address of the 8 bytes at (row l / 2, columns 8 (l % 2)..+7) of an 8 k x 16 column tile and
// receives column l, k ascending.  Block kb reads rows 8 kb.., so one read is the whole B operand
// (32 k x 16 columns) of one MFMA; its two dwords become eight bf16 by four
// v_cvt_scalef32_pk_bf16_fp8 at scale 1.0 (exact: e4m3 has 3 mantissa bits, bf16 has 7).
//
// A operand path.  The rows of A go through LDS in chunks of kChunkK = 256 k (64 rows x 264
// bf16 = 33 KiB; the 16-byte pad spreads the 16 rows of a ds_read_b128 over the banks), shared by
// the four waves; an A fragment read once feeds the MFMAs of the wave's two strips.  With the two
// code buffers that is 70,656 bytes of LDS: two workgroups per compute unit.  One barrier per
// step, one more per chunk.
//
// Arithmetic.  Per output element two fp32 accumulators, the 32-k MFMA steps of even and odd
// index of each 128-k step in ascending k, added once at the end of the slice; slices of
// ceil(KT / splits) 128-k steps; the partial sums of the slices added in slice order; then
// * scale[n] (exact for the quantiser's power-of-two scales), the fp32 epilogue under fp
// contract(off), one rounding to bf16.  An MFMA output element is a function of its A row and its
// B column only, so a row's result depends on (N, K, num_splits, its x row) only -- not on M, on
// its position or on the other rows -- and two runs give the same bits.  The bits of
// gemm_skinny_f8.hip (fp32 FMAs) or of dequant + the bf16 GEMM are not promised.
//
// Split-K: raw fp32 partials [splits, M, N] with plain stores, a second kernel adds them in slice
// order, applies scale and epilogue and rounds once.  No atomics, flags or spins.
//
// Epilogues: 0 none, 1 + bias[N], 2 gelu_tanh(. + bias), 3 SwiGLU over gate|up interleaved in
// 16-column blocks (output [M, N/2]).
//
// Covered: 1 <= M <= 256, K a positive multiple of 16, N a multiple of 16 (32 with SwiGLU),
// 16-byte aligned operands, lda / ldc multiples of 8, ldq a multiple of 16.  All offsets are
// 64-bit; nothing outside the operands is read or written: rows of A from M on, k from K on and
// columns from N on are never loaded (zero codes stand in for them).
//
// Parameters: 64 rows x 128 columns, 128-k steps one step ahead, the 256-k chunk of A (staged
// synchronously), two accumulators and the split rule are the starting values; none has been
// timed against an alternative (profiles/fp8_rows_bench.md has the measurements against
// dequant + ops.linear, from which ops/rows_fp8.py takes ROUTED_ROWS = 128).  Resource remarks for
// gfx950: 113 VGPRs (112 for the split-K form), no AGPRs, 70,656 bytes of LDS, no scratch, two
// waves per SIMD.
#include "common.h"

using namespace pa;

namespace rows_f8 {

constexpr int kThreads = 256;
constexpr int kWaves = 4;
constexpr int kStrips = 2;     // 16-column strips per wave: an A fragment read from LDS feeds kStrips MFMAs
constexpr int kRowTiles = 4;   // 16-row A tiles per workgroup
constexpr int kTileM = kRowTiles * 16;
constexpr int kTileN = kWaves * kStrips * 16;
constexpr int kMaxRows = 256;
constexpr int kMaxSplits = 1024;
constexpr int kStepK = 128;    // k per staged tile of codes
constexpr int kChunkK = 256;   // k of A staged in LDS at a time
constexpr int kMinSliceK = 512;  // the split rule cuts K into slices of at least this many k
constexpr int kRowPad = 8;     // bf16 elements of padding per LDS row of A
constexpr int kBRow = kTileN + 16;  // LDS row stride of the codes, bytes
constexpr int kLoads = kStepK * (kTileN / 16) / kThreads;  // 16-byte loads per thread and step
constexpr unsigned long kLimit = 0xFFFFFF00ul;  // bytes per operand, as pa_gemm_skinny_f8_ok
static_assert(kChunkK % kStepK == 0 && kLoads * kThreads == kStepK * kTileN / 16, "tile constants");

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef int i32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef uint8_t u8;
typedef __attribute__((address_space(3))) i32x2 lds_i32x2;

struct Params {
  const u16* a;
  const u8* q;         // codes [K, ldq]
  const float* scale;  // [N]
  u16* c;
  float* ws;         // [splits, M, N] raw fp32 partials (splits > 1)
  const void* bias;  // [N] or null
  long lda, ldq, ldc;
  int M, N, K;
  int KT;           // 128-k steps over K (the last one may be partial)
  int splits, kts;  // kts: steps per slice
  int epi, bias_f32;
};

// ------------------------------------------------------------------ epilogues (the siblings' expressions)
#pragma clang fp contract(off)
__device__ __forceinline__ float bias_at(const Params& p, int n) {
  return p.bias_f32 ? ((const float*)p.bias)[n] : bf2f(((const u16*)p.bias)[n]);
}
__device__ __forceinline__ float gelu_tanh(float z) {
  const float u = 0.7978845608028654f * (z + 0.044715f * z * z * z);
  const float t = 1.f - 2.f / (1.f + __expf(2.f * u));
  return 0.5f * z * (1.f + t);
}
// sum: the fp32 sum over K of column n, before the scale
__device__ __forceinline__ float epi_col(const Params& p, float sum, int n) {
  float v = sum * p.scale[n];
  if (p.epi >= 1) v = v + bias_at(p, n);
  if (p.epi == 2) v = gelu_tanh(v);
  return v;
}
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

// ------------------------------------------------------------------ main kernel
template <bool DIRECT>
__global__ __launch_bounds__(kThreads, 2) void rows_kernel(Params p) {
  constexpr int ROW = kChunkK + kRowPad;  // LDS row stride of A, bf16 elements
  // the A chunk [64][ROW] bf16 during the K loop, the workgroup's [64][128] fp32 sums after it
  __shared__ __attribute__((aligned(16))) u16 sA[kTileM * ROW];
  __shared__ __attribute__((aligned(16))) u8 sB[2][kStepK * kBRow];
  static_assert(sizeof(u16) * kTileM * ROW >= sizeof(float) * kTileM * kTileN, "sC lives in sA");
  float* sC = reinterpret_cast<float*>(sA);

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = lane & 15, kb = lane >> 4;  // B: column and k-slot; A: row c of a tile and k-slot
  const int split = blockIdx.z;
  const int row0 = blockIdx.y * kTileM;
  const int rows = p.M - row0 < kTileM ? p.M - row0 : kTileM;  // >= 1: the grid has ceil(M / 64) row tiles
  const int rt = (rows + 15) >> 4;                             // 16-row tiles that hold a row
  const int kt0 = split * p.kts;
  int kt1 = kt0 + p.kts;
  if (kt1 > p.KT) kt1 = p.KT;
  const int nsteps = kt1 > kt0 ? kt1 - kt0 : 0;  // the same for the four waves; 0: a slice past K
  const int K = p.K, N = p.N;
  const int n0 = blockIdx.x * kTileN;
  const u16* arow = p.a + (long)row0 * p.lda;

  // the thread's 16-byte pieces of a step: row (tid >> 3) + 32 i, piece tid & 7 of the 128 bytes
  const int pc = tid & 7, pr = tid >> 3;
  const int gcol = n0 + 16 * pc;
  const bool cvalid = gcol < N;
  const u32x4 zero4 = {0u, 0u, 0u, 0u};
  const u16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  // step t of the slice; k from K on and columns from N on are not read
  auto fetch = [&](int t, u32x4 (&w)[kLoads]) {
#pragma unroll
    for (int i = 0; i < kLoads; ++i) {
      const int k = (kt0 + t) * kStepK + pr + 32 * i;
      w[i] = (cvalid && k < K) ? *reinterpret_cast<const u32x4*>(p.q + (long)k * p.ldq + gcol) : zero4;
    }
  };

  // transposed read: lane l of a 16-lane block points at (row l / 2, bytes 8 (l % 2)..) of the block's 8 k
  const int troff = (8 * kb + (c >> 1)) * kBRow + 8 * (c & 1) + 32 * wave;

  f32x4 acc[kRowTiles][kStrips][2];
#pragma unroll
  for (int r = 0; r < kRowTiles; ++r)
#pragma unroll
    for (int s = 0; s < kStrips; ++s) acc[r][s][0] = acc[r][s][1] = f32x4{0.f, 0.f, 0.f, 0.f};

  u32x4 wq[kLoads];
  if (nsteps > 0) fetch(0, wq);
#pragma unroll 1
  for (int t = 0; t < nsteps; ++t) {
    constexpr int kPer = kChunkK / kStepK;
    if (t % kPer == 0) {
      // next chunk of A -> LDS; k >= K are zeros, rows >= M are not staged
      if (t > 0) __syncthreads();  // every wave is done with the previous chunk
      const long a0 = (long)(kt0 + t) * kStepK;
      for (int it = tid; it < rows * (kChunkK / 8); it += kThreads) {
        const int m = it / (kChunkK / 8), k8 = it % (kChunkK / 8);
        const long k = a0 + k8 * 8;
        u16x8 v = zero8;
        if (k < K) v = *reinterpret_cast<const u16x8*>(arow + (long)m * p.lda + k);
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
      if ((kt0 + t) * kStepK + kk * 32 < K) {  // uniform
        bf16x8 bv[kStrips];
#pragma unroll
        for (int s = 0; s < kStrips; ++s) {
          const u8* ad = sb + kk * 32 * kBRow + troff + 16 * s;
          bv[s] = cvt8(__builtin_amdgcn_ds_read_tr8_b64_v2i32((lds_i32x2*)ad));
        }
#pragma unroll
        for (int r = 0; r < kRowTiles; ++r) {
          if (r < rt) {  // uniform: a tile wholly beyond M costs nothing
            u16x8 av = zero8;  // rows M .. of the last tile: zeros made here
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
  __syncthreads();  // the last chunk of A has been read by every wave: sC takes its place
#pragma unroll
  for (int r = 0; r < kRowTiles; ++r) {
    if (r < rt) {
#pragma unroll
      for (int s = 0; s < kStrips; ++s) {
        const f32x4 sum = acc[r][s][0] + acc[r][s][1];
#pragma unroll
        for (int i = 0; i < 4; ++i) sC[(r * 16 + kb * 4 + i) * kTileN + (wave * kStrips + s) * 16 + c] = sum[i];
      }
    }
  }
  __syncthreads();

  if (!DIRECT) {
    for (int it = tid; it < rows * (kTileN / 8); it += kThreads) {
      const int m = it / (kTileN / 8), c0 = (it % (kTileN / 8)) * 8;
      const int n = n0 + c0;
      if (n >= N) continue;
      float o[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = sC[m * kTileN + c0 + j];
      store8(p.ws + ((long)split * p.M + row0 + m) * N + n, o);
    }
  } else if (p.epi == 3) {
    // 8 outputs per item: block b of 32 columns holds gate 0..15 | up 16..31
    for (int it = tid; it < rows * (kTileN / 16); it += kThreads) {
      const int m = it / (kTileN / 16), og = it % (kTileN / 16);
      const int gc = (og >> 1) * 32 + (og & 1) * 8;  // gate columns inside the workgroup's 128
      const int n = n0 + gc;
      if (n >= N) continue;
      float o[8];
#pragma unroll
      for (int j = 0; j < 8; ++j)
        o[j] = swiglu_val(sC[m * kTileN + gc + j] * p.scale[n + j], sC[m * kTileN + gc + 16 + j] * p.scale[n + 16 + j]);
      store8(p.c + (long)(row0 + m) * p.ldc + blockIdx.x * (kTileN / 2) + og * 8, o);
    }
  } else {
    for (int it = tid; it < rows * (kTileN / 8); it += kThreads) {
      const int m = it / (kTileN / 8), c0 = (it % (kTileN / 8)) * 8;
      const int n = n0 + c0;
      if (n >= N) continue;
      float o[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = epi_col(p, sC[m * kTileN + c0 + j], n + j);
      store8(p.c + (long)(row0 + m) * p.ldc + n, o);
    }
  }
}

// ------------------------------------------------------------------ split-K sum + epilogue
// one thread per output element: partials added in slice order, scale and epilogue in fp32, one
// rounding
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
    r = swiglu_val(g * p.scale[gc], u * p.scale[gc + 16]);
  } else {
    float v = src[o];
    for (int s = 1; s < p.splits; ++s) v = v + src[s * slab + o];
    r = epi_col(p, v, o);
  }
  p.c[(long)m * p.ldc + o] = f2bf(r);
}

}  // namespace rows_f8

// Whether pa_gemm_rows_f8 takes this problem.  Sizes, strides (lda, ldc in bf16 elements, ldq in
// bytes = codes) and addresses only: nothing is dereferenced.  The conditions of
// pa_gemm_skinny_f8_ok with M up to 256, K in whole 16s, and a partial slab that 32-bit element
// counts can index.
PA_EXPORT int pa_gemm_rows_f8_ok(int M, int N, int K, long lda, long ldq, long ldc, int epi, int num_splits,
                                 const void* a, const void* q, const void* c, const void* bias, const void* scale) {
  using rows_f8::kLimit;
  if (M < 1 || M > rows_f8::kMaxRows || N < 16 || N % 16 || K < 16 || K % 16) return 0;
  if (epi < 0 || epi > 3 || num_splits < 1 || num_splits > rows_f8::kMaxSplits) return 0;
  if ((epi == 1 || epi == 2) && bias == nullptr) return 0;
  if (epi == 3 && N % 32) return 0;
  const int nout = epi == 3 ? N / 2 : N;
  if (a == nullptr || q == nullptr || c == nullptr || scale == nullptr) return 0;
  if (((uintptr_t)a & 15) || ((uintptr_t)q & 15) || ((uintptr_t)c & 15) || ((uintptr_t)scale & 3)) return 0;
  if (lda < K || lda % 8 || ldq < N || ldq % 16 || ldc < nout || ldc % 8) return 0;
  if ((unsigned long)M * (unsigned long)lda * 2 >= kLimit || (unsigned long)M * (unsigned long)ldc * 2 >= kLimit ||
      (unsigned long)K * (unsigned long)ldq >= kLimit)
    return 0;
  if ((long)num_splits * M * N > 0x7FFFFFFFl) return 0;
  if (bias != nullptr && ((uintptr_t)bias & 3)) return 0;
  return 1;
}

// Split count from N and K alone (never from M: the summation order of an output element must
// not depend on the batch).  The partial slab is splits * M * N * 4 bytes, written and read
// once: at 256 rows every slice costs as much traffic as 2048 k of the codes, so K is cut far
// less than for the decode kernel -- the rule of pa_gemm_rows_mxfp4_splits: the largest power of
// two that keeps workgroups of the first 64-row tile (128 columns each) times splits at or below
// 512 (two resident workgroups on each of 256 compute units), with slices of at least 512 k, at
// most 8.
PA_EXPORT int pa_gemm_rows_f8_splits(int N, int K) {
  if (N < 1 || K < 16) return 1;
  const long wgs = ((long)N + rows_f8::kTileN - 1) / rows_f8::kTileN;
  long want = 1;
  while (want * 2 * wgs <= 512) want *= 2;
  while (want > 1 && want > K / rows_f8::kMinSliceK) want /= 2;
  if (want > 8) want = 8;
  return want < 1 ? 1 : (int)want;
}

// fp32 workspace elements pa_gemm_rows_f8 needs (none for a single slice)
PA_EXPORT int pa_gemm_rows_f8_ws_floats(int M, int N, int splits) {
  return splits > 1 ? splits * M * N : 0;
}

// C [M, ldc] bf16 = epilogue(scale * (A [M, lda] . q [K, ldq])).  ws: pa_gemm_rows_f8_ws_floats(M,
// N, num_splits) floats, 16-byte aligned.  A refused problem returns hipErrorInvalidValue and
// launches nothing.  No host synchronisation, no host read of device memory, no allocation:
// capturable into a HIP graph.
PA_EXPORT int pa_gemm_rows_f8(const void* a, const void* q, long ldq, const void* scale, void* c, const void* bias,
                              int bias_f32, float* ws, int M, int N, int K, long lda, long ldc, int epi,
                              int num_splits, hipStream_t st) {
  if (!pa_gemm_rows_f8_ok(M, N, K, lda, ldq, ldc, epi, num_splits, a, q, c, bias, scale))
    return (int)hipErrorInvalidValue;
  if (num_splits > 1 && (ws == nullptr || ((uintptr_t)ws & 15))) return (int)hipErrorInvalidValue;
  rows_f8::Params p;
  p.a = (const u16*)a; p.q = (const rows_f8::u8*)q; p.scale = (const float*)scale;
  p.c = (u16*)c; p.ws = num_splits > 1 ? ws : nullptr; p.bias = bias;
  p.lda = lda; p.ldq = ldq; p.ldc = ldc;
  p.M = M; p.N = N; p.K = K;
  p.KT = (K + rows_f8::kStepK - 1) / rows_f8::kStepK;
  p.splits = num_splits;
  p.kts = (p.KT + num_splits - 1) / num_splits;
  p.epi = epi; p.bias_f32 = bias_f32;
  const dim3 grid((N + rows_f8::kTileN - 1) / rows_f8::kTileN, (M + rows_f8::kTileM - 1) / rows_f8::kTileM,
                  num_splits);
  if (num_splits == 1) {
    hipLaunchKernelGGL(rows_f8::rows_kernel<true>, grid, dim3(rows_f8::kThreads), 0, st, p);
  } else {
    hipLaunchKernelGGL(rows_f8::rows_kernel<false>, grid, dim3(rows_f8::kThreads), 0, st, p);
    const long outs = (long)M * (epi == 3 ? N / 2 : N);
    hipLaunchKernelGGL(rows_f8::rows_sum_kernel, dim3((unsigned)((outs + 255) / 256)), dim3(256), 0, st, p);
  }
  PA_LAUNCH_CHECK();
}
