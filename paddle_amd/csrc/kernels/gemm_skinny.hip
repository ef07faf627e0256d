// Skinny-M GEMM for decode steps on gfx950: C[M, N] = epilogue(A[M, K] . B), bf16 operands,
// fp32 accumulation, 1 <= M <= 16 (any M, not only multiples of 8).
//
// A decode GEMM is a bandwidth problem: every weight byte is used by at most 16 rows, so the
// kernels below do one thing, stream B from HBM once with 16-byte loads, and keep everything
// else (A, partial sums) on chip.  B comes in the two layouts pa_gemm knows:
//
//   MN-major  B [K, ldb] (the [in, out] weight).  A workgroup owns a tile of 128 output
//             columns and one K slice.  A lane owns 8 adjacent columns (one 16-byte load of
//             a weight row; 16 lanes cover the tile's 256 contiguous bytes) and the four
//             16-lane groups of a wave times the four waves take different K rows: per step
//             a lane loads 8 consecutive K rows (128 B in flight per lane, 32 KiB per
//             workgroup -- the per-CU figure HBM streaming wants; the next step's rows are
//             fetched before the current ones are consumed).  The M rows of A are staged in
//             LDS in chunks of 1024 K values and read back as 16-byte broadcasts.
//             Accumulators: M x 8 fp32 per lane; lane groups are merged by shuffles, the
//             waves through LDS.
//   K-major   B [N, ldb] (a tied embedding table used as the head), any N >= 1.  A wave owns
//             4 output columns (rows of B) at a time, its lanes stride K with 16-byte loads,
//             A is staged in LDS, and the M x 4 dot products are reduced across the lanes by
//             a halving butterfly (63 shuffles for 64 values instead of 384).
//
// M 9..16 stays on the VALU as well: the inner product is written on float2 and lowers to
// v_pk_fma_f32.  An MFMA form would need B transposed through LDS for the MN-major layout and
// would change the summation order between M <= 8 and M > 8, which the batch-invariance
// contract below forbids.  Measured (profiles/skinny_gemm_bench.md) the VALU form wins up to
// 8 rows and loses to the MFMA GEMMs at 16, so ops/skinny.py routes at most 8 rows here; the
// kernel itself covers 16.  Row counts are rounded up to 1, 2, 4, 8 or 16 accumulator rows;
// the padding rows hold zeros and are never stored.
//
// Split-K follows attn_decode.hip: slice s of `num_splits` (a multiple of 8 K rows; a slice
// past the end of K contributes exact zeros) stores an fp32 partial [M, N] with plain stores
// into the caller's workspace [splits, M, N], and a second kernel adds the partials in split
// order, applies the epilogue in fp32 and rounds to bf16 once.  No atomics, flags or spins:
// the two launches on one stream are the only ordering.  num_splits == 1 writes C directly.
//
// Determinism and batch invariance: for a given (layout, N, K, num_splits) the K terms of one
// output element are always added in the same order -- per lane in ascending K, then the
// fixed shuffle tree, then waves 0..3, then splits 0..S-1 -- whatever M is, so row i of an
// M-row call equals the 1-row call on that row bit for bit, and two runs give the same bits.
// The epilogue functions are compiled with contraction off for the same reason.
//
// Epilogues (fp32, on the summed accumulator): 0 none, 1 + bias[N], 2 gelu_tanh(. + bias),
// 3 SwiGLU over gate|up interleaved in 16-column blocks (MN-major only, output [M, N/2]).
//
// All offsets are 64-bit: operands up to 4 GiB (byte offsets past 2^31) are covered.
#include "common.h"

using namespace pa;

namespace skinny {

constexpr int kThreads = 256;
constexpr int kWaves = 4;
constexpr int kMaxSplits = 1024;
constexpr unsigned long kLimit = 0xFFFFFF00ul;  // bytes per operand, as ops/gemm.py

typedef float f32x2 __attribute__((ext_vector_type(2)));

struct Params {
  const u16* a;
  const u16* b;
  u16* c;
  float* ws;         // [splits, M, N] fp32 partials (splits > 1)
  const void* bias;  // [N] or null
  long lda, ldb, ldc;
  int M, N, K;
  int splits, ks;  // ks: K rows per slice (multiple of 8)
  int epi, bias_f32;
  int groups;  // K-major: row groups per workgroup
};

// ------------------------------------------------------------------ epilogues
#pragma clang fp contract(off)
__device__ __forceinline__ float bias_at(const Params& p, int n) {
  return p.bias_f32 ? ((const float*)p.bias)[n] : bf2f(((const u16*)p.bias)[n]);
}
__device__ __forceinline__ float gelu_tanh(float z) {
  const float u = 0.7978845608028654f * (z + 0.044715f * z * z * z);
  const float t = 1.f - 2.f / (1.f + __expf(2.f * u));
  return 0.5f * z * (1.f + t);
}
// epilogues 0..2 on the summed accumulator of column n
__device__ __forceinline__ float epi_col(const Params& p, float v, int n) {
  if (p.epi >= 1) v = v + bias_at(p, n);
  if (p.epi == 2) v = gelu_tanh(v);
  return v;
}
__device__ __forceinline__ float swiglu_val(float g, float u) {
  return g / (1.f + __expf(-g)) * u;
}

// ------------------------------------------------------------------ MN-major B
constexpr int kTileN = 128;    // columns per workgroup
constexpr int kStepK = 128;    // K rows per workgroup step: 4 waves x 4 lane groups x 8 rows
constexpr int kChunkK = 1024;  // K values of A staged in LDS at a time (8 steps)

template <int MT, bool DIRECT>
__global__ __launch_bounds__(kThreads, 2) void mn_kernel(Params p) {
  // A chunk [MT][kChunkK] bf16, later the per-wave sums [4][MT][128] fp32: MT * 2 KiB each
  __shared__ __attribute__((aligned(16))) float s_buf[MT * 512];
  u16* sA = reinterpret_cast<u16*>(s_buf);
  constexpr bool PF = MT <= 8;
  constexpr int MH = MT < 8 ? MT : MT == 8 ? 8 : 4;  // accumulator rows per pass over a step

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int cg = lane & 15, kg = lane >> 4;
  const int col = blockIdx.x * kTileN + cg * 8;
  const bool col_ok = col < p.N;
  const int split = blockIdx.y;
  const long kbeg = (long)split * p.ks;
  long kend = kbeg + p.ks;
  if (kend > p.K) kend = p.K;
  const int nsteps = kend > kbeg ? (int)((kend - kbeg + kStepK - 1) / kStepK) : 0;

  f32x2 acc[MT][4];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[m][j] = f32x2{0.f, 0.f};

  const u16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  const u16* bcol = p.b + col;
  const int koff = wave * 32 + kg * 8;  // this lane's first K row inside a step

  u16x8 wc[8];
  {
    const long k0 = kbeg + koff;
    const bool v = col_ok && k0 < kend;
#pragma unroll
    for (int r = 0; r < 8; ++r) wc[r] = v ? *reinterpret_cast<const u16x8*>(bcol + (k0 + r) * p.ldb) : zero8;
  }

#pragma unroll 1
  for (int s = 0; s < nsteps; ++s) {
    if ((s & 7) == 0) {  // next chunk of A -> LDS; rows >= M and K values >= kend are zeros
      __syncthreads();
      const long a0 = kbeg + (long)s * kStepK;
      for (int it = tid; it < MT * (kChunkK / 8); it += kThreads) {
        const int m = it / (kChunkK / 8), k8 = it % (kChunkK / 8);
        const long k = a0 + k8 * 8;
        u16x8 v = zero8;
        if (m < p.M && k < kend) v = *reinterpret_cast<const u16x8*>(p.a + (long)m * p.lda + k);
        *reinterpret_cast<u16x8*>(sA + m * kChunkK + k8 * 8) = v;
      }
      __syncthreads();
    }
    // the next step's weight rows are in flight while this step's are consumed (at 16
    // accumulator rows the registers go to the accumulators instead and the second
    // resident workgroup of the CU covers the latency)
    u16x8 wn[PF ? 8 : 1];
    if (PF) {
      const long k0 = kbeg + (long)(s + 1) * kStepK + koff;
      const bool v = col_ok && k0 < kend;
#pragma unroll
      for (int r = 0; r < 8; ++r) wn[r] = v ? *reinterpret_cast<const u16x8*>(bcol + (k0 + r) * p.ldb) : zero8;
    } else if (s > 0) {
      const long k0 = kbeg + (long)s * kStepK + koff;
      const bool v = col_ok && k0 < kend;
#pragma unroll
      for (int r = 0; r < 8; ++r) wc[r] = v ? *reinterpret_cast<const u16x8*>(bcol + (k0 + r) * p.ldb) : zero8;
    }
    const u16* sa = sA + (s & 7) * kStepK + koff;
#pragma unroll
    for (int mh = 0; mh < MT; mh += MH) {
      u16x8 av[MH];
#pragma unroll
      for (int m = 0; m < MH; ++m) av[m] = *reinterpret_cast<const u16x8*>(sa + (mh + m) * kChunkK);
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        f32x2 wf[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) wf[j] = f32x2{bf2f(wc[r][2 * j]), bf2f(wc[r][2 * j + 1])};
#pragma unroll
        for (int m = 0; m < MH; ++m) {
          const float a = bf2f(av[m][r]);
          const f32x2 a2 = {a, a};
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[mh + m][j] = __builtin_elementwise_fma(a2, wf[j], acc[mh + m][j]);
        }
      }
    }
    if (PF) {
#pragma unroll
      for (int r = 0; r < 8; ++r) wc[r] = wn[r];
    }
  }

  // the four lane groups of a wave -> one sum (fixed tree: xor 16, then xor 32)
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      f32x2 v = acc[m][j];
      v.x += __shfl_xor(v.x, 16, 64);
      v.y += __shfl_xor(v.y, 16, 64);
      v.x += __shfl_xor(v.x, 32, 64);
      v.y += __shfl_xor(v.y, 32, 64);
      acc[m][j] = v;
    }
  __syncthreads();  // every wave is done reading A from s_buf
  if (kg == 0) {
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      float* d = s_buf + (wave * MT + m) * kTileN + cg * 8;
      *reinterpret_cast<f32x4*>(d) = f32x4{acc[m][0].x, acc[m][0].y, acc[m][1].x, acc[m][1].y};
      *reinterpret_cast<f32x4*>(d + 4) = f32x4{acc[m][2].x, acc[m][2].y, acc[m][3].x, acc[m][3].y};
    }
  }
  __syncthreads();

  // waves 0..3 in order -> the tile's sums; 8 adjacent columns of one row per item
  auto tile_sum8 = [&](int m, int c0, float (&o)[8]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float v = s_buf[(0 * MT + m) * kTileN + c0 + j];
#pragma unroll
      for (int w = 1; w < kWaves; ++w) v = v + s_buf[(w * MT + m) * kTileN + c0 + j];
      o[j] = v;
    }
  };
  if (!DIRECT) {
    for (int it = tid; it < p.M * 16; it += kThreads) {
      const int m = it >> 4, c0 = (it & 15) * 8;
      const int n = blockIdx.x * kTileN + c0;
      if (n >= p.N) continue;
      float o[8];
      tile_sum8(m, c0, o);
      store8(p.ws + ((long)split * p.M + m) * p.N + n, o);
    }
  } else if (p.epi == 3) {
    // 8 outputs per item: block b of 32 columns holds gate 0..15 | up 16..31
    for (int it = tid; it < p.M * 8; it += kThreads) {
      const int m = it >> 3, og = it & 7;
      const int gc = (og >> 1) * 32 + (og & 1) * 8;  // gate columns inside the tile
      if (blockIdx.x * kTileN + gc >= p.N) continue;
      float g[8], u[8], o[8];
      tile_sum8(m, gc, g);
      tile_sum8(m, gc + 16, u);
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = swiglu_val(g[j], u[j]);
      store8(p.c + (long)m * p.ldc + blockIdx.x * (kTileN / 2) + og * 8, o);
    }
  } else {
    for (int it = tid; it < p.M * 16; it += kThreads) {
      const int m = it >> 4, c0 = (it & 15) * 8;
      const int n = blockIdx.x * kTileN + c0;
      if (n >= p.N) continue;
      float o[8];
      tile_sum8(m, c0, o);
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = epi_col(p, o[j], n + j);
      store8(p.c + (long)m * p.ldc + n, o);
    }
  }
}

// ------------------------------------------------------------------ K-major B
constexpr int kRows = 4;  // output columns (rows of B) per wave at a time

template <int MT>
struct KChunk {  // K values of A in LDS at a time: at most 64 KiB, a multiple of 1024
  static constexpr int value = 32768 / MT < 8192 ? 32768 / MT : 8192;
};

// Halving butterfly over the 64 lanes: stage `O` exchanges half of the CNT live values with
// lane ^ O and adds, so the value count halves while the lanes covered double; once one value
// is left the remaining stages are the plain butterfly.  The tree (xor 32, 16, .., 1) is the
// same for every CNT.  Afterwards v[0] of lane L is the sum of value index L >> (6 - log2 CNT).
template <int CNT, int O>
struct Fold {
  template <int N>
  static __device__ __forceinline__ void run(float (&v)[N], int lane) {
    if constexpr (CNT > 1) {
      constexpr int H = CNT / 2;
      const bool up = (lane & O) != 0;
#pragma unroll
      for (int i = 0; i < H; ++i) {
        const float send = up ? v[i] : v[i + H];
        const float keep = up ? v[i + H] : v[i];
        v[i] = keep + __shfl_xor(send, O, 64);
      }
      if constexpr (O > 1) Fold<H, O / 2>::run(v, lane);
    } else {
      v[0] = v[0] + __shfl_xor(v[0], O, 64);
      if constexpr (O > 1) Fold<1, O / 2>::run(v, lane);
    }
  }
};

constexpr int ilog2(int x) { return x <= 1 ? 0 : 1 + ilog2(x / 2); }

template <int MT, bool DIRECT>
__global__ __launch_bounds__(kThreads, 2) void km_kernel(Params p) {
  constexpr int KCH = KChunk<MT>::value;
  constexpr int CNT = MT * kRows;
  constexpr int U = MT <= 8 ? 2 : 1;  // 512-wide K steps in flight per lane
  __shared__ __attribute__((aligned(16))) u16 sA[MT * KCH];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int split = blockIdx.y;
  const long kbeg = (long)split * p.ks;
  long kend = kbeg + p.ks;
  if (kend > p.K) kend = p.K;
  const bool one_chunk = kend - kbeg <= KCH;
  const u16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};

#pragma unroll 1
  for (int g = 0; g < p.groups; ++g) {
    const long n0 = (((long)blockIdx.x * p.groups + g) * kWaves + wave) * kRows;
    const u16* brow[kRows];
    bool row_ok[kRows];
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
      row_ok[r] = n0 + r < p.N;
      brow[r] = p.b + (row_ok[r] ? n0 + r : 0) * p.ldb;
    }
    float acc[CNT];
#pragma unroll
    for (int i = 0; i < CNT; ++i) acc[i] = 0.f;

#pragma unroll 1
    for (long a0 = kbeg; a0 < kend; a0 += KCH) {
      const int klen = kend - a0 < KCH ? (int)(kend - a0) : KCH;
      if (!(one_chunk && g > 0)) {  // A [M, a0 .. a0 + klen) -> LDS (rows >= M: zeros)
        __syncthreads();
        for (int it = tid; it < MT * (klen / 8); it += kThreads) {
          const int m = it / (klen / 8), k8 = it % (klen / 8);
          u16x8 v = zero8;
          if (m < p.M) v = *reinterpret_cast<const u16x8*>(p.a + (long)m * p.lda + a0 + k8 * 8);
          *reinterpret_cast<u16x8*>(sA + m * KCH + k8 * 8) = v;
        }
        __syncthreads();
      }
#pragma unroll 1
      for (int kk = lane * 8; kk < klen; kk += 512 * U) {
        u16x8 w[U][kRows];
        bool valid[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int kv = kk + u * 512;
          valid[u] = kv < klen;
#pragma unroll
          for (int r = 0; r < kRows; ++r)
            w[u][r] = valid[u] && row_ok[r] ? *reinterpret_cast<const u16x8*>(brow[r] + a0 + kv) : zero8;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if (!valid[u]) continue;
          const int kv = kk + u * 512;
          float wf[kRows][8];
#pragma unroll
          for (int r = 0; r < kRows; ++r)
#pragma unroll
            for (int j = 0; j < 8; ++j) wf[r][j] = bf2f(w[u][r][j]);
#pragma unroll
          for (int m = 0; m < MT; ++m) {
            const u16x8 av = *reinterpret_cast<const u16x8*>(sA + m * KCH + kv);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              const float a = bf2f(av[j]);
#pragma unroll
              for (int r = 0; r < kRows; ++r) acc[m * kRows + r] = fmaf(a, wf[r][j], acc[m * kRows + r]);
            }
          }
        }
      }
    }

    Fold<CNT, 32>::run(acc, lane);
    constexpr int SH = 6 - ilog2(CNT);
    const int idx = lane >> SH;
    const int m = idx / kRows;
    const long n = n0 + idx % kRows;
    if ((lane & ((1 << SH) - 1)) == 0 && m < p.M && n < p.N) {
      if (DIRECT) p.c[(long)m * p.ldc + n] = f2bf(epi_col(p, acc[0], (int)n));
      else p.ws[((long)split * p.M + m) * p.N + n] = acc[0];
    }
  }
}

// ------------------------------------------------------------------ split-K sum + epilogue
// one thread per output element: partials added in split order, epilogue in fp32, one rounding
__global__ __launch_bounds__(256) void sum_kernel(Params p) {
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

template <bool DIRECT>
static void launch_main(const Params& p, int b_kmaj, hipStream_t st) {
  const int mt = p.M <= 1 ? 1 : p.M <= 2 ? 2 : p.M <= 4 ? 4 : p.M <= 8 ? 8 : 16;
  if (!b_kmaj) {
    const dim3 grid((p.N + kTileN - 1) / kTileN, p.splits);
    switch (mt) {
      case 1: hipLaunchKernelGGL((mn_kernel<1, DIRECT>), grid, dim3(kThreads), 0, st, p); break;
      case 2: hipLaunchKernelGGL((mn_kernel<2, DIRECT>), grid, dim3(kThreads), 0, st, p); break;
      case 4: hipLaunchKernelGGL((mn_kernel<4, DIRECT>), grid, dim3(kThreads), 0, st, p); break;
      case 8: hipLaunchKernelGGL((mn_kernel<8, DIRECT>), grid, dim3(kThreads), 0, st, p); break;
      default: hipLaunchKernelGGL((mn_kernel<16, DIRECT>), grid, dim3(kThreads), 0, st, p); break;
    }
  } else {
    const long per_wg = (long)p.groups * kWaves * kRows;
    const dim3 grid((unsigned)((p.N + per_wg - 1) / per_wg), p.splits);
    switch (mt) {
      case 1: hipLaunchKernelGGL((km_kernel<1, DIRECT>), grid, dim3(kThreads), 0, st, p); break;
      case 2: hipLaunchKernelGGL((km_kernel<2, DIRECT>), grid, dim3(kThreads), 0, st, p); break;
      case 4: hipLaunchKernelGGL((km_kernel<4, DIRECT>), grid, dim3(kThreads), 0, st, p); break;
      case 8: hipLaunchKernelGGL((km_kernel<8, DIRECT>), grid, dim3(kThreads), 0, st, p); break;
      default: hipLaunchKernelGGL((km_kernel<16, DIRECT>), grid, dim3(kThreads), 0, st, p); break;
    }
  }
}

}  // namespace skinny

// Whether pa_gemm_skinny takes this problem.  Sizes, element strides and addresses only:
// nothing is dereferenced.  epi: 0 none, 1 bias, 2 bias + gelu_tanh, 3 SwiGLU (interleaved).
PA_EXPORT int pa_gemm_skinny_ok(int b_kmaj, int M, int N, int K, long lda, long ldb, long ldc, int epi,
                                int num_splits, const void* a, const void* b, const void* c, const void* bias) {
  using skinny::kLimit;
  if (M < 1 || M > 16 || N < 1 || K < 8 || K % 8) return 0;
  if (epi < 0 || epi > 3 || num_splits < 1 || num_splits > skinny::kMaxSplits) return 0;
  if ((epi == 1 || epi == 2) && bias == nullptr) return 0;
  const int nout = epi == 3 ? N / 2 : N;
  if (lda < K || lda % 8 || ldc < nout || ((uintptr_t)a & 15) || ((uintptr_t)b & 15) || a == nullptr ||
      b == nullptr || c == nullptr)
    return 0;
  if ((unsigned long)M * (unsigned long)lda * 2 >= kLimit || (unsigned long)M * (unsigned long)ldc * 2 >= kLimit)
    return 0;
  if (b_kmaj) {
    if (epi == 3 || ldb < K || ldb % 8 || ((uintptr_t)c & 1)) return 0;
    if ((unsigned long)N * (unsigned long)ldb * 2 >= kLimit) return 0;
  } else {
    if (N % 8 || ldb < N || ldb % 8 || ldc % 8 || ((uintptr_t)c & 15)) return 0;
    if (epi == 3 && N % 32) return 0;
    if ((unsigned long)K * (unsigned long)ldb * 2 >= kLimit) return 0;
  }
  if (bias != nullptr && ((uintptr_t)bias & 3)) return 0;
  return 1;
}

// Split count from the layout, N and K alone (never from M: the summation order of an output
// element must not depend on the batch).  MN-major: the power of two nearest (in ratio) to
// 512 / (128-column tiles) -- measured best or within 7 % of it on the llama-7b products
// (profiles/skinny_gemm_bench.md); powers of two keep the slices of the usual K whole
// 128-row steps; slices of at least 256 K rows.  K-major: 16 outputs per workgroup; K is cut
// only where N alone cannot fill the chip.
PA_EXPORT int pa_gemm_skinny_splits(int b_kmaj, int N, int K) {
  if (N < 1 || K < 8) return 1;
  long want;
  if (b_kmaj) {
    const long units = ((long)N + 15) / 16;
    want = (512 + units - 1) / units;
    if (want > K / 1024) want = K / 1024;
  } else {
    const long tiles = ((long)N + skinny::kTileN - 1) / skinny::kTileN;
    want = 1;
    while (want * 2 * tiles <= 512) want *= 2;
    if (512l * 512l > 2 * (want * tiles) * (want * tiles)) want *= 2;  // 512 / tiles > want * sqrt(2)
    while (want > 1 && want > K / 256) want /= 2;
  }
  if (want > 64) want = 64;
  return want < 1 ? 1 : (int)want;
}

// fp32 workspace elements pa_gemm_skinny needs (none for a single slice)
PA_EXPORT int pa_gemm_skinny_ws_floats(int M, int N, int splits) {
  return splits > 1 ? splits * M * N : 0;
}

// C [M, ldc] bf16 = epilogue(A [M, lda] . B); B [K, ldb] (b_kmaj 0) or [N, ldb] (b_kmaj 1).
// ws: pa_gemm_skinny_ws_floats(M, N, num_splits) floats.  A refused problem returns
// hipErrorInvalidValue and launches nothing.  No host synchronisation, no host read of
// device memory: capturable into a HIP graph.
PA_EXPORT int pa_gemm_skinny(int b_kmaj, const void* a, const void* b, void* c, const void* bias, int bias_f32,
                             float* ws, int M, int N, int K, long lda, long ldb, long ldc, int epi,
                             int num_splits, hipStream_t st) {
  if (!pa_gemm_skinny_ok(b_kmaj, M, N, K, lda, ldb, ldc, epi, num_splits, a, b, c, bias))
    return (int)hipErrorInvalidValue;
  if (num_splits > 1 && (ws == nullptr || (long)num_splits * M * N > 0x7FFFFFFFl)) return (int)hipErrorInvalidValue;
  skinny::Params p;
  p.a = (const u16*)a; p.b = (const u16*)b; p.c = (u16*)c; p.ws = ws; p.bias = bias;
  p.lda = lda; p.ldb = ldb; p.ldc = ldc;
  p.M = M; p.N = N; p.K = K;
  p.splits = num_splits;
  p.ks = ((K / 8 + num_splits - 1) / num_splits) * 8;
  p.epi = epi; p.bias_f32 = bias_f32;
  // K-major: a workgroup keeps its slice of A in LDS over several 16-column groups when the
  // slice fits one chunk; at least ~1024 workgroups stay
  const long blocks = ((long)N + 15) / 16;
  p.groups = (int)(blocks / 1024 < 1 ? 1 : blocks / 1024 > 8 ? 8 : blocks / 1024);
  if (num_splits == 1) {
    skinny::launch_main<true>(p, b_kmaj, st);
  } else {
    skinny::launch_main<false>(p, b_kmaj, st);
    const long outs = (long)M * (epi == 3 ? N / 2 : N);
    hipLaunchKernelGGL(skinny::sum_kernel, dim3((unsigned)((outs + 255) / 256)), dim3(256), 0, st, p);
  }
  PA_LAUNCH_CHECK();
}
