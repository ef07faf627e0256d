// FP8 weight-only skinny-M GEMM for decode steps on gfx950:
//
//   C[M, nout] bf16 = epilogue(scale[n] * sum_k A[m, k] * Bq[k, n])
//
// A [M, lda] bf16, Bq [K, ldb] OCP e4m3 codes (the [in, out] weight, MN-major only), scale [N]
// fp32 (one per output column), 1 <= M <= 16.  The sibling of gemm_skinny.hip's mn_kernel: the
// weight bytes are the traffic, so they are streamed from HBM once with 16-byte loads and
// everything else stays on chip.
//
// Arithmetic, all fp32: v_cvt_pk_f32_fp8 turns two codes into two floats (exact), the inner
// product runs on float2 (v_pk_fma_f32), the summed accumulator is multiplied by scale[n], then
// bias, then the activation, then one rounding to bf16.  The kernel takes any finite scale; the
// quantiser's powers of two make q * scale exact in bf16, which is what lets a quantised model
// be compared bit for bit with a bf16 twin (ops/skinny_fp8.py).
//
// Geometry.  A 16-byte load holds 16 columns of one weight row, so a lane owns 16 adjacent
// columns and M x 16 fp32 accumulators.  CL lanes cover a tile of CL * 16 columns (contiguous
// bytes of a row), the 64 / CL lane groups of a wave times the four waves take different K
// rows, 8 consecutive rows per lane and step:
//
//   CL 16: 256-column tiles, 128 K rows per workgroup step      (the default, kTileDefault)
//   CL  8: 128-column tiles, 256 K rows per workgroup step
//
// (pa_gemm_skinny_f8_set_tile switches, for benchmarks/skinny_fp8_bench.py; the measurements
// behind the default are in profiles/skinny_fp8_bench.md.)  The rows a lane needs next are in
// flight while the current ones are consumed: 8 rows ahead up to 4 accumulator rows, 4 rows
// ahead at 8, where the 128 accumulators leave fewer registers.  The M rows of A are staged in
// LDS in chunks of 1024 K values and read back as broadcasts.  More than 8 rows would need 256
// accumulators per lane: M 9..16 runs as two passes of up to 8 rows (the weight is read twice,
// which still beats dequantising it: profiles/skinny_fp8_bench.md).
//
// Split-K, determinism and batch invariance are gemm_skinny.hip's: slice s of `num_splits` (a
// multiple of 8 K rows; a slice past the end of K contributes exact zeros) stores a raw fp32
// partial [M, N] with plain stores into the caller's workspace, a second kernel adds the
// partials in split order, scales, applies the epilogue and rounds once.  No atomics, flags or
// spins.  For a given (tile, N, K, num_splits) the K terms of an output element are added in
// one order -- per lane in ascending K, the fixed shuffle tree, waves 0..3, splits 0..S-1 --
// whatever M is: row i of an M-row call equals the 1-row call bit for bit.
//
// Epilogues: 0 none, 1 + bias[N], 2 gelu_tanh(. + bias), 3 SwiGLU over gate|up interleaved in
// 16-column blocks (output [M, N/2]; gate and up columns each take their own scale).
//
// All offsets are 64-bit (operands up to 4 GiB); nothing outside the operands is read or
// written.
//
// pa_fp8w_dequant: out[K, N] bf16 = q * scale[n] (fp32 product, one rounding; exact for the
// quantiser's power-of-two scales), 16-byte loads and stores.
#include "common.h"

using namespace pa;

namespace skinny_f8 {

constexpr int kThreads = 256;
constexpr int kWaves = 4;
constexpr int kMaxSplits = 1024;
constexpr int kChunkK = 1024;  // K values of A staged in LDS at a time
constexpr unsigned long kLimit = 0xFFFFFF00ul;  // bytes per operand, as pa_gemm_skinny_ok
constexpr int kTileDefault = 256;

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint8_t u8;

static int g_tile = kTileDefault;

struct Params {
  const u16* a;
  const u8* b;
  const float* scale;  // [N]
  u16* c;
  float* ws;         // [splits, M, N] raw fp32 partials (splits > 1)
  const void* bias;  // [N] or null
  long lda, ldb, ldc;
  int M, N, K;
  int splits, ks;  // ks: K rows per slice (multiple of 8)
  int epi, bias_f32;
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
// scale, then epilogues 0..2, on the summed accumulator of column n
__device__ __forceinline__ float epi_col(const Params& p, float v, int n) {
  v = v * p.scale[n];
  if (p.epi >= 1) v = v + bias_at(p, n);
  if (p.epi == 2) v = gelu_tanh(v);
  return v;
}
__device__ __forceinline__ float swiglu_val(float g, float u) {
  return g / (1.f + __expf(-g)) * u;
}

template <int R>
struct U16V;
template <>
struct U16V<8> { typedef u16x8 type; };
template <>
struct U16V<4> { typedef u16x4 type; };

// ------------------------------------------------------------------ main kernel
template <int MT, int CL, bool DIRECT>
__global__ __launch_bounds__(kThreads, 2) void f8_kernel(Params p) {
  constexpr int TILE = CL * 16;             // columns per workgroup
  constexpr int KG = 64 / CL;               // lane groups of a wave over K
  constexpr int STEP = kWaves * KG * 8;     // K rows per workgroup step
  constexpr int SPC = kChunkK / STEP;       // steps per chunk of A
  constexpr int RH = MT <= 4 ? 8 : 4;       // weight rows fetched (and consumed) at a time
  constexpr int NH = 8 / RH;                // ticks per step
  constexpr int A_FLOATS = MT * kChunkK / 2, S_FLOATS = kWaves * MT * TILE;
  // A chunk [MT][kChunkK] bf16, later the per-wave sums [4][MT][TILE] fp32
  __shared__ __attribute__((aligned(16))) float s_buf[A_FLOATS > S_FLOATS ? A_FLOATS : S_FLOATS];
  u16* sA = reinterpret_cast<u16*>(s_buf);
  typedef typename U16V<RH>::type avec;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int cg = lane % CL, kg = lane / CL;
  const int col = blockIdx.x * TILE + cg * 16;
  const bool col_ok = col < p.N;
  const int split = blockIdx.y;
  const long kbeg = (long)split * p.ks;
  long kend = kbeg + p.ks;
  if (kend > p.K) kend = p.K;
  const int nsteps = kend > kbeg ? (int)((kend - kbeg + STEP - 1) / STEP) : 0;
  const int nticks = nsteps * NH;

  f32x2 acc[MT][8];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[m][j] = f32x2{0.f, 0.f};

  const u32x4 zero4 = {0u, 0u, 0u, 0u};
  const u16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  const u8* bcol = p.b + col;
  const int koff = wave * (KG * 8) + kg * 8;  // this lane's first K row inside a step

  // the RH weight rows of tick t (rows at or past kend, and columns past N: zeros, not read;
  // K, the slice length and a lane's row offset are multiples of 8, so the rows of a tick are
  // inside the slice together or not at all)
  auto fetch = [&](int t, u32x4 (&w)[RH]) {
    const long k0 = kbeg + (long)(t / NH) * STEP + koff + (t % NH) * RH;
    const bool v = col_ok && k0 < kend;
#pragma unroll
    for (int r = 0; r < RH; ++r) w[r] = v ? *reinterpret_cast<const u32x4*>(bcol + (k0 + r) * p.ldb) : zero4;
  };

  u32x4 wc[RH];
  fetch(0, wc);

#pragma unroll 1
  for (int t = 0; t < nticks; ++t) {
    const int s = t / NH;
    if (t % (SPC * NH) == 0) {  // next chunk of A -> LDS; rows >= M and K values >= kend are zeros
      __syncthreads();
      const long a0 = kbeg + (long)s * STEP;
      for (int it = tid; it < MT * (kChunkK / 8); it += kThreads) {
        const int m = it / (kChunkK / 8), k8 = it % (kChunkK / 8);
        const long k = a0 + k8 * 8;
        u16x8 v = zero8;
        if (m < p.M && k < kend) v = *reinterpret_cast<const u16x8*>(p.a + (long)m * p.lda + k);
        *reinterpret_cast<u16x8*>(sA + m * kChunkK + k8 * 8) = v;
      }
      __syncthreads();
    }
    u32x4 wn[RH];
    fetch(t + 1, wn);  // in flight while wc is consumed
    const u16* sa = sA + (s % SPC) * STEP + koff + (t % NH) * RH;
    avec av[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) av[m] = *reinterpret_cast<const avec*>(sa + m * kChunkK);
#pragma unroll
    for (int r = 0; r < RH; ++r) {
      f32x2 wf[8];
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        wf[2 * d] = __builtin_amdgcn_cvt_pk_f32_fp8(wc[r][d], false);
        wf[2 * d + 1] = __builtin_amdgcn_cvt_pk_f32_fp8(wc[r][d], true);
      }
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        const float a = bf2f(av[m][r]);
        const f32x2 a2 = {a, a};
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[m][j] = __builtin_elementwise_fma(a2, wf[j], acc[m][j]);
      }
    }
#pragma unroll
    for (int r = 0; r < RH; ++r) wc[r] = wn[r];
  }

  // the lane groups of a wave -> one sum (fixed tree: xor CL, 2 CL, .., 32)
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      f32x2 v = acc[m][j];
#pragma unroll
      for (int o = CL; o < 64; o *= 2) {
        v.x += __shfl_xor(v.x, o, 64);
        v.y += __shfl_xor(v.y, o, 64);
      }
      acc[m][j] = v;
    }
  __syncthreads();  // every wave is done reading A from s_buf
  if (kg == 0) {
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      float* d = s_buf + (wave * MT + m) * TILE + cg * 16;
#pragma unroll
      for (int q = 0; q < 4; ++q)
        *reinterpret_cast<f32x4*>(d + 4 * q) =
            f32x4{acc[m][2 * q].x, acc[m][2 * q].y, acc[m][2 * q + 1].x, acc[m][2 * q + 1].y};
    }
  }
  __syncthreads();

  // waves 0..3 in order -> the tile's sums; 8 adjacent columns of one row per item
  auto tile_sum8 = [&](int m, int c0, float (&o)[8]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float v = s_buf[(0 * MT + m) * TILE + c0 + j];
#pragma unroll
      for (int w = 1; w < kWaves; ++w) v = v + s_buf[(w * MT + m) * TILE + c0 + j];
      o[j] = v;
    }
  };
  constexpr int G8 = TILE / 8;
  if (!DIRECT) {
    for (int it = tid; it < p.M * G8; it += kThreads) {
      const int m = it / G8, c0 = (it % G8) * 8;
      const int n = blockIdx.x * TILE + c0;
      if (n >= p.N) continue;
      float o[8];
      tile_sum8(m, c0, o);
      store8(p.ws + ((long)split * p.M + m) * p.N + n, o);
    }
  } else if (p.epi == 3) {
    // 8 outputs per item: block b of 32 columns holds gate 0..15 | up 16..31
    constexpr int G16 = TILE / 16;
    for (int it = tid; it < p.M * G16; it += kThreads) {
      const int m = it / G16, og = it % G16;
      const int gc = (og >> 1) * 32 + (og & 1) * 8;  // gate columns inside the tile
      const int n = blockIdx.x * TILE + gc;
      if (n >= p.N) continue;
      float g[8], u[8], o[8];
      tile_sum8(m, gc, g);
      tile_sum8(m, gc + 16, u);
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = swiglu_val(g[j] * p.scale[n + j], u[j] * p.scale[n + 16 + j]);
      store8(p.c + (long)m * p.ldc + blockIdx.x * (TILE / 2) + og * 8, o);
    }
  } else {
    for (int it = tid; it < p.M * G8; it += kThreads) {
      const int m = it / G8, c0 = (it % G8) * 8;
      const int n = blockIdx.x * TILE + c0;
      if (n >= p.N) continue;
      float o[8];
      tile_sum8(m, c0, o);
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = epi_col(p, o[j], n + j);
      store8(p.c + (long)m * p.ldc + n, o);
    }
  }
}

// ------------------------------------------------------------------ split-K sum + epilogue
// one thread per output element: partials added in split order, scale and epilogue in fp32,
// one rounding
__global__ __launch_bounds__(256) void f8_sum_kernel(Params p) {
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

template <int CL, bool DIRECT>
static void launch_main(const Params& p, hipStream_t st) {
  const dim3 grid((p.N + CL * 16 - 1) / (CL * 16), p.splits);
  const int mt = p.M <= 1 ? 1 : p.M <= 2 ? 2 : p.M <= 4 ? 4 : 8;
  switch (mt) {
    case 1: hipLaunchKernelGGL((f8_kernel<1, CL, DIRECT>), grid, dim3(kThreads), 0, st, p); break;
    case 2: hipLaunchKernelGGL((f8_kernel<2, CL, DIRECT>), grid, dim3(kThreads), 0, st, p); break;
    case 4: hipLaunchKernelGGL((f8_kernel<4, CL, DIRECT>), grid, dim3(kThreads), 0, st, p); break;
    default: hipLaunchKernelGGL((f8_kernel<8, CL, DIRECT>), grid, dim3(kThreads), 0, st, p); break;
  }
}

// ------------------------------------------------------------------ dequantiser
// one item = 16 adjacent columns of one row: a 16-byte load of codes, two 16-byte stores
__global__ __launch_bounds__(256) void dequant_kernel(const u8* q, const float* scale, u16* out, long K, long N,
                                                      long ldq, long ldo) {
  const long per_row = N / 16, items = K * per_row;
  for (long it = (long)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += (long)gridDim.x * blockDim.x) {
    const long k = it / per_row, n = (it % per_row) * 16;
    const u32x4 w = *reinterpret_cast<const u32x4*>(q + k * ldq + n);
    float o[16];
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8(w[d], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8(w[d], true);
      o[4 * d] = lo.x; o[4 * d + 1] = lo.y; o[4 * d + 2] = hi.x; o[4 * d + 3] = hi.y;
    }
    float lo8[8], hi8[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      lo8[j] = o[j] * scale[n + j];
      hi8[j] = o[8 + j] * scale[n + 8 + j];
    }
    store8(out + k * ldo + n, lo8);
    store8(out + k * ldo + n + 8, hi8);
  }
}

}  // namespace skinny_f8

// Column tile of the main kernel: 256 (16 lanes x 16 columns, the default) or 128.  A
// benchmark switch; the split rule follows it.  Returns the tile now in force.
PA_EXPORT int pa_gemm_skinny_f8_set_tile(int cols) {
  if (cols == 128 || cols == 256) skinny_f8::g_tile = cols;
  return skinny_f8::g_tile;
}

// Whether pa_gemm_skinny_f8 takes this problem.  Sizes, strides (lda, ldc in bf16 elements, ldb
// in bytes = codes) and addresses only: nothing is dereferenced.
PA_EXPORT int pa_gemm_skinny_f8_ok(int M, int N, int K, long lda, long ldb, long ldc, int epi, int num_splits,
                                   const void* a, const void* b, const void* c, const void* bias,
                                   const void* scale) {
  using skinny_f8::kLimit;
  if (M < 1 || M > 16 || N < 16 || N % 16 || K < 8 || K % 8) return 0;
  if (epi < 0 || epi > 3 || num_splits < 1 || num_splits > skinny_f8::kMaxSplits) return 0;
  if ((epi == 1 || epi == 2) && bias == nullptr) return 0;
  if (epi == 3 && N % 32) return 0;
  const int nout = epi == 3 ? N / 2 : N;
  if (a == nullptr || b == nullptr || c == nullptr || scale == nullptr) return 0;
  if (((uintptr_t)a & 15) || ((uintptr_t)b & 15) || ((uintptr_t)c & 15) || ((uintptr_t)scale & 3)) return 0;
  if (lda < K || lda % 8 || ldb < N || ldb % 16 || ldc < nout || ldc % 8) return 0;
  if ((unsigned long)M * (unsigned long)lda * 2 >= kLimit || (unsigned long)M * (unsigned long)ldc * 2 >= kLimit ||
      (unsigned long)K * (unsigned long)ldb >= kLimit)
    return 0;
  if (bias != nullptr && ((uintptr_t)bias & 3)) return 0;
  return 1;
}

// Split count from N and K alone (never from M: the summation order of an output element must
// not depend on the batch): the largest power of two that keeps tiles * splits below 512 (two
// resident workgroups on each of 256 compute units), with slices of at least 256 K rows, at
// most 64.  This kernel's own rule, not the bf16 kernel's: a tile holds half the bytes, and
// the forced-split sweep (profiles/skinny_fp8_bench.md) has its minimum at 250 to 400
// workgroups on all five llama-7b products, at 1 row and at 8.
PA_EXPORT int pa_gemm_skinny_f8_splits(int N, int K) {
  if (N < 1 || K < 8) return 1;
  const long tiles = ((long)N + skinny_f8::g_tile - 1) / skinny_f8::g_tile;
  long want = 1;
  while (want * 2 * tiles < 512) want *= 2;
  while (want > 1 && want > K / 256) want /= 2;
  if (want > 64) want = 64;
  return want < 1 ? 1 : (int)want;
}

// fp32 workspace elements pa_gemm_skinny_f8 needs (none for a single slice)
PA_EXPORT int pa_gemm_skinny_f8_ws_floats(int M, int N, int splits) {
  return splits > 1 ? splits * M * N : 0;
}

// C [M, ldc] bf16 = epilogue(scale * (A [M, lda] . Bq [K, ldb])).  ws:
// pa_gemm_skinny_f8_ws_floats(M, N, num_splits) floats.  A refused problem returns
// hipErrorInvalidValue and launches nothing.  No host synchronisation, no host read of device
// memory: capturable into a HIP graph.
PA_EXPORT int pa_gemm_skinny_f8(const void* a, const void* b, const void* scale, void* c, const void* bias,
                                int bias_f32, float* ws, int M, int N, int K, long lda, long ldb, long ldc, int epi,
                                int num_splits, hipStream_t st) {
  if (!pa_gemm_skinny_f8_ok(M, N, K, lda, ldb, ldc, epi, num_splits, a, b, c, bias, scale))
    return (int)hipErrorInvalidValue;
  if (num_splits > 1 && (ws == nullptr || (long)num_splits * M * N > 0x7FFFFFFFl)) return (int)hipErrorInvalidValue;
  skinny_f8::Params p;
  p.b = (const skinny_f8::u8*)b; p.scale = (const float*)scale; p.bias = bias;
  p.lda = lda; p.ldb = ldb; p.ldc = ldc;
  p.N = N; p.K = K;
  p.splits = num_splits;
  p.ks = ((K / 8 + num_splits - 1) / num_splits) * 8;
  p.epi = epi; p.bias_f32 = bias_f32;
  const int tile = skinny_f8::g_tile;
  for (int m0 = 0; m0 < M; m0 += 8) {  // passes of up to 8 rows, each with its own slab of ws
    p.M = M - m0 < 8 ? M - m0 : 8;
    p.a = (const u16*)a + (long)m0 * lda;
    p.c = (u16*)c + (long)m0 * ldc;
    p.ws = num_splits > 1 ? ws + (long)num_splits * m0 * N : nullptr;
    if (num_splits == 1) {
      if (tile == 256) skinny_f8::launch_main<16, true>(p, st);
      else skinny_f8::launch_main<8, true>(p, st);
    } else {
      if (tile == 256) skinny_f8::launch_main<16, false>(p, st);
      else skinny_f8::launch_main<8, false>(p, st);
      const long outs = (long)p.M * (epi == 3 ? N / 2 : N);
      hipLaunchKernelGGL(skinny_f8::f8_sum_kernel, dim3((unsigned)((outs + 255) / 256)), dim3(256), 0, st, p);
    }
  }
  PA_LAUNCH_CHECK();
}

// out [K, ldo] bf16 = q [K, ldq] e4m3 * scale[n].  N % 16 == 0, 16-byte aligned rows.
PA_EXPORT int pa_fp8w_dequant(const void* q, const void* scale, void* out, long K, long N, long ldq, long ldo,
                              hipStream_t st) {
  if (K < 1 || N < 16 || N % 16 || ldq < N || ldq % 16 || ldo < N || ldo % 8 || q == nullptr || scale == nullptr ||
      out == nullptr || ((uintptr_t)q & 15) || ((uintptr_t)out & 15) || ((uintptr_t)scale & 3))
    return (int)hipErrorInvalidValue;
  const long items = K * (N / 16);
  hipLaunchKernelGGL(skinny_f8::dequant_kernel, dim3(stream_grid(items, 256)), dim3(256), 0, st,
                     (const skinny_f8::u8*)q, (const float*)scale, (u16*)out, K, N, ldq, ldo);
  PA_LAUNCH_CHECK();
}
