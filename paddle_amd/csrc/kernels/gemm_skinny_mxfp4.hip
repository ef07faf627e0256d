// MXFP4 weight-only skinny-M GEMM for decode steps on gfx950:
//
//   C[M, nout] bf16 = epilogue(sum_k A[m, k] * dq[k, n]),   dq[k, n] = e2m1(code[k, n]) * 2^(e8m0[k / 32, n] - 127)
//
// A [M, lda] bf16, 1 <= M <= 16; the weight is an OCP MX image: one 4-bit e2m1 code per element
// and one power-of-two scale (an e8m0 byte) per 32 consecutive k of one output column.  The
// weight bytes are the traffic (4.25 bits per element): they are streamed from HBM once with
// 16-byte loads, whatever M is.
//
// Arithmetic.  v_cvt_scalef32_pk_bf16_fp4 turns two codes and the group's scale into two bf16
// values, exactly (3 significant bits, exponents inside bf16's normal range), so the scale costs
// nothing and there is no per-column scale step.  The bf16 values are the B operand of
// v_mfma_f32_16x16x32_bf16; the M rows of A, padded to 16 with zeros made in registers, are the
// A operand; accumulation is fp32 inside the MFMA; bias and activation in fp32; one rounding.
// The per-element cost is half a conversion and 1/512 of an MFMA, whatever M is -- unlike the
// bf16 and e4m3 siblings, whose FMAs per element grow with M.
//
// Weight image (ops/skinny_mxfp4.py packs it): [N / 16 strips][K / 32 groups][16 columns][16
// bytes].  The 16 bytes hold the 32 codes of one scale group -- k = 32 g .. 32 g + 31 of column
// 16 ct + c --, byte b with k + 2 b in its low nibble and k + 2 b + 1 in its high one.  Four
// consecutive groups of a strip are a tile of 16 columns x 128 k, 1 KiB, one wave load: lane
// l = kb * 16 + c owns bytes 16 l .. 16 l + 15 of it, so one global_load_dwordx4 per lane feeds
// four MFMAs and needs one scale byte, and the tiles of a strip are contiguous in ascending k.
// MFMA j of a step takes the lane's dword j, i.e. k = kb * 32 + 8 j .. + 7, as the eight B
// values of MFMA k-slot kb; the A fragment is read in the same permuted order, lane (r, kb)
// taking x[r, kb * 32 + 8 j .. + 7].  The image is not padded: the groups of the last tile that
// lie at or beyond K / 32 are not loaded and count as zeros.
//
// Geometry.  256 threads; wave w of workgroup (bx, s) owns the 16-column strip 4 bx + w and the
// workgroup owns K slice s (a multiple of 128 k).  The rows of A for the slice are staged in
// LDS in chunks of 1024 k (row stride padded by 16 bytes, so the 16 rows of a ds_read_b128 fall
// into different banks) and shared by the four waves.  A wave keeps kAhead = 4 steps of weight
// (4 KiB) and their scale bytes in flight under the conversions and MFMAs of the current step.
// The four MFMAs of a step accumulate into four accumulators (no dependent MFMA chain); they are
// added in a fixed order at the end.
//
// Split-K, determinism, batch invariance: the siblings' scheme.  With more than one slice the
// workgroup stores its raw fp32 partial [M, N] with plain stores, a second kernel adds the
// partials in split order, applies the epilogue and rounds once.  No atomics, flags or spins.
// One instantiation runs for every M and the order of the K terms of an output element depends
// on (N, K, num_splits) only: row i of an M-row call equals the 1-row call bit for bit.
//
// Epilogues: 0 none, 1 + bias[N], 2 gelu_tanh(. + bias), 3 SwiGLU over gate|up interleaved in
// 16-column blocks (output [M, N/2]).
//
// All offsets are 64-bit (operands up to 4 GiB); nothing outside the operands is read or
// written: rows of A from M on, k from K on and columns from N on are never loaded.
//
// pa_mxfp4w_dequant: out[K, N] bf16 = the dequantised image (exact), one wave per tile,
// transposed through LDS so that the stores are 16 bytes wide.
#include "common.h"

using namespace pa;

namespace skinny_mx4 {

constexpr int kThreads = 256;
constexpr int kWaves = 4;
constexpr int kMaxSplits = 1024;
constexpr int kStepK = 128;    // k per tile = per wave step
constexpr int kChunkK = 1024;  // k of A staged in LDS at a time
constexpr int kRowPad = 8;     // bf16 elements of padding per LDS row of A
constexpr int kAhead = 4;      // weight steps in flight per wave
constexpr int kTileBytes = 1024;
constexpr unsigned long kLimit = 0xFFFFFF00ul;  // bytes per operand, as pa_gemm_skinny_ok

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
  int KT;          // 128-k tiles over K (the last one may be partial)
  int splits, kts;  // kts: tiles per slice
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
__device__ __forceinline__ float epi_col(const Params& p, float v, int n) {
  if (p.epi >= 1) v = v + bias_at(p, n);
  if (p.epi == 2) v = gelu_tanh(v);
  return v;
}
__device__ __forceinline__ float swiglu_val(float g, float u) {
  return g / (1.f + __expf(-g)) * u;
}

// 2^(e - 127) of an e8m0 byte; the quantiser's bytes are 27 .. 227, any byte 1 .. 254 is a
// normal float
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
__global__ __launch_bounds__(kThreads, 2) void mx4_kernel(Params p) {
  constexpr int ROW = kChunkK + kRowPad;   // LDS row stride of A, bf16 elements
  constexpr int SPC = kChunkK / kStepK;    // steps per chunk of A
  __shared__ __attribute__((aligned(16))) u16 sA[16 * ROW];
  __shared__ __attribute__((aligned(16))) float sC[16 * 64];  // the workgroup's [16 rows][64 columns]

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = lane & 15, kb = lane >> 4;  // B: column and k-slot; A: row r = c and k-slot
  const int strip = blockIdx.x * kWaves + wave;
  const bool strip_ok = strip * 16 < p.N;
  const int col = strip * 16 + c;
  const int split = blockIdx.y;
  const int kt0 = split * p.kts;
  int kt1 = kt0 + p.kts;
  if (kt1 > p.KT) kt1 = p.KT;
  const int nsteps = kt1 > kt0 ? kt1 - kt0 : 0;  // the same for the four waves
  const int groups = p.K / 32;

  const u32x4 zero4 = {0u, 0u, 0u, 0u};
  const u16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  const u8* bstrip = p.b + (long)strip * p.K * 8 + lane * 16;  // a strip is K / 32 groups of 256 bytes
  const u8* scol = p.scale + col;

  // the weight of step t (tile kt0 + t) and its scale byte; a step past the slice, a strip past
  // N and a group past K (the last tile may be partial) are not read: zero codes
  auto fetch = [&](int t, u32x4& w, uint32_t& e) {
    const int kt = kt0 + t;
    const int g = kt * 4 + kb;
    const bool v = strip_ok && t < nsteps && g < groups;
    w = v ? *reinterpret_cast<const u32x4*>(bstrip + (long)kt * kTileBytes) : zero4;
    e = v ? (uint32_t)scol[(long)g * p.N] : 127u;
  };

  u32x4 wq[kAhead];
  uint32_t eq[kAhead];
#pragma unroll
  for (int i = 0; i < kAhead; ++i) fetch(i, wq[i], eq[i]);

  f32x4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};

#pragma unroll 1
  for (int t0 = 0; t0 < nsteps; t0 += kAhead) {
#pragma unroll
    for (int i = 0; i < kAhead; ++i) {
      const int t = t0 + i;  // uniform over the workgroup
      if (t < nsteps) {
        if (t % SPC == 0) {  // next chunk of A -> LDS; k >= K are zeros, rows >= M are not staged
          __syncthreads();
          const long a0 = (long)(kt0 + t) * kStepK;
          for (int it = tid; it < p.M * (kChunkK / 8); it += kThreads) {
            const int m = it / (kChunkK / 8), k8 = it % (kChunkK / 8);
            const long k = a0 + k8 * 8;
            u16x8 v = zero8;
            if (k < p.K) v = *reinterpret_cast<const u16x8*>(p.a + (long)m * p.lda + k);
            *reinterpret_cast<u16x8*>(sA + m * ROW + k8 * 8) = v;
          }
          __syncthreads();
        }
        const u32x4 w = wq[i];
        const float sc = e8m0_to_f32(eq[i]);
        fetch(t + kAhead, wq[i], eq[i]);  // in flight while w is consumed
        const u16* sa = sA + c * ROW + (t % SPC) * kStepK + kb * 32;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          u16x8 av = zero8;  // rows M .. 15 of A: zeros made here
          if (c < p.M) av = *reinterpret_cast<const u16x8*>(sa + j * 8);
          acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, av), cvt8(w[j], sc), acc[j],
                                                           0, 0, 0);
        }
      }
    }
  }

  // lane (c, kb) holds rows 4 kb .. 4 kb + 3 of column c of the wave's strip
  const f32x4 sum = (acc[0] + acc[1]) + (acc[2] + acc[3]);
#pragma unroll
  for (int i = 0; i < 4; ++i) sC[(kb * 4 + i) * 64 + wave * 16 + c] = sum[i];
  __syncthreads();

  const int n0 = blockIdx.x * 64;
  if (!DIRECT) {
    for (int it = tid; it < p.M * 8; it += kThreads) {
      const int m = it / 8, c0 = (it % 8) * 8;
      const int n = n0 + c0;
      if (n >= p.N) continue;
      float o[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = sC[m * 64 + c0 + j];
      store8(p.ws + ((long)split * p.M + m) * p.N + n, o);
    }
  } else if (p.epi == 3) {
    // 8 outputs per item: block b of 32 columns holds gate 0..15 | up 16..31
    for (int it = tid; it < p.M * 4; it += kThreads) {
      const int m = it / 4, og = it % 4;
      const int gc = (og >> 1) * 32 + (og & 1) * 8;  // gate columns inside the workgroup's 64
      if (n0 + gc >= p.N) continue;
      float o[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = swiglu_val(sC[m * 64 + gc + j], sC[m * 64 + gc + 16 + j]);
      store8(p.c + (long)m * p.ldc + blockIdx.x * 32 + og * 8, o);
    }
  } else {
    for (int it = tid; it < p.M * 8; it += kThreads) {
      const int m = it / 8, c0 = (it % 8) * 8;
      const int n = n0 + c0;
      if (n >= p.N) continue;
      float o[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = epi_col(p, sC[m * 64 + c0 + j], n + j);
      store8(p.c + (long)m * p.ldc + n, o);
    }
  }
}

// ------------------------------------------------------------------ split-K sum + epilogue
// one thread per output element: partials added in split order, epilogue in fp32, one rounding
__global__ __launch_bounds__(256) void mx4_sum_kernel(Params p) {
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

// ------------------------------------------------------------------ dequantiser
// one wave per tile: the GEMM's load and conversion, [128 k][16 columns] bf16 through LDS, then
// two 16-byte stores per k row; groups from K / 32 on are not read, rows from K on not written
__global__ __launch_bounds__(kThreads) void dequant_kernel(const u8* b, const u8* scale, u16* out, long K, long N,
                                                           long ldo, int KT) {
  __shared__ __attribute__((aligned(16))) u16 sT[kWaves][kStepK * 16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = lane & 15, kb = lane >> 4;
  const long tiles = (N / 16) * KT, groups = K / 32;
  for (long base = (long)blockIdx.x * kWaves; base < tiles; base += (long)gridDim.x * kWaves) {
    const long tile = base + wave;
    const bool ok = tile < tiles;
    const long ct = tile / KT, kt = tile % KT;
    const long g = kt * 4 + kb;
    if (ok && g < groups) {
      const u32x4 w = *reinterpret_cast<const u32x4*>(b + ct * K * 8 + kt * kTileBytes + lane * 16);
      const float sc = e8m0_to_f32((uint32_t)scale[g * N + ct * 16 + c]);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const u16x8 v = __builtin_bit_cast(u16x8, cvt8(w[j], sc));
#pragma unroll
        for (int i = 0; i < 8; ++i) sT[wave][(kb * 32 + j * 8 + i) * 16 + c] = v[i];
      }
    }
    __syncthreads();
    if (ok) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int row = q * 32 + (lane >> 1), half = lane & 1;
        const long k = kt * kStepK + row;
        if (k < K)
          *reinterpret_cast<u16x8*>(out + k * ldo + ct * 16 + half * 8) =
              *reinterpret_cast<const u16x8*>(&sT[wave][row * 16 + half * 8]);
      }
    }
    __syncthreads();
  }
}

}  // namespace skinny_mx4

// Whether pa_gemm_skinny_mxfp4 takes this problem.  Sizes, strides (lda, ldc in bf16 elements)
// and addresses only: nothing is dereferenced.  The image is the packed one of a [K, N] weight.
PA_EXPORT int pa_gemm_skinny_mxfp4_ok(int M, int N, int K, long lda, long ldc, int epi, int num_splits,
                                      const void* a, const void* b, const void* c, const void* bias,
                                      const void* scale) {
  using skinny_mx4::kLimit;
  if (M < 1 || M > 16 || N < 16 || N % 16 || K < 32 || K % 32) return 0;
  if (epi < 0 || epi > 3 || num_splits < 1 || num_splits > skinny_mx4::kMaxSplits) return 0;
  if ((epi == 1 || epi == 2) && bias == nullptr) return 0;
  if (epi == 3 && N % 32) return 0;
  const int nout = epi == 3 ? N / 2 : N;
  if (a == nullptr || b == nullptr || c == nullptr || scale == nullptr) return 0;
  if (((uintptr_t)a & 15) || ((uintptr_t)b & 15) || ((uintptr_t)c & 15)) return 0;
  if (lda < K || lda % 8 || ldc < nout || ldc % 8) return 0;
  if ((unsigned long)M * (unsigned long)lda * 2 >= kLimit || (unsigned long)M * (unsigned long)ldc * 2 >= kLimit ||
      (unsigned long)K * 8ul * (unsigned long)(N / 16) >= kLimit)
    return 0;
  if (bias != nullptr && ((uintptr_t)bias & 3)) return 0;
  return 1;
}

// Split count from N and K alone (never from M: the summation order of an output element must
// not depend on the batch): the largest power of two that keeps workgroups (64 columns each)
// times splits at or below 1024 -- four resident workgroups on each of 256 compute units; a
// workgroup holds 33 KiB of LDS and few registers --, with slices of at least 512 k, at most 64.
PA_EXPORT int pa_gemm_skinny_mxfp4_splits(int N, int K) {
  if (N < 1 || K < 32) return 1;
  const long wgs = ((long)N + 63) / 64;
  long want = 1;
  while (want * 2 * wgs <= 1024) want *= 2;
  while (want > 1 && want > K / 512) want /= 2;
  if (want > 64) want = 64;
  return want < 1 ? 1 : (int)want;
}

// fp32 workspace elements pa_gemm_skinny_mxfp4 needs (none for a single slice)
PA_EXPORT int pa_gemm_skinny_mxfp4_ws_floats(int M, int N, int splits) {
  return splits > 1 ? splits * M * N : 0;
}

// C [M, ldc] bf16 = epilogue(A [M, lda] . dq [K, N]).  ws: pa_gemm_skinny_mxfp4_ws_floats(M, N,
// num_splits) floats.  A refused problem returns hipErrorInvalidValue and launches nothing.  No
// host synchronisation, no host read of device memory: capturable into a HIP graph.
PA_EXPORT int pa_gemm_skinny_mxfp4(const void* a, const void* b, const void* scale, void* c, const void* bias,
                                   int bias_f32, float* ws, int M, int N, int K, long lda, long ldc, int epi,
                                   int num_splits, hipStream_t st) {
  if (!pa_gemm_skinny_mxfp4_ok(M, N, K, lda, ldc, epi, num_splits, a, b, c, bias, scale))
    return (int)hipErrorInvalidValue;
  if (num_splits > 1 && (ws == nullptr || (long)num_splits * M * N > 0x7FFFFFFFl)) return (int)hipErrorInvalidValue;
  skinny_mx4::Params p;
  p.a = (const u16*)a; p.b = (const skinny_mx4::u8*)b; p.scale = (const skinny_mx4::u8*)scale;
  p.c = (u16*)c; p.ws = num_splits > 1 ? ws : nullptr; p.bias = bias;
  p.lda = lda; p.ldc = ldc;
  p.M = M; p.N = N; p.K = K;
  p.KT = (K + 127) / 128;
  p.splits = num_splits;
  p.kts = (p.KT + num_splits - 1) / num_splits;
  p.epi = epi; p.bias_f32 = bias_f32;
  const dim3 grid((N + 63) / 64, num_splits);
  if (num_splits == 1) {
    hipLaunchKernelGGL(skinny_mx4::mx4_kernel<true>, grid, dim3(skinny_mx4::kThreads), 0, st, p);
  } else {
    hipLaunchKernelGGL(skinny_mx4::mx4_kernel<false>, grid, dim3(skinny_mx4::kThreads), 0, st, p);
    const long outs = (long)M * (epi == 3 ? N / 2 : N);
    hipLaunchKernelGGL(skinny_mx4::mx4_sum_kernel, dim3((unsigned)((outs + 255) / 256)), dim3(256), 0, st, p);
  }
  PA_LAUNCH_CHECK();
}

// out [K, ldo] bf16 = the dequantised [K, N] image.  K % 32 == 0, N % 16 == 0, 16-byte aligned
// rows of out.
PA_EXPORT int pa_mxfp4w_dequant(const void* b, const void* scale, void* out, long K, long N, long ldo,
                                hipStream_t st) {
  if (K < 32 || K % 32 || N < 16 || N % 16 || ldo < N || ldo % 8 || b == nullptr || scale == nullptr ||
      out == nullptr || ((uintptr_t)b & 15) || ((uintptr_t)out & 15) || K > 0x3FFFFFFFl)
    return (int)hipErrorInvalidValue;
  const int KT = (int)((K + 127) / 128);
  const long tiles = (N / 16) * KT;
  hipLaunchKernelGGL(skinny_mx4::dequant_kernel, dim3(stream_grid(tiles, skinny_mx4::kWaves)),
                     dim3(skinny_mx4::kThreads), 0, st, (const skinny_mx4::u8*)b, (const skinny_mx4::u8*)scale,
                     (u16*)out, K, N, ldo, KT);
  PA_LAUNCH_CHECK();
}
