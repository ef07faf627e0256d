// Memory-bound fused elementwise kernels for gfx950: rotary embedding, SwiGLU,
// embedding gather/scatter-add, and cast.  All of them move 16 B per lane per
// access (guide Guideline 13) and use grid-stride loops capped at 2048 blocks.
//
// Parity: the reference has no rotary/SwiGLU (north-star ops); embedding
// follows lookup_table (paddle/fluid/operators/lookup_table_op.cu:89-166,
// dense grad by atomics) re-derived for wave64 with 16-byte row vectors.
#include "common.h"

namespace pa {

// ---------------------------------------------------------------- rotary
// x: [B*S tokens, nh_total heads, D] with token stride x_ts (elements), head stride D;
// heads [0, n_rot) are rotated, heads [n_rot, nh_total) are copied unchanged (used
// to repack [q|k|v] -> rotated [q|k] + v in one pass).  y may alias x (in place).
// neox / rotate-half convention: pairs (i, i + D/2).  cos/sin tables: [S, D/2] fp32.
// pos: optional int64 [B*S] position ids (null => position = s).
// sign = +1 forward, -1 backward (rotation by -theta).  TI/TO allow fp32 -> bf16
// (fused dq-accumulator cast + inverse rotation in the attention backward).
template <typename TI, typename TO>
__global__ void rope_kernel(const TI* x, long x_ts, TO* y, long y_ts,
                            const float* __restrict__ cosT, const float* __restrict__ sinT,
                            const long* __restrict__ pos, long B, long S, int nh, int n_rot,
                            int D, float sign) {
  const int half = D / 2;
  const int cpp = half / 8;  // 8-wide chunks per head half
  const long total = B * S * nh * cpp;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i % cpp);
    long t = i / cpp;
    const int h = (int)(t % nh);
    t /= nh;  // token index b*S + s
    const TI* xb = x + t * x_ts + (long)h * D + c * 8;
    TO* yb = y + t * y_ts + (long)h * D + c * 8;
    float a[8], b[8];
    load8(xb, a);
    load8(xb + half, b);
    if (h < n_rot) {
      const long s = t % S;
      const long p = pos ? pos[t] : s;
      float co[8], si[8];
      load8(cosT + p * half + c * 8, co);
      load8(sinT + p * half + c * 8, si);
      float oa[8], ob[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float sn = sign * si[j];
        oa[j] = a[j] * co[j] - b[j] * sn;
        ob[j] = b[j] * co[j] + a[j] * sn;
      }
      store8(yb, oa);
      store8(yb + half, ob);
    } else {
      store8(yb, a);
      store8(yb + half, b);
    }
  }
}

// ---------------------------------------------------------------- SwiGLU
// gu: [N, 2I] = [gate | up]; out: [N, I] = silu(gate) * up
template <typename T>
__global__ void swiglu_fwd_kernel(const T* __restrict__ gu, T* __restrict__ out, long N, int I) {
  const int cpr = I / 8;
  const long total = N * cpr;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    const long r = i / cpr;
    const int c = (int)(i % cpr) * 8;
    float g[8], u[8], o[8];
    load8(gu + r * 2 * I + c, g);
    load8(gu + r * 2 * I + I + c, u);
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = g[j] / (1.f + __expf(-g[j])) * u[j];
    store8(out + r * I + c, o);
  }
}

template <typename T>
__global__ void swiglu_bwd_kernel(const T* __restrict__ gu, const T* __restrict__ dout,
                                  T* __restrict__ dgu, long N, int I) {
  const int cpr = I / 8;
  const long total = N * cpr;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    const long r = i / cpr;
    const int c = (int)(i % cpr) * 8;
    float g[8], u[8], d[8], dg[8], du[8];
    load8(gu + r * 2 * I + c, g);
    load8(gu + r * 2 * I + I + c, u);
    load8(dout + r * I + c, d);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float sg = 1.f / (1.f + __expf(-g[j]));
      const float silu = g[j] * sg;
      du[j] = d[j] * silu;
      dg[j] = d[j] * u[j] * sg * (1.f + g[j] * (1.f - sg));
    }
    store8(dgu + r * 2 * I + c, dg);
    store8(dgu + r * 2 * I + I + c, du);
  }
}

// ---------------------------------------------------------------- embedding
template <typename T>
__global__ void embedding_fwd_kernel(const long* __restrict__ ids, const T* __restrict__ W,
                                     T* __restrict__ out, long N, int H, long padding_idx) {
  const int cpr = H / 8;
  const long total = N * cpr;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (long)gridDim.x * blockDim.x) {
    const long r = i / cpr;
    const int c = (int)(i % cpr) * 8;
    const long id = ids[r];
    float v[8];
    if (id == padding_idx) {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = 0.f;
    } else {
      load8(W + id * H + c, v);
    }
    store8(out + r * H + c, v);
  }
}

// dW (fp32 accumulator) += scatter(dout) over the token rows [r0, r1), without float
// atomics: the same bits every run.  One 16-wave block per token row.  The block of the
// FIRST row of the range that carries an id owns that id: it sums the range's rows with
// this id in ascending row order in registers, its waves sharing the columns, and adds the
// sum to dW with a plain read-modify-write (no other block of the launch touches that dW
// row); the blocks of later duplicates leave.  Each lane adds 4 contiguous floats (VEC:
// one 8- / 16-B access; needs H % 4 == 0 and 16-B aligned pointers).  The id scans are
// wave-wide 512-B loads of a cache-resident array, (r1 - r0)^2 / 64 of them per launch: the
// launcher walks long inputs in ranges of EMB_BWD_ROWS rows (launches of one stream run in
// order, which keeps the summation order fixed across ranges too).
// Measured against the float-atomic kernel it replaces (16384 rows, H 4096, bf16 dout,
// 32000 ids, MI355X): uniform ids 377 vs 844 us, Zipf(1) ids (most frequent id on 1490
// rows) 584 vs 1128 us; the serial sum of one dominant id costs more: 30 % of the rows on
// one id 2.38 vs 1.45 ms, all rows on one id 5.77 vs 2.75 ms.
constexpr long EMB_BWD_ROWS = 8192;
constexpr int EMB_BWD_WAVES = 16;
constexpr int EMB_BWD_U = 16;

__device__ __forceinline__ void ld4(const u16* p, float* v) {
  const u16x4 t = *reinterpret_cast<const u16x4*>(p);
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = bf2f(t[j]);
}
__device__ __forceinline__ void ld4(const float* p, float* v) {
  const f32x4 t = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = t[j];
}

template <typename T, bool VEC>
__global__ __launch_bounds__(64 * EMB_BWD_WAVES) void embedding_bwd_kernel(const long* __restrict__ ids, const T* __restrict__ dout,
                                     float* __restrict__ dW, long r0, long r1, int H, long padding_idx) {
  __shared__ unsigned long long match[EMB_BWD_ROWS / 64];  // bit i of word c: row r + 64c + i has this id
  __shared__ int off[EMB_BWD_ROWS / 64 + 1];               // matches before chunk c
  __shared__ u16 rows[EMB_BWD_ROWS];                       // the matching rows (minus r), ascending
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long r = r0 + blockIdx.x;  // r, id: block-uniform
  const long id = ids[r];
  if (id == padding_idx) return;
  // an earlier row of the range with this id?  64-row chunks of [r0, r), round-robin over the waves
  bool hit = false;
  for (long b = r0 + 64 * w; b < r; b += 64 * EMB_BWD_WAVES) {
    const long q = b + lane;
    hit |= q < r && ids[q] == id;
  }
  if (__syncthreads_or(hit)) return;
  // the rows of [r, r1) with this id, found once by the whole block and compacted in order
  const int nch = (int)((r1 - r + 63) / 64);
  for (int c = w; c < nch; c += EMB_BWD_WAVES) {
    const long q = r + 64L * c + lane;
    const unsigned long long m = __ballot(q < r1 && ids[q] == id);
    if (lane == 0) match[c] = m;
  }
  __syncthreads();
  for (int c = threadIdx.x; c <= nch; c += blockDim.x) {
    int n = 0;
    for (int i = 0; i < c; ++i) n += __popcll(match[i]);
    off[c] = n;
  }
  __syncthreads();
  for (int c = w; c < nch; c += EMB_BWD_WAVES) {
    const unsigned long long m = match[c];
    if ((m >> lane) & 1) rows[off[c] + __popcll(m & ((1ULL << lane) - 1))] = (u16)(64 * c + lane);
  }
  __syncthreads();
  const int nrows = off[nch];
  float* dst = dW + id * H;
  // a pass covers EMB_BWD_WAVES x 256 = 4096 columns, wave w the w-th 256 of them.  The
  // loads of EMB_BWD_U rows are issued before they are added (in row order), so a
  // frequent id costs one memory latency per EMB_BWD_U rows; dW is read and written once.
  for (int c0 = 0; c0 < H; c0 += 256 * EMB_BWD_WAVES) {
    const int col = c0 + w * 256 + lane * 4;
    if (col >= H) continue;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int g = 0; g < nrows; g += EMB_BWD_U) {
      float v[EMB_BWD_U][4];
#pragma unroll
      for (int u = 0; u < EMB_BWD_U; ++u) {
        const bool on = g + u < nrows;
        const T* src = dout + (r + rows[on ? g + u : 0]) * H + col;
        if (VEC) {
          if (on) ld4(src, v[u]);
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) v[u][j] = (on && col + j < H) ? IO<T>::ld(src, j) : 0.f;
        }
        if (VEC && !on)
#pragma unroll
          for (int j = 0; j < 4; ++j) v[u][j] = 0.f;
      }
#pragma unroll
      for (int u = 0; u < EMB_BWD_U; ++u)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] += v[u][j];
    }
    if (VEC) {
      f32x4 t = *reinterpret_cast<f32x4*>(dst + col);
#pragma unroll
      for (int j = 0; j < 4; ++j) t[j] += acc[j];
      *reinterpret_cast<f32x4*>(dst + col) = t;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (col + j < H) dst[col + j] += acc[j];
    }
  }
}

template <typename TI, typename TO>
__global__ void cast_kernel(const TI* __restrict__ in, TO* __restrict__ out, long n) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (long)gridDim.x * blockDim.x)
    IO<TO>::st(out, i, IO<TI>::ld(in, i));
}

}  // namespace pa

using namespace pa;

// in/out dtype: 0 fp32, 1 bf16
PA_EXPORT int pa_rope(int in_dtype, int out_dtype, const void* x, long x_ts, void* y, long y_ts,
                      const float* cosT, const float* sinT, const long* pos, long B, long S,
                      int nh, int n_rot, int D, int backward, hipStream_t st) {
  if (D % 16) return (int)hipErrorInvalidValue;
  const long work = B * S * nh * (D / 16);
  const int g = stream_grid(work, 256);
  const float sign = backward ? -1.f : 1.f;
#define PA_R(TI, TO) \
  hipLaunchKernelGGL((rope_kernel<TI, TO>), dim3(g), dim3(256), 0, st, (const TI*)x, x_ts, (TO*)y, y_ts, cosT, sinT, pos, B, S, nh, n_rot, D, sign)
  if (in_dtype == 1 && out_dtype == 1) PA_R(u16, u16);
  else if (in_dtype == 0 && out_dtype == 1) PA_R(float, u16);
  else if (in_dtype == 0 && out_dtype == 0) PA_R(float, float);
  else PA_R(u16, float);
#undef PA_R
  PA_LAUNCH_CHECK();
}

PA_EXPORT int pa_swiglu_fwd(int dtype, const void* gu, void* out, long N, int I, hipStream_t st) {
  if (I % 8) return (int)hipErrorInvalidValue;
  const int g = stream_grid(N * (I / 8), 256);
  if (dtype == 1)
    hipLaunchKernelGGL(swiglu_fwd_kernel<u16>, dim3(g), dim3(256), 0, st, (const u16*)gu, (u16*)out, N, I);
  else
    hipLaunchKernelGGL(swiglu_fwd_kernel<float>, dim3(g), dim3(256), 0, st, (const float*)gu, (float*)out, N, I);
  PA_LAUNCH_CHECK();
}

PA_EXPORT int pa_swiglu_bwd(int dtype, const void* gu, const void* dout, void* dgu, long N, int I,
                            hipStream_t st) {
  if (I % 8) return (int)hipErrorInvalidValue;
  const int g = stream_grid(N * (I / 8), 256);
  if (dtype == 1)
    hipLaunchKernelGGL(swiglu_bwd_kernel<u16>, dim3(g), dim3(256), 0, st, (const u16*)gu, (const u16*)dout, (u16*)dgu, N, I);
  else
    hipLaunchKernelGGL(swiglu_bwd_kernel<float>, dim3(g), dim3(256), 0, st, (const float*)gu, (const float*)dout, (float*)dgu, N, I);
  PA_LAUNCH_CHECK();
}

PA_EXPORT int pa_embedding_fwd(int dtype, const long* ids, const void* W, void* out, long N, int H,
                               long padding_idx, hipStream_t st) {
  if (H % 8) return (int)hipErrorInvalidValue;
  const int g = stream_grid(N * (H / 8), 256);
  if (dtype == 1)
    hipLaunchKernelGGL(embedding_fwd_kernel<u16>, dim3(g), dim3(256), 0, st, ids, (const u16*)W, (u16*)out, N, H, padding_idx);
  else
    hipLaunchKernelGGL(embedding_fwd_kernel<float>, dim3(g), dim3(256), 0, st, ids, (const float*)W, (float*)out, N, H, padding_idx);
  PA_LAUNCH_CHECK();
}

PA_EXPORT int pa_embedding_bwd(int dtype, const long* ids, const void* dout, float* dW, long N,
                               int H, long padding_idx, hipStream_t st) {
  const bool vec = H % 4 == 0 && ((uintptr_t)dout | (uintptr_t)dW) % 16 == 0;
  for (long r0 = 0; r0 < N; r0 += EMB_BWD_ROWS) {
    const long r1 = r0 + EMB_BWD_ROWS < N ? r0 + EMB_BWD_ROWS : N;
    const dim3 g(r1 - r0), b(64 * EMB_BWD_WAVES);  // one block per row
#define PA_EB(T, VEC_) \
  hipLaunchKernelGGL((embedding_bwd_kernel<T, VEC_>), g, b, 0, st, ids, (const T*)dout, dW, r0, r1, H, padding_idx)
    if (dtype == 1) { if (vec) PA_EB(u16, true); else PA_EB(u16, false); }
    else { if (vec) PA_EB(float, true); else PA_EB(float, false); }
#undef PA_EB
  }
  PA_LAUNCH_CHECK();
}

// in_dtype/out_dtype: 0 fp32, 1 bf16
PA_EXPORT int pa_cast(int in_dtype, int out_dtype, const void* in, void* out, long n, hipStream_t st) {
  const int g = stream_grid(n, 256);
  if (in_dtype == 0 && out_dtype == 1)
    hipLaunchKernelGGL((cast_kernel<float, u16>), dim3(g), dim3(256), 0, st, (const float*)in, (u16*)out, n);
  else if (in_dtype == 1 && out_dtype == 0)
    hipLaunchKernelGGL((cast_kernel<u16, float>), dim3(g), dim3(256), 0, st, (const u16*)in, (float*)out, n);
  else
    return (int)hipErrorInvalidValue;
  PA_LAUNCH_CHECK();
}
