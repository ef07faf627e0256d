// Token selection for generation: logits [B, V] -> the next token per row, plus the
// EOS / done / lengths bookkeeping of generate(), in one launch.  The contract (what is
// kept, what is drawn, what a degenerate row gives) is written down and implemented in
// float64 in ops/sampling.py; this file is its gfx950 kernel.
//
// One workgroup of 1024 threads per row.  The row is read from global memory in every
// pass (16-byte loads; after the first pass it comes from L2):
//   pass 0     maximum and its lowest index                    (greedy ends here)
//   top-k      radix select over order-preserving integer keys of the logits, 8 bits a
//              pass, weight 1 per token:   keep key >= t, t the smallest key value with
//              fewer than k tokens strictly above it
//   top-p      the same select, weight exp((x - max) / T) per token, limit top_p * total
//   draw       each thread sums the survivors of one contiguous index range, one block
//              scan in thread (= index) order, the owner of u * total walks its range
// Histogram weights are integers (counts, or masses in 2^-40 fixed point) added with
// integer LDS atomics, the float sums have a fixed order, so a row's token depends on its
// own logits, (seed, step, row) and nothing else, and is bit-identical from run to run.
// Rows may start at any element-aligned address: vectors are cut at 16-byte boundaries of
// the address, the ragged head and tail are read element by element.
// The keys, the row walk, the radix select and Philox are in sample_common.h (shared with
// spec_verify.hip).
#include "sample_common.h"

namespace pa {
namespace smp {

__device__ __forceinline__ float philox_u(u64 seed, int step, int row) {
  return (float)(philox_x0(seed, (uint32_t)step, (uint32_t)row) >> 8) * 5.9604644775390625e-8f;  // 2^-24
}

__global__ void philox_kernel(u64 seed, const int* step_ptr, int step, float* u, int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) u[b] = philox_u(seed, step_ptr ? *step_ptr : step, b);
}

struct Args {
  const void* logits;
  long ld;
  int B, V;
  u64 seed;
  const int* step_ptr;
  int step;
  int do_sample;
  float inv_t;
  int top_k;
  float top_p;
  long long* tok;       // [B]
  // bookkeeping (null out: none)
  long long* out;       // [B, max_new]
  int max_new;
  long long* lengths;   // [B]
  unsigned char* done;  // [B]
  long long eos;        // < 0: none
  long long pad;
};

template <typename T>
__global__ __launch_bounds__(kThreads) void sample_kernel(Args a) {
  __shared__ Shared s;
  constexpr int E = Key<T>::kVec;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int V = a.V;
  const T* row = reinterpret_cast<const T*>(a.logits) + (long)b * a.ld;
  const int off = (int)((reinterpret_cast<uintptr_t>(row) & 15u) / sizeof(T));
  const int nvec = (V + off + E - 1) / E;
  const int step = a.step_ptr ? *a.step_ptr : a.step;

  // ---- pass 0: the maximum and its lowest index, packed so that one max finds both
  u64 best = 0;
  for (int jv = tid; jv < nvec; jv += kThreads) {
    visit_vec<T>(row, off, V, jv, [&](int i, uint32_t k) {
      const u64 c = ((u64)k << 32) | (uint32_t)(0x7fffffff - i);
      best = c > best ? c : best;
    });
  }
  best = wave_max_u64(best);
  if (lane == 0) s.wred[wave] = best;
  __syncthreads();
  best = s.wred[0];
#pragma unroll
  for (int w = 1; w < kWaves; ++w) best = s.wred[w] > best ? s.wred[w] : best;
  const uint32_t kmax = (uint32_t)(best >> 32);
  const int greedy = 0x7fffffff - (int)(uint32_t)best;
  const float xmax = Key<T>::value(kmax);
  int token = greedy;

  // sampling has something to draw from only when the maximum is finite
  if (a.do_sample && fabsf(xmax) < INFINITY) {  // uniform over the block
    uint32_t thr = 0;
    if (a.top_k > 0 && a.top_k < V)
      thr = radix_select<T, false>(s, row, off, V, nvec, 0u, (u64)a.top_k, 0.f, 0.f, 0.f);
    if (a.top_p < 1.f) {
      const uint32_t tp = radix_select<T, true>(s, row, off, V, nvec, thr, 0, a.top_p, xmax, a.inv_t);
      thr = tp > thr ? tp : thr;
    }
    // ---- draw: thread t owns the vectors [t * per, (t + 1) * per), i.e. a contiguous index range
    const int per = (nvec + kThreads - 1) / kThreads;
    const int jv0 = tid * per, jv1 = min(nvec, jv0 + per);
    float seg = 0.f;
    int last = -1;
    for (int jv = jv0; jv < jv1; ++jv) {
      visit_vec<T>(row, off, V, jv, [&](int i, uint32_t k) {
        if (k < thr) return;
        const float e = expf((Key<T>::value(k) - xmax) * a.inv_t);
        if (e > 0.f) { seg += e; last = i; }
      });
    }
    if (tid == 0) { s.found = kThreads; s.last = -1; s.token = -1; }
    // inclusive scan in thread order: within the wave, then over the wave totals
    float inc = seg;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const float t = __shfl_up(inc, o, 64);
      if (lane >= o) inc += t;
    }
    if (lane == 63) s.fred[wave] = inc;
    __syncthreads();
    float base = 0.f, total = 0.f;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      if (w == wave) base = total;
      total += s.fred[w];
    }
    inc += base;
    const float target = philox_u(a.seed, step, b) * total;
    if (seg > 0.f && target < inc) atomicMin(&s.found, tid);
    if (last >= 0) atomicMax(&s.last, last);
    __syncthreads();
    if (total > 0.f && total < INFINITY) {  // uniform: total comes from LDS
      if (s.found == tid) {
        float run = inc - seg;  // the exclusive sum of this range
        int pick = -1, seen = -1;
        for (int jv = jv0; jv < jv1; ++jv) {
          visit_vec<T>(row, off, V, jv, [&](int i, uint32_t k) {
            if (k < thr || pick >= 0) return;
            const float e = expf((Key<T>::value(k) - xmax) * a.inv_t);
            if (e > 0.f) {
              run += e;
              seen = i;
              if (target < run) pick = i;
            }
          });
        }
        s.token = pick >= 0 ? pick : seen;  // rounding: the range's last survivor
      }
      __syncthreads();
      token = s.found < kThreads ? s.token : s.last;  // target == total: the last survivor
      if (token < 0 || token >= V) token = greedy;
    }
  }

  if (tid == 0) {
    long long nxt = token;
    if (a.out) {
      const bool was_done = a.done[b] != 0;
      if (was_done) nxt = a.pad;
      if (step >= 0 && step < a.max_new) a.out[(long)b * a.max_new + step] = nxt;
      if (a.eos >= 0 && nxt == a.eos && !was_done) {
        a.lengths[b] = (long long)step + 1;
        a.done[b] = 1;
      }
    }
    a.tok[b] = nxt;
  }
}

}  // namespace smp
}  // namespace pa

using namespace pa;

// Whether pa_sample takes these logits (dtype 0 fp32 / 1 bf16, unit column stride implied):
// rows of 1..131072 entries at element-aligned addresses, any row stride.
PA_EXPORT int pa_sample_ok(int dtype, int B, int V, long ld, const void* logits) {
  if (dtype != 0 && dtype != 1) return 0;
  if (B < 1 || V < 1 || V > 131072 || logits == nullptr) return 0;
  if (ld < 0 || (B > 1 && ld != 0 && ld < V)) return 0;
  const size_t sz = dtype ? 2 : 4;
  if (reinterpret_cast<uintptr_t>(logits) % sz) return 0;
  return 1;
}

PA_EXPORT int pa_philox_uniform(unsigned long long seed, const int* step_ptr, int step, float* u, int B,
                                hipStream_t st) {
  if (B < 1 || u == nullptr) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(smp::philox_kernel, dim3((B + 255) / 256), dim3(256), 0, st, seed, step_ptr, step, u, B);
  PA_LAUNCH_CHECK();
}

// tok[b] = the next token of row b.  With `out` the generate() bookkeeping as well: a done
// row emits pad, out[b][step] = tok[b], a first eos sets lengths[b] = step + 1 and done[b].
// step comes from step_ptr (device int32) when given, else from the argument; it is not
// advanced here (the caller launches the increment after this kernel).
PA_EXPORT int pa_sample(int dtype, const void* logits, long ld, int B, int V, unsigned long long seed,
                        const int* step_ptr, int step, int do_sample, float temperature, int top_k, float top_p,
                        long long* tok, long long* out, int max_new, long long* lengths, unsigned char* done,
                        long eos, long pad, hipStream_t st) {
  if (!pa_sample_ok(dtype, B, V, ld, logits) || tok == nullptr) return (int)hipErrorInvalidValue;
  if (out != nullptr && (lengths == nullptr || done == nullptr || max_new < 1)) return (int)hipErrorInvalidValue;
  smp::Args a;
  a.logits = logits; a.ld = ld; a.B = B; a.V = V; a.seed = seed; a.step_ptr = step_ptr; a.step = step;
  a.do_sample = do_sample;
  a.inv_t = 1.f / fmaxf(temperature, 1e-6f);
  a.top_k = top_k; a.top_p = top_p;
  a.tok = tok; a.out = out; a.max_new = max_new; a.lengths = lengths; a.done = done; a.eos = eos; a.pad = pad;
  if (dtype) hipLaunchKernelGGL(smp::sample_kernel<u16>, dim3(B), dim3(smp::kThreads), 0, st, a);
  else hipLaunchKernelGGL(smp::sample_kernel<float>, dim3(B), dim3(smp::kThreads), 0, st, a);
  PA_LAUNCH_CHECK();
}
