// Speculative decoding, the device side of one round: judge G candidate tokens per row
// against the target's logits (and the draft's), then commit what survives into the
// generation state.  The contract (the accept test, the residual draw, the bookkeeping) is
// written down and implemented in float64 in ops/speculative.py; this file is its gfx950
// kernel, on the helpers of sample.hip (sample_common.h).
//
// pa_spec_judge: one workgroup of 1024 threads per (position j, row b); target logits
// [B, G+1, V] and draft logits [B, G, V] with any position / row stride, rows at any
// element-aligned address.  Greedy mode is the maximum pass alone.  Sampled mode filters
// the target row and the draft row as sample.hip filters a row (maximum, radix selects for
// top-k and top-p), sums each row's surviving masses e = exp((x - max) / T) to Z in a fixed
// order, and then, with p = e_p / Z_p and q = e_q / Z_q never formed:
//   accept   u * e_q(d) * Z_p < e_p(d) * Z_q                (u of counter word 2j + 1)
//   alt      drawn from max(e_p * Z_q - e_q * Z_p, 0) by a block scan in index order, or
//            from e_p where that sums to nothing; position G draws from e_p (word 2j + 2)
// Integer LDS atomics only and float sums in a fixed order: a (position, row) depends on its
// own two logit rows, its candidate, (seed, round, row) and nothing else, bit for bit.
//
// pa_spec_commit: one thread per row walks the row's G + 1 decisions and writes out /
// lengths / done / pos / tok / kept / accepted with plain stores.
#include "sample_common.h"

namespace pa {
namespace spec {

using namespace smp;

constexpr int kMaxDraft = 16;

struct JArgs {
  const void* tl;        // target logits [B, G+1, V]
  long t_rs, t_ps;       // its row and position strides, in elements
  const void* dl;        // draft logits [B, G, V] (null: greedy mode only)
  long d_rs, d_ps;
  const long long* cand; // [B, G]
  int B, G, V;
  u64 seed;
  const int* round_ptr;
  int round;
  int do_sample;
  float inv_t;
  int top_k;
  float top_p;
  unsigned char* accept; // [B, G]
  long long* alt;        // [B, G+1]
};

__device__ __forceinline__ float philox_u3(u64 seed, int c0, int row, int c2) {
  return (float)(philox_x0(seed, (uint32_t)c0, (uint32_t)row, (uint32_t)c2) >> 8) * 5.9604644775390625e-8f;
}

// One row of logits as the kernel sees it.
template <typename T> struct Row {
  const T* p;
  int off, nvec;
  uint32_t kmax, thr;  // key of the maximum; survivors have key >= thr
  int greedy;          // lowest index among the maxima
  float xmax;
};

template <typename T>
__device__ __forceinline__ Row<T> make_row(const void* base, long index, int V) {
  constexpr int E = Key<T>::kVec;
  Row<T> r;
  r.p = reinterpret_cast<const T*>(base) + index;
  r.off = (int)((reinterpret_cast<uintptr_t>(r.p) & 15u) / sizeof(T));
  r.nvec = (V + r.off + E - 1) / E;
  r.kmax = r.thr = 0u;
  r.greedy = 0;
  r.xmax = 0.f;
  return r;
}

// The maximum and its lowest index, packed so that one max finds both (sample.hip pass 0).
template <typename T>
__device__ __forceinline__ void row_max(Shared& s, Row<T>& r, int V) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  u64 best = 0;
  for (int jv = tid; jv < r.nvec; jv += kThreads) {
    visit_vec<T>(r.p, r.off, V, jv, [&](int i, uint32_t k) {
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
  __syncthreads();  // wred is free again
  r.kmax = (uint32_t)(best >> 32);
  r.greedy = 0x7fffffff - (int)(uint32_t)best;
  r.xmax = Key<T>::value(r.kmax);
}

// top-k then top-p, as sample.hip: the key threshold of the survivors.
template <typename T>
__device__ __forceinline__ void row_filter(Shared& s, Row<T>& r, int V, const JArgs& a) {
  uint32_t thr = 0;
  if (a.top_k > 0 && a.top_k < V)
    thr = radix_select<T, false>(s, r.p, r.off, V, r.nvec, 0u, (u64)a.top_k, 0.f, 0.f, 0.f);
  if (a.top_p < 1.f) {
    const uint32_t tp = radix_select<T, true>(s, r.p, r.off, V, r.nvec, thr, 0, a.top_p, r.xmax, a.inv_t);
    thr = tp > thr ? tp : thr;
  }
  r.thr = thr;
}

// Mass of a logit of row r given its key: exp((x - max) / T) for a survivor, else 0.
template <typename T>
__device__ __forceinline__ float row_mass(const Row<T>& r, uint32_t k, float inv_t) {
  return k >= r.thr ? expf((Key<T>::value(k) - r.xmax) * inv_t) : 0.f;
}

// Sum of mass(i, key) over the row in a fixed order: thread t sums a contiguous index
// range, the ranges are added in thread order.  Uniform over the block.
template <typename T, typename F>
__device__ __forceinline__ float block_total(Shared& s, const Row<T>& r, int V, F&& mass) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int per = (r.nvec + kThreads - 1) / kThreads;
  const int jv0 = tid * per, jv1 = min(r.nvec, jv0 + per);
  float seg = 0.f;
  for (int jv = jv0; jv < jv1; ++jv)
    visit_vec<T>(r.p, r.off, V, jv, [&](int i, uint32_t k) { seg += mass(i, k); });
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float t = __shfl_up(seg, o, 64);
    if (lane >= o) seg += t;
  }
  if (lane == 63) s.fred[wave] = seg;
  __syncthreads();
  float total = 0.f;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) total += s.fred[w];
  __syncthreads();  // fred is free again
  return total;
}

// Draw from the masses mass(i, key) >= 0 of the row, in index order: the first i whose
// running sum passes u * total (sample.hip's draw).  Returns -1, with `total` set, when the
// masses do not sum to a positive finite number.  Uniform over the block.
template <typename T, typename F>
__device__ __forceinline__ int scan_draw(Shared& s, const Row<T>& r, int V, float u, F&& mass, float& total_out) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int per = (r.nvec + kThreads - 1) / kThreads;
  const int jv0 = tid * per, jv1 = min(r.nvec, jv0 + per);
  float seg = 0.f;
  int last = -1;
  for (int jv = jv0; jv < jv1; ++jv) {
    visit_vec<T>(r.p, r.off, V, jv, [&](int i, uint32_t k) {
      const float e = mass(i, k);
      if (e > 0.f) { seg += e; last = i; }
    });
  }
  if (tid == 0) { s.found = kThreads; s.last = -1; s.token = -1; }
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
  const float target = u * total;
  if (seg > 0.f && target < inc) atomicMin(&s.found, tid);
  if (last >= 0) atomicMax(&s.last, last);
  __syncthreads();
  int token = -1;
  if (total > 0.f && total < INFINITY) {  // uniform: total comes from LDS
    if (s.found == tid) {
      float run = inc - seg;  // the exclusive sum of this range
      int pick = -1, seen = -1;
      for (int jv = jv0; jv < jv1; ++jv) {
        visit_vec<T>(r.p, r.off, V, jv, [&](int i, uint32_t k) {
          if (pick >= 0) return;
          const float e = mass(i, k);
          if (e > 0.f) {
            run += e;
            seen = i;
            if (target < run) pick = i;
          }
        });
      }
      s.token = pick >= 0 ? pick : seen;  // rounding: the range's last index with mass
    }
    __syncthreads();
    token = s.found < kThreads ? s.token : s.last;  // target == total: the last index with mass
  }
  __syncthreads();  // found / last / token / fred are free again
  total_out = total;
  return token;
}

template <typename T>
__global__ __launch_bounds__(kThreads) void judge_kernel(JArgs a) {
  __shared__ Shared s;
  const int j = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int V = a.V, G = a.G;
  const int round = a.round_ptr ? *a.round_ptr : a.round;

  Row<T> P = make_row<T>(a.tl, (long)b * a.t_rs + (long)j * a.t_ps, V);
  row_max<T>(s, P, V);
  const long long d = j < G ? a.cand[(long)b * G + j] : -1;
  const bool d_ok = d >= 0 && d < (long long)V;

  int token = P.greedy;
  bool acc = d == (long long)P.greedy;  // the greedy rule

  // sampling has something to draw from only when the maximum is finite and the masses
  // sum to a positive finite number
  if (a.do_sample && fabsf(P.xmax) < INFINITY) {  // uniform over the block
    row_filter<T>(s, P, V, a);
    const float inv_t = a.inv_t;
    auto ep = [&](int, uint32_t k) { return row_mass<T>(P, k, inv_t); };
    const float u_draw = philox_u3(a.seed, round, b, 2 * j + 2);
    if (j == G) {  // the bonus token: a draw from P
      float zp;
      const int t = scan_draw<T>(s, P, V, u_draw, ep, zp);
      if (t >= 0 && t < V) token = t;
    } else {
      const float zp = block_total<T>(s, P, V, ep);
      if (zp > 0.f && zp < INFINITY) {  // uniform
        Row<T> Q = make_row<T>(a.dl, (long)b * a.d_rs + (long)j * a.d_ps, V);
        row_max<T>(s, Q, V);
        float zq = 1.f;
        bool q_ok = fabsf(Q.xmax) < INFINITY;
        if (q_ok) {  // uniform
          row_filter<T>(s, Q, V, a);
          zq = block_total<T>(s, Q, V, [&](int, uint32_t k) { return row_mass<T>(Q, k, inv_t); });
          q_ok = zq > 0.f && zq < INFINITY;
          if (!q_ok) zq = 1.f;
        }
        // e_q of index i: the draft's mass, or one-hot at its greedy token when the draft
        // has nothing to draw from
        auto eq = [&](int i) {
          return q_ok ? row_mass<T>(Q, Key<T>::key(Q.p[i]), inv_t) : (i == Q.greedy ? 1.f : 0.f);
        };
        acc = false;
        if (d_ok) {
          const float u = philox_u3(a.seed, round, b, 2 * j + 1);
          const float epd = row_mass<T>(P, Key<T>::key(P.p[d]), inv_t);
          acc = u * eq((int)d) * zp < epd * zq;
        }
        float zr;
        int t = scan_draw<T>(s, P, V, u_draw,
                             [&](int i, uint32_t k) { return fmaxf(row_mass<T>(P, k, inv_t) * zq - eq(i) * zp, 0.f); },
                             zr);
        if (t < 0) {  // the residual is empty (q covers p): a draw from P
          float z2;
          t = scan_draw<T>(s, P, V, u_draw, ep, z2);
        }
        if (t >= 0 && t < V) token = t;
      }
    }
  }

  if (tid == 0) {
    a.alt[(long)b * (G + 1) + j] = token;
    if (j < G) a.accept[(long)b * G + j] = acc ? 1 : 0;
  }
}

struct CArgs {
  const unsigned char* accept;  // [B, G]
  const long long* alt;         // [B, G+1]
  const long long* cand;        // [B, G]
  int B, G;
  long long* out;               // [B, max_new]
  int max_new;
  long long* lengths;           // [B]
  unsigned char* done;          // [B]
  int* pos;                     // [B]
  long long* tok;               // [B]
  int* kept;                    // [B]
  int* accepted;                // [B]
  long long eos;                // < 0: none
  long long pad;
};

__global__ void commit_kernel(CArgs c) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= c.B) return;
  const int G = c.G;
  int pos = c.pos[b];
  if (c.done[b] != 0 || pos < 0 || pos >= c.max_new) {  // nothing to emit (no room: done as well)
    c.done[b] = 1;
    c.kept[b] = 0;
    c.tok[b] = c.pad;
    return;
  }
  int a = G;
  for (int j = G - 1; j >= 0; --j)
    if (c.accept[(long)b * G + j] == 0) a = j;
  int emitted = 0;
  long long last = c.pad;
  bool done = false;
  for (int t = 0; t <= a && !done; ++t) {
    last = t < a ? c.cand[(long)b * G + t] : c.alt[(long)b * (G + 1) + a];
    c.out[(long)b * c.max_new + pos] = last;
    ++pos;
    ++emitted;
    if (c.eos >= 0 && last == c.eos) {
      c.lengths[b] = pos;
      done = true;
    } else if (pos >= c.max_new) {
      done = true;
    }
  }
  if (done) c.done[b] = 1;
  c.pos[b] = pos;
  c.tok[b] = last;
  c.kept[b] = emitted;
  c.accepted[b] += a < emitted ? a : emitted;
}

}  // namespace spec
}  // namespace pa

using namespace pa;

// Whether pa_spec_judge takes this problem (dtype 0 fp32 / 1 bf16 for both logit tensors,
// unit column stride implied): 1 <= V <= 131072, 1 <= G <= 16, element-aligned rows, any
// non-negative position and row stride.  Sampled mode needs the draft's logits.
PA_EXPORT int pa_spec_judge_ok(int dtype, int B, int G, int V, const void* tl, long t_rs, long t_ps,
                               const void* dl, long d_rs, long d_ps, int do_sample) {
  if (dtype != 0 && dtype != 1) return 0;
  if (B < 1 || B > 65535 || G < 1 || G > spec::kMaxDraft || V < 1 || V > 131072) return 0;
  if (tl == nullptr || t_rs < 0 || t_ps < 0) return 0;
  const size_t sz = dtype ? 2 : 4;
  if (reinterpret_cast<uintptr_t>(tl) % sz) return 0;
  if (do_sample && dl == nullptr) return 0;
  if (dl != nullptr && (d_rs < 0 || d_ps < 0 || reinterpret_cast<uintptr_t>(dl) % sz)) return 0;
  return 1;
}

// accept[b][j] (j < G) and alt[b][j] (j <= G) of one round; see the file comment.  round
// comes from round_ptr (device int32) when given, else from the argument.
PA_EXPORT int pa_spec_judge(int dtype, const void* tl, long t_rs, long t_ps, const void* dl, long d_rs, long d_ps,
                            const long long* cand, int B, int G, int V, unsigned long long seed,
                            const int* round_ptr, int round, int do_sample, float temperature, int top_k,
                            float top_p, unsigned char* accept, long long* alt, hipStream_t st) {
  if (!pa_spec_judge_ok(dtype, B, G, V, tl, t_rs, t_ps, dl, d_rs, d_ps, do_sample)) return (int)hipErrorInvalidValue;
  if (cand == nullptr || accept == nullptr || alt == nullptr) return (int)hipErrorInvalidValue;
  spec::JArgs a;
  a.tl = tl; a.t_rs = t_rs; a.t_ps = t_ps; a.dl = dl; a.d_rs = d_rs; a.d_ps = d_ps; a.cand = cand;
  a.B = B; a.G = G; a.V = V; a.seed = seed; a.round_ptr = round_ptr; a.round = round;
  a.do_sample = do_sample;
  a.inv_t = 1.f / fmaxf(temperature, 1e-6f);
  a.top_k = top_k; a.top_p = top_p; a.accept = accept; a.alt = alt;
  const dim3 grid(G + 1, B);
  if (dtype) hipLaunchKernelGGL(spec::judge_kernel<u16>, grid, dim3(smp::kThreads), 0, st, a);
  else hipLaunchKernelGGL(spec::judge_kernel<float>, grid, dim3(smp::kThreads), 0, st, a);
  PA_LAUNCH_CHECK();
}

// The bookkeeping of one round on the generation state; see ops/speculative.py.
PA_EXPORT int pa_spec_commit(const unsigned char* accept, const long long* alt, const long long* cand, int B, int G,
                             long long* out, int max_new, long long* lengths, unsigned char* done, int* pos,
                             long long* tok, int* kept, int* accepted, long eos, long pad, hipStream_t st) {
  if (B < 1 || G < 1 || G > spec::kMaxDraft || max_new < 1) return (int)hipErrorInvalidValue;
  if (accept == nullptr || alt == nullptr || cand == nullptr || out == nullptr || lengths == nullptr ||
      done == nullptr || pos == nullptr || tok == nullptr || kept == nullptr || accepted == nullptr)
    return (int)hipErrorInvalidValue;
  spec::CArgs c;
  c.accept = accept; c.alt = alt; c.cand = cand; c.B = B; c.G = G; c.out = out; c.max_new = max_new;
  c.lengths = lengths; c.done = done; c.pos = pos; c.tok = tok; c.kept = kept; c.accepted = accepted;
  c.eos = eos; c.pad = pad;
  hipLaunchKernelGGL(spec::commit_kernel, dim3((B + 63) / 64), dim3(64), 0, st, c);
  PA_LAUNCH_CHECK();
}
