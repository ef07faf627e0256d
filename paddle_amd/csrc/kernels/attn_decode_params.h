// The launch parameters of the split-KV decode attention kernels, shared by the VALU kernel
// and the merge kernel (attn_decode.hip) and the MFMA kernel (attn_decode_gqa.hip).
#pragma once
#include "common.h"

namespace dec {

constexpr int kMaxSplits = 64;

struct DecodeParams {
  const pa::u16* q;
  long qsb, qsh;  // element strides of q [B, 1, Hq, D] over b and head
  const pa::u16* kc;
  const pa::u16* vc;
  const int* kv_len;
  float* ws;   // [B, Hq, ns, 2] (m, l) then [B, Hq, ns, D] acc
  pa::u16* o;  // [B, 1, Hq, D] contiguous
  int B, S_max, Hq, Hk, ns;
  float scale_log2;  // scale * log2(e): scores live in the log2 domain
  // paged only: kc / vc are pools [num_blocks, 1 << bs_shift, Hk, D]
  const int* table;  // [B, max_blocks]
  int max_blocks, num_blocks, bs_shift;
  // e4m3 only: kc / vc hold one byte per element, ks / vs one scale per (slot, kv head)
  const float* ks;
  const float* vs;
};

// attn_decode_gqa.hip: every split's partial (m, l, acc[D]) into p.ws, for any 1 <= Hq / Hk
// <= 16.  p.table null: a contiguous cache; p.ks null: a bf16 one.  D is 64 or 128.  The merge
// kernel of attn_decode.hip finishes the job.
void launch_decode_gqa(const DecodeParams& p, int D, hipStream_t st);

}  // namespace dec
