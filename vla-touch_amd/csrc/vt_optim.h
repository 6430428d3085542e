// vt_optim.h — what every optimizer kernel has to agree on, stated once: one element of torch.optim.AdamW / torch_ema, and the multi-tensor
// table (record, chunk size, chunk -> row lookup) of vt_adamw_ema_multi, vt_grad_clip_multi, vt_grad_accum_multi, vt_ema_multi,
// vt_grad_fold_pack_multi, vt_grad_unpack_multi (vt_train.hip, vt_train_rdt.hip) and vt_adamw8_ema_multi (vt_adam8.hip).  Contraction is switched off in the element functions so that all
// of their users round identically: a replayed graph and the eager step, the EMA-only launch and the per-tensor one, and the 8-bit step's
// fp32 tensors and the 32-bit step, then agree bit for bit.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ float adamw_elem(float p, float gv, float& m, float& v, float lr, float b1, float b2, float eps, float wd, float bc1, float bc2_sqrt) {
#pragma clang fp contract(off)
  const float pv = p * (1.0f - lr * wd);
  const float mv = b1 * m + (1.0f - b1) * gv;
  const float vv = b2 * v + (1.0f - b2) * gv * gv;
  m = mv; v = vv;
  const float denom = sqrtf(vv) / bc2_sqrt + eps;
  return pv - (lr / bc1) * (mv / denom);
}
__device__ __forceinline__ float ema_elem(float sh, float p, float one_minus_decay) {
#pragma clang fp contract(off)
  return sh - one_minus_decay * (sh - p);
}

// The table: a step updates ~380 tensors, most of them a few KB, so one launch walks them all.  tab[k] is the record documented in
// include/vlatouch.h; a 256-thread block owns one MT_CHUNK-element chunk and finds its row by binary search over first_chunk (the running
// sum of ceil(n / MT_CHUNK)).  g is written by the clip and accumulate kernels; m / v point at `unsigned char` codes in a row whose
// moments vt_adamw8_ema_multi keeps quantised (it casts).  vlatouch/train.py's `mt_table` builds the rows.
struct MtEntry { float* p; float* g; float* m; float* v; float* shadow; long n; long first_chunk; };
constexpr int MT_CHUNK = 4096;
__device__ __forceinline__ int mt_find(const MtEntry* tab, int ntensors, long chunk) {
  int lo = 0, hi = ntensors - 1;
  while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (tab[mid].first_chunk <= chunk) lo = mid; else hi = mid - 1; }
  return lo;
}

// One chunk of a tensor with fp32 moments, 256 threads: the body of the multi-tensor AdamW + EMA kernels (vt_train.hip's
// adamw_ema_mt_kernel, and vt_adam8.hip's for a tensor it leaves unquantised), kept here so that the two cannot drift apart.
__device__ __forceinline__ void adamw_ema_chunk_f32(float* p, const float* g, float* m, float* v,
                                                    float* shadow, long base, long n, float lr, float b1, float b2, float eps, float wd,
                                                    float bc1, float bc2_sqrt, float omd) {
  static_assert(16 * 256 == MT_CHUNK, "16 passes of 256 threads walk one chunk");
#pragma unroll 4
  for (int it = 0; it < 16; ++it) {
    const long i = base + it * 256 + threadIdx.x;
    if (i >= n) break;
    float mv = m[i], vv = v[i];
    const float pv = adamw_elem(p[i], g[i], mv, vv, lr, b1, b2, eps, wd, bc1, bc2_sqrt);
    m[i] = mv; v[i] = vv;
    p[i] = pv;
    if (shadow) shadow[i] = ema_elem(shadow[i], pv, omd);
  }
}
