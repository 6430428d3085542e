// vt_optim.h — what every optimizer kernel has to agree on, stated once: one element of torch.optim.AdamW / torch_ema and of the gradient
// fold, and the multi-tensor table (record, chunk size, chunk -> row lookup, a block's chunk and the walk over it) of vt_adamw_ema_multi
// (vt_train.hip), vt_adamw8_ema_multi (vt_adam8.hip) and, in vt_train_rdt.hip, vt_grad_clip_multi, vt_grad_unscale_clip_multi,
// vt_grad_accum_multi, vt_grad_fold_pack_multi, vt_grad_unpack_multi and vt_ema_multi.  Contraction is switched off in the AdamW and EMA
// element functions so that all of their users round identically: a replayed graph and the eager step, the EMA-only launch and the
// per-tensor one, and the 8-bit step's fp32 tensors and the 32-bit step, then agree bit for bit.
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
// One element of a micro-batch's gradient folded into its accumulator: stored as g * scale by a window's first micro-batch (acc is not looked
// at), added with one rounding by the others.  vt_grad_accum_multi stores this value and vt_grad_fold_pack_multi rounds it to bf16, so the
// bf16 exchange rounds exactly what the fp32 one would have summed.
__device__ __forceinline__ float grad_fold_elem(float g, float scale, float acc, int accumulate) { return accumulate ? fmaf(g, scale, acc) : g * scale; }

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
// This block's chunk: the table row it belongs to, the row's record, the chunk's first element within the tensor and how many of the
// tensor's n elements it holds (MT_CHUNK but for a tensor's last chunk).  A chunk starts 16 KiB into its tensor, so a tensor's 16-byte
// alignment is its chunks'.
struct MtChunk { int row; MtEntry e; long base; int cnt; };
__device__ __forceinline__ MtChunk mt_chunk(const MtEntry* __restrict__ tab, int ntensors) {
  MtChunk c;
  c.row = mt_find(tab, ntensors, blockIdx.x);
  c.e = tab[c.row];
  c.base = ((long)blockIdx.x - c.e.first_chunk) * MT_CHUNK;
  const long left = c.e.n - c.base;
  c.cnt = left < MT_CHUNK ? (int)left : MT_CHUNK;
  return c;
}
// The walk of 256 threads over a chunk's cnt elements: quad(j) for every whole 16-byte word j when the caller found its pointers 16-byte
// aligned (which pointers count differs from kernel to kernel), then elem(i) for what is left of cnt behind the last whole word, or for
// the whole chunk of an unaligned tensor.
template <typename QuadFn, typename ElemFn>
__device__ __forceinline__ void mt_walk(int cnt, bool aligned, QuadFn quad, ElemFn elem) {
  static_assert(4 * 256 * 4 == MT_CHUNK, "4 float4 passes of 256 threads walk one chunk");
  const int quads = aligned ? cnt >> 2 : 0;
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int j = it * 256 + threadIdx.x;
    if (j >= quads) break;
    quad(j);
  }
  for (int i = quads * 4 + threadIdx.x; i < cnt; i += 256) elem(i);
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
