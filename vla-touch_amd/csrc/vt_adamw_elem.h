// vt_adamw_elem.h — one element of torch.optim.AdamW / torch_ema, shared by every optimizer kernel (vt_train.hip: scalar arguments, scalars from
// device memory, multi-tensor table; vt_adam8.hip: block-wise 8-bit moments).  Contraction is switched off so that all of them round
// identically: a replayed graph and the eager step, and the 8-bit step's fp32 tensors and the 32-bit step, then agree bit for bit.
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
// One 4096-element chunk of a tensor with fp32 moments, 256 threads: the body of the multi-tensor AdamW + EMA kernels (vt_train.hip's
// adamw_ema_mt_kernel, and vt_adam8.hip's for a tensor it leaves unquantised), kept here so that the two cannot drift apart.
__device__ __forceinline__ void adamw_ema_chunk_f32(float* p, const float* g, float* m, float* v,
                                                    float* shadow, long base, long n, float lr, float b1, float b2, float eps, float wd,
                                                    float bc1, float bc2_sqrt, float omd) {
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
