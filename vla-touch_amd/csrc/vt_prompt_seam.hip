// vt_prompt_seam.hip — the deep visual prompts of the CLIP tactile tower (octopi_s/utils/encoder.py:59-91, 108-124, vision branch) between
// two blocks of vt_dino_forward, on the fp32 residual stream tok [Bt][rows][D] whose last n rows per image are the prompt rows ("the tail").
//   prompt_seam_kernel: ONE launch between block i-1 and block i, per element of the Bt * n tail rows and in this order:
//     gate of block i-1   v = g * v + (1 - g) * before      (g = sigmoid(VPT_gamma_{i-1}), a device scalar; `before` = the tail as block i-1 received it)
//     save                before = v                          (block i will gate against what arrives now)
//     overwrite           v = VPT_shallow_i                   (the rows block i sees; not normed)
//     The two products and the sum of the gate are rounded separately (no fma contraction): the result is the fp32 statement's, bit for bit.
//     16-byte accesses, one float4 per thread over Bt * n * D / 4; D % 4 == 0 is the only assumption on D.
//   prompt_compact_kernel: block P drops the tail: [Bt][rows][D] -> [Bt][rows - n][D] out of place (any grid), or
//   prompt_compact_inplace_kernel: the same in place by ONE workgroup that walks the stream front to back in chunks of 1024 float4: every lane
//     loads its vector, a barrier, every lane stores.  A destination lies at or below its source, and chunks are taken in ascending order, so
//     no store lands on a vector that is still to be read.
#include "vt_common.h"
#include "vt_host.h"
#include "../../include/vlatouch.h"

namespace {

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

__global__ __launch_bounds__(256) void prompt_seam_kernel(float* __restrict__ tok, long img4, long tail4, int nD4, long total4, const float* __restrict__ gate,
                                                          float* __restrict__ before, int save, const float* __restrict__ shallow) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;          // float4 index into [Bt][n][D / 4]
  if (i >= total4) return;
  const long b = i / nD4;
  const int j = (int)(i - b * nD4);                             // float4 index inside one image's tail = inside VPT_shallow
  float4* t = reinterpret_cast<float4*>(tok) + b * img4 + tail4 + j;
  float4* bf = reinterpret_cast<float4*>(before) + i;
  float4 v;
  if (gate || save) v = *t;
  if (gate) {
#pragma clang fp contract(off)      // g * v + h * o with three roundings: the compiler's default would fuse one product into an fma
    const float g = *gate, h = 1.0f - g;
    const float4 o = *bf;
    v.x = g * v.x + h * o.x; v.y = g * v.y + h * o.y;
    v.z = g * v.z + h * o.z; v.w = g * v.w + h * o.w;
  }
  if (save) *bf = v;
  if (shallow) v = reinterpret_cast<const float4*>(shallow)[j];
  if (gate || shallow) *t = v;
}

__global__ __launch_bounds__(256) void prompt_compact_kernel(const float* __restrict__ src, float* __restrict__ dst, long src4, long dst4, long total4) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;          // float4 index into dst [Bt][dst4]
  if (i >= total4) return;
  const long b = i / dst4;
  reinterpret_cast<float4*>(dst)[i] = reinterpret_cast<const float4*>(src)[b * src4 + (i - b * dst4)];
}

__global__ __launch_bounds__(1024) void prompt_compact_inplace_kernel(float* tok, long src4, long dst4, long total4) {
  float4* t = reinterpret_cast<float4*>(tok);
  for (long c = dst4; c < total4; c += 1024) {                   // image 0 stays where it is
    const long i = c + threadIdx.x;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < total4) { const long b = i / dst4; v = t[b * src4 + (i - b * dst4)]; }
    __syncthreads();
    if (i < total4) t[i] = v;
    __syncthreads();
  }
}

}  // namespace

int vt_prompt_seam(float* tok, int Bt, int rows, int n, int D, const float* gate, float* before, int save, const float* shallow, vt_stream_t stream) {
  if (!tok) return vt_fail(VT_ERR_ARG, "vt_prompt_seam: null tok");
  if (Bt < 1 || n < 1 || D < 1 || n > rows || D % 4) return vt_fail(VT_ERR_ARG, "vt_prompt_seam: Bt, n, D >= 1, n <= rows and D %% 4 == 0 are required");
  if ((gate || save) && !before) return vt_fail(VT_ERR_ARG, "vt_prompt_seam: gate and save need `before`");
  if (!gate && !save && !shallow) return vt_fail(VT_ERR_ARG, "vt_prompt_seam: nothing to do");
  if (!al16(tok) || !al16(before) || !al16(shallow)) return vt_fail(VT_ERR_ARG, "vt_prompt_seam: tok, before and shallow must be 16-byte aligned");
  const long nD4 = (long)n * D / 4, total4 = (long)Bt * nD4;
  if (nD4 >= (1L << 31) || (total4 + 255) / 256 >= (1L << 31)) return vt_fail(VT_ERR_ARG, "vt_prompt_seam: too many elements");
  hipLaunchKernelGGL(prompt_seam_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, tok, (long)rows * D / 4,
                     (long)(rows - n) * D / 4, (int)nD4, total4, gate, before, save, shallow);
  return vt_check_launch();
}

int vt_prompt_compact(const float* src, float* dst, int Bt, int rows, int n, int D, vt_stream_t stream) {
  if (!src || !dst) return vt_fail(VT_ERR_ARG, "vt_prompt_compact: null pointer");
  if (Bt < 1 || D < 1 || n < 1 || n >= rows || D % 4) return vt_fail(VT_ERR_ARG, "vt_prompt_compact: Bt, D, n >= 1, n < rows and D %% 4 == 0 are required");
  if (!al16(src) || !al16(dst)) return vt_fail(VT_ERR_ARG, "vt_prompt_compact: src and dst must be 16-byte aligned");
  const long src4 = (long)rows * D / 4, dst4 = (long)(rows - n) * D / 4, total4 = (long)Bt * dst4;
  if ((total4 + 255) / 256 >= (1L << 31)) return vt_fail(VT_ERR_ARG, "vt_prompt_compact: too many elements");
  if (src == dst) {
    if (Bt > 1) hipLaunchKernelGGL(prompt_compact_inplace_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, dst, src4, dst4, total4);
  } else {
    hipLaunchKernelGGL(prompt_compact_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, src, dst, src4, dst4, total4);
  }
  return vt_check_launch();
}
