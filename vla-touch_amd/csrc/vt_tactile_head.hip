// vt_tactile_head.hip — the heads of Octopi's tactile video encoder that are reductions, not Linears (those run on vt_mlp / vt_gemm):
//   video feature   ViFiCLIP.forward (octopi_s/utils/encoder.py:401-411): mean of the l pooled frame features, then / its L2 norm (no eps);
//   retrieval       dataset.py:189-195: nn.CosineSimilarity(dim=1, eps=1e-8) of a saved bank [R][D] against the video feature, then torch.topk(k).
// Batched over b videos that share one bank (the reference calls retrieval once per video).
//   video_kernel   one workgroup per video: a thread owns columns tid, tid + 256, ..; the l frames are added in frame order, the squares are
//                  folded wave_sum -> four waves in wave order.
//   sims_kernel    one wave per (video, bank row): float4 loads, lane-strided over D, wave_sum of the dot product and of |video|^2.
//   topk_kernel    one workgroup per video, k <= 16 rounds of selection: every thread scans its rows (stride 256) for the best (value, index)
//                  not yet taken, the workgroup folds the 256 candidates in a tree.  "Better" = larger value, or the same value at a LOWER
//                  INDEX: ties go to the lower index, as the header says.
// All sums are fp32 in an order fixed by (l, D, R): a video's results do not depend on how many videos the call carries.
#include <math.h>
#include "vt_common.h"
#include "vt_host.h"
#include "../../include/vlatouch.h"

namespace {

constexpr int TOPK_MAX = 16;
inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// sum over the workgroup's 256 threads, the same value in every thread: wave_sum, then the four waves in wave order
__device__ __forceinline__ float block256_sum(float v, float* red) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  const float s = ((red[0] + red[1]) + red[2]) + red[3];
  __syncthreads();
  return s;
}

__global__ __launch_bounds__(256) void video_kernel(const float* __restrict__ pooled, float* __restrict__ video, int l, int D) {
  __shared__ float red[4];
  const float* p = pooled + (long)blockIdx.x * l * D;
  float* o = video + (long)blockIdx.x * D;
  const float inv_l = 1.0f / (float)l;
  float ss = 0.f;
  for (int c = threadIdx.x; c < D; c += 256) {
    float s = 0.f;
    for (int f = 0; f < l; ++f) s += p[(long)f * D + c];
    s *= inv_l;
    o[c] = s;                                                     // the mean, scaled below by the thread that wrote it
    ss += s * s;
  }
  const float inv = 1.0f / sqrtf(block256_sum(ss, red));
  for (int c = threadIdx.x; c < D; c += 256) o[c] *= inv;
}

__global__ __launch_bounds__(256) void rownorm2_kernel(const float* __restrict__ x, float* __restrict__ norm, int R, int D) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= R) return;
  const float4* xr = reinterpret_cast<const float4*>(x + (long)r * D);
  float ss = 0.f;
  for (int c = lane; c < D / 4; c += 64) { const float4 v = xr[c]; ss += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w; }
  ss = wave_sum(ss);
  if (lane == 0) norm[r] = sqrtf(ss);
}

__global__ __launch_bounds__(256) void sims_kernel(const float* __restrict__ video, const float* __restrict__ bank, const float* __restrict__ bank_norm,
                                                   float* __restrict__ sims, int R, int D) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63, v = blockIdx.y;
  if (r >= R) return;
  const float4* br = reinterpret_cast<const float4*>(bank + (long)r * D);
  const float4* vr = reinterpret_cast<const float4*>(video + (long)v * D);
  float dot = 0.f, vv = 0.f;
  for (int c = lane; c < D / 4; c += 64) {
    const float4 a = br[c], x = vr[c];
    dot += a.x * x.x + a.y * x.y + a.z * x.z + a.w * x.w;
    vv += x.x * x.x + x.y * x.y + x.z * x.z + x.w * x.w;
  }
  dot = wave_sum(dot); vv = wave_sum(vv);
  if (lane == 0) sims[(long)v * R + r] = dot / (fmaxf(bank_norm[r], 1e-8f) * fmaxf(sqrtf(vv), 1e-8f));
}

__device__ __forceinline__ bool better(float av, int ai, float bv, int bi) { return av > bv || (av == bv && ai < bi); }

__global__ __launch_bounds__(256) void topk_kernel(const float* __restrict__ sims, int* __restrict__ idx, float* __restrict__ val, int R, int k) {
  __shared__ float sv[256];
  __shared__ int si[256];
  __shared__ int taken[TOPK_MAX];
  const float* s = sims + (long)blockIdx.x * R;
  const int tid = threadIdx.x;
  for (int j = 0; j < k; ++j) {
    float bv = -INFINITY; int bi = 0x7fffffff;
    for (int r = tid; r < R; r += 256) {
      bool free_ = true;
      for (int t = 0; t < j; ++t) free_ = free_ && taken[t] != r;
      const float x = s[r];
      if (free_ && better(x, r, bv, bi)) { bv = x; bi = r; }
    }
    sv[tid] = bv; si[tid] = bi;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
      if (tid < w && better(sv[tid + w], si[tid + w], sv[tid], si[tid])) { sv[tid] = sv[tid + w]; si[tid] = si[tid + w]; }
      __syncthreads();
    }
    if (tid == 0) {
      int pick = si[0];
      if (pick == 0x7fffffff) {                                   // every free similarity is NaN (a zero video feature): the lowest free index, value NaN
        for (pick = 0; pick < R; ++pick) {
          bool free_ = true;
          for (int t = 0; t < j; ++t) free_ = free_ && taken[t] != pick;
          if (free_) break;
        }
        sv[0] = s[pick];
      }
      taken[j] = pick; idx[(long)blockIdx.x * k + j] = pick; val[(long)blockIdx.x * k + j] = sv[0];
    }
    __syncthreads();
  }
}

}  // namespace

int vt_tactile_bank_norms(const float* bank, int R, int D, float* bank_norm, vt_stream_t stream) {
  if (!bank || !bank_norm) return vt_fail(VT_ERR_ARG, "vt_tactile_bank_norms: null pointer");
  if (R < 1 || D < 1 || D % 4) return vt_fail(VT_ERR_ARG, "vt_tactile_bank_norms: R, D >= 1 and D %% 4 == 0 are required");
  if (!al16(bank)) return vt_fail(VT_ERR_ARG, "vt_tactile_bank_norms: bank must be 16-byte aligned");
  hipLaunchKernelGGL(rownorm2_kernel, dim3((R + 3) / 4), dim3(256), 0, (hipStream_t)stream, bank, bank_norm, R, D);
  return vt_check_launch();
}

int vt_tactile_head(const float* pooled, int b, int l, int D, const float* bank, const float* bank_norm, int R, int k, float* video, float* sims,
                    int* topk_idx, float* topk_val, vt_stream_t stream) {
  if (!pooled || !video) return vt_fail(VT_ERR_ARG, "vt_tactile_head: null pooled / video");
  if (b < 1 || l < 1 || D < 1 || D % 4 || b > 65535) return vt_fail(VT_ERR_ARG, "vt_tactile_head: 1 <= b <= 65535, l, D >= 1 and D %% 4 == 0 are required");
  if (bank && (!al16(bank) || !al16(video))) return vt_fail(VT_ERR_ARG, "vt_tactile_head: bank and video must be 16-byte aligned");
  if (bank) {
    if (!bank_norm || !sims) return vt_fail(VT_ERR_ARG, "vt_tactile_head: a bank needs bank_norm and sims");
    if (R < 1 || k < 0 || k > R || k > TOPK_MAX) return vt_fail(VT_ERR_ARG, "vt_tactile_head: R >= 1 and 0 <= k <= min(R, %d) are required (R %d, k %d)", TOPK_MAX, R, k);
    if (k > 0 && (!topk_idx || !topk_val)) return vt_fail(VT_ERR_ARG, "vt_tactile_head: k > 0 needs topk_idx and topk_val");
  }
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(video_kernel, dim3(b), dim3(256), 0, s, pooled, video, l, D);
  if (bank) {
    hipLaunchKernelGGL(sims_kernel, dim3((R + 3) / 4, b), dim3(256), 0, s, (const float*)video, bank, bank_norm, sims, R, D);
    if (k > 0) hipLaunchKernelGGL(topk_kernel, dim3(b), dim3(256), 0, s, (const float*)sims, topk_idx, topk_val, R, k);
  }
  return vt_check_launch();
}
