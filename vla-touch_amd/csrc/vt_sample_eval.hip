// vt_sample_eval.hip — the metrics of fine-tuning's periodic sampling evaluation (VLA/train/sample.py:55-86, `log_sample_res`): masked MSE and
// masked, state-norm-relative L2 error of a sampled action chunk against the ground truth, per sample and over the batch, folded into the
// running per-dataset sums of one evaluation.  The reference forms the per-sample values on the device and then reads them one by one
// (`.item()` in a Python loop) to add them up on the host; here the sums live on the device and the host reads them once per evaluation.
//   kernel 1 (one block per sample): per element in fp32, as the reference's `.float()` tensors, sq = (pred - target)^2 and
//     l2 = sqrt(sq) / (state_norm + 1e-3); sum sq m, sum l2 m and sum m over the sample's H * A elements in fp64 -> ws[b][3].
//   kernel 2 (one thread): per_sample[b] = the two ratios rounded once to fp32; the batch's overall pair from the sums of ws over b; then
//     acc[dataset_idx[b]] += per_sample[b] and count[..] += 1 in index order (what the reference adds through .item()), acc[n_datasets] +=
//     the overall pair.
// Every sum has a fixed order (a thread walks its elements with stride 256, the block folds its 256 partial sums in a tree, one thread
// folds the samples): no atomics, two calls on the same inputs give the same bits.  A sample whose mask is all zero gives 0 / 0 = NaN for
// its pair and for its dataset's row, and adds zero to the overall sums, as in the reference.
#include <math.h>
#include "vt_common.h"
#include "vt_host.h"
#include "../../include/vlatouch.h"

namespace {

template <typename T>
__global__ __launch_bounds__(256) void sample_sums_kernel(const T* __restrict__ pred, const float* __restrict__ target, const float* __restrict__ mask,
                                                          const float* __restrict__ state_norm, double* __restrict__ ws, int H, int A) {
  __shared__ double red[3][256];
  const int b = blockIdx.x, tid = threadIdx.x;
  const long n = (long)H * A;
  const T* p = pred + (long)b * n;
  const float* t = target + (long)b * n;
  const float* m = mask + (long)b * A;
  const float* sn = state_norm + (long)b * A;
  double s_sq = 0.0, s_l2 = 0.0, s_m = 0.0;
  const int step = 256 % A, wrap = A - step;                     // a = i % A walks with the stride: a 32-bit compare and add, no division
  int a = tid % A;
  for (long i = tid; i < n; i += 256, a = a >= wrap ? a - wrap : a + step) {
    const float d = ldf<T>(p, i) - t[i];
    const float sq = d * d;                                     // rounded to fp32 before the square root: the reference's statement
    const float l2 = sqrtf(sq) / (sn[a] + 1e-3f);
    const float mk = m[a];
    s_sq += (double)(sq * mk);                                   // the products are fp32 (a 0 / 1 mask: exact), the sums fp64
    s_l2 += (double)(l2 * mk);
    s_m += (double)mk;
  }
  red[0][tid] = s_sq; red[1][tid] = s_l2; red[2][tid] = s_m;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) { red[0][tid] += red[0][tid + w]; red[1][tid] += red[1][tid + w]; red[2][tid] += red[2][tid + w]; }
    __syncthreads();
  }
  if (tid < 3) ws[(long)b * 3 + tid] = red[tid][0];
}

__global__ __launch_bounds__(64) void sample_fold_kernel(const double* __restrict__ ws, const int* __restrict__ dataset_idx, int B, int n_datasets,
                                                         float* __restrict__ per_sample, float* __restrict__ overall, double* __restrict__ acc,
                                                         int* __restrict__ count) {
  if (threadIdx.x != 0) return;
  double t_sq = 0.0, t_l2 = 0.0, t_m = 0.0;
  for (int b = 0; b < B; ++b) {
    const double s_sq = ws[(long)b * 3], s_l2 = ws[(long)b * 3 + 1], s_m = ws[(long)b * 3 + 2];
    const float mse = (float)(s_sq / s_m), l2 = (float)(s_l2 / s_m);
    per_sample[2 * b] = mse;
    per_sample[2 * b + 1] = l2;
    t_sq += s_sq; t_l2 += s_l2; t_m += s_m;
    const int d = dataset_idx[b];
    if (d >= 0 && d < n_datasets) {                             // the host checks the indices; one outside the table is not written anywhere
      acc[2 * d] += (double)mse;
      acc[2 * d + 1] += (double)l2;
      count[d] += 1;
    }
  }
  const float o_mse = (float)(t_sq / t_m), o_l2 = (float)(t_l2 / t_m);
  overall[0] = o_mse;
  overall[1] = o_l2;
  acc[2 * n_datasets] += (double)o_mse;
  acc[2 * n_datasets + 1] += (double)o_l2;
  count[n_datasets] += 1;
}

}  // namespace

int vt_sample_metrics(const void* pred, int dt, const float* target, const float* mask, const float* state_norm, const int* dataset_idx, int B, int H,
                      int A, int n_datasets, float* per_sample, float* overall, double* acc, int* count, double* ws, vt_stream_t s) {
  if (!pred || !target || !mask || !state_norm || !dataset_idx || !per_sample || !overall || !acc || !count || !ws)
    return vt_fail(VT_ERR_ARG, "vt_sample_metrics: null pointer");
  if (B < 1 || H < 1 || A < 1 || n_datasets < 1) return vt_fail(VT_ERR_ARG, "vt_sample_metrics: B, H, A and n_datasets must be >= 1");
  if (!vt_is_act_dtype(dt)) return vt_fail(VT_ERR_UNSUPPORTED, "vt_sample_metrics: pred dtype must be fp32 (0), bf16 (1) or fp16 (3)");
  DISPATCH_T(dt, T, hipLaunchKernelGGL(sample_sums_kernel<T>, dim3(B), dim3(256), 0, (hipStream_t)s, (const T*)pred, target, mask, state_norm, ws, H, A))
  hipLaunchKernelGGL(sample_fold_kernel, dim3(1), dim3(64), 0, (hipStream_t)s, (const double*)ws, dataset_idx, B, n_datasets, per_sample, overall, acc, count);
  return vt_check_launch();
}
