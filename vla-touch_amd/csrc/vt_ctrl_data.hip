// vt_ctrl_data.hip — one controller-training batch out of device-resident episodes (vlatouch/ctrl_data.py, `ControllerStore.assemble`).
// Stands for what the reference does per sample on host workers and per step on the device: ControllerDataset.__getitem__
// (controller_dataset.py:101-170, restated by vlatouch.eval.make_sample: the window's pose rows with the gripper of rows >= cf divided by
// 255, the VLA chunk of frame start + cf, the force rows), normalize_actions (:303-346), the slicing of `_prepare_batch_for_diffusion`
// (bridge_train.py:105-164) / `_prepare_batch` (lstm_train.py:56-84) and the concatenation [cls_cam1 | cls_cam2 | state | force] in front of the
// observation MLP.  The frozen DINOv2 tower does not run: the CLS vector of every frame was encoded once, with the ImageNet normalisation off
// (mode 0) and on (mode 1), and the batch picks the mode the reference's whole-batch decision gives (visual_encoder.py:78,100).
//   launch 1, one block: per camera the exact integer sum of the batch's frame sums -> norm_flags[cam] = 2 * sum >= 255 * B * P.
//   launch 2, one block per (sample, part): part 0 the obs_in row (16-byte words along dv when the row pitch allows it, else scalar; the
//     state and force columns and the zero padding), part 1 the two action chunks (16-byte fp64 loads, two values per lane: the gripper is the
//     second of its pair; /255 in fp64, one rounding to fp32, then vt_actnorm, the arithmetic of vt_action_normalize), part 2 the force rows.
//   vt_ctrl_pixsum, one block per frame: the byte sums the decision reads, taken when the store is built.
// Integer sums, no atomics, no host read: two calls give the same bits.  A plan entry outside the tables (the host refuses those before the
// launch) reads nothing: its rows are written as NaN and it adds nothing to the sums.
#include <math.h>
#include "vt_common.h"
#include "vt_host.h"
#include "../../include/vlatouch.h"

namespace {

typedef __attribute__((ext_vector_type(2))) double double2_t;
typedef unsigned long long u64;

// Row of the tables that holds the window's last context frame (start + cf - 1), or -1 when the episode is not in the tables or too short
// for one window.  The start is clamped so that every row the window reads (up to start + cf + h - 1) lies inside its episode.
__device__ __forceinline__ long ctrl_frame_row(const int* __restrict__ plan, const int* __restrict__ ep_off, int E, long rows, int cf, int h, int b) {
  const int e = plan[2 * b];
  if (e < 0 || e >= E) return -1;
  const long off = ep_off[e], n = (long)ep_off[e + 1] - off;
  if (off < 0 || off + n > rows || n < (long)cf + h) return -1;
  const long start = min(max((long)plan[2 * b + 1], 0l), n - cf - h);
  return off + start + cf - 1;
}

// sum over the block's 256 threads (whole numbers: the order does not matter)
__device__ __forceinline__ u64 block256_sum(u64 v, u64* sh) {
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
    __syncthreads();
  }
  const u64 r = sh[0];
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(256) void ctrl_pixsum_kernel(const unsigned char* __restrict__ frames, long P, u64* __restrict__ sums) {
  __shared__ u64 sh[256];
  const unsigned char* f = frames + (long)blockIdx.x * P;
  const long nvec = ((reinterpret_cast<size_t>(f) & 15) == 0) ? P / 16 : 0;
  u64 acc = 0;
  const uint4* v4 = reinterpret_cast<const uint4*>(f);
  for (long i = threadIdx.x; i < nvec; i += 256) {
    const uint4 q = v4[i];
    const unsigned w[4] = {q.x, q.y, q.z, q.w};
    unsigned t = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) t += (w[k] & 0x00ff00ffu) + ((w[k] >> 8) & 0x00ff00ffu);      // two 16-bit lanes, each at most 8 * 255
    acc += (t & 0xffffu) + (t >> 16);
  }
  for (long i = nvec * 16 + threadIdx.x; i < P; i += 256) acc += f[i];                       // unaligned frame or a tail
  acc = block256_sum(acc, sh);
  if (threadIdx.x == 0) sums[blockIdx.x] = acc;
}

__global__ __launch_bounds__(256) void ctrl_decide_kernel(const u64* __restrict__ pix_sum, const int* __restrict__ ep_off, const int* __restrict__ plan,
                                                          int E, long rows, long P, int cf, int h, int B, float* __restrict__ norm_flags) {
  __shared__ u64 sh[256];
  u64 a0 = 0, a1 = 0;
  for (int b = threadIdx.x; b < B; b += 256) {
    const long fr = ctrl_frame_row(plan, ep_off, E, rows, cf, h, b);
    if (fr >= 0) { a0 += pix_sum[fr]; a1 += pix_sum[rows + fr]; }
  }
  a0 = block256_sum(a0, sh);
  a1 = block256_sum(a1, sh);
  if (threadIdx.x == 0) {
    const u64 half = (u64)255 * (u64)B * (u64)P;                 // mean >= 0.5  <=>  2 * sum >= 255 * B * P
    norm_flags[0] = 2 * a0 >= half ? 1.f : 0.f;
    norm_flags[1] = 2 * a1 >= half ? 1.f : 0.f;
  }
}

__global__ __launch_bounds__(128) void ctrl_batch_kernel(const double* __restrict__ pose10, const double* __restrict__ vla, const float* __restrict__ forces,
                                                         const int* __restrict__ ep_off, const float* __restrict__ feat, const float* __restrict__ stats,
                                                         const int* __restrict__ plan, const float* __restrict__ norm_flags, int E, long rows, int Hv, int Fd,
                                                         int dv, float pad, int cf, int h, int bridge, int fdo, int vec, float* __restrict__ obs_in, int in_pad,
                                                         float* __restrict__ expert_act, float* __restrict__ vla_act, float* __restrict__ forces_out,
                                                         float* __restrict__ current_force) {
  const int b = blockIdx.x, part = blockIdx.y, tid = threadIdx.x;
  const long fr = ctrl_frame_row(plan, ep_off, E, rows, cf, h, b);
  const float nanv = __builtin_nanf("");
  if (part == 0) {
    float* o = obs_in + (long)b * in_pad;
    if (fr < 0) {
      for (int j = tid; j < in_pad; j += 128) o[j] = nanv;
      return;
    }
    const float* s0 = feat + ((0 * rows + fr) * 2 + (norm_flags[0] != 0.f ? 1 : 0)) * dv;
    const float* s1 = feat + ((1 * rows + fr) * 2 + (norm_flags[1] != 0.f ? 1 : 0)) * dv;
    if (vec) {
      for (int i = tid; i < dv / 4; i += 128) {
        const float4_t v0 = ((const float4_t*)s0)[i], v1 = ((const float4_t*)s1)[i];
        ((float4_t*)o)[i] = v0;
        ((float4_t*)(o + dv))[i] = v1;
      }
    } else {
      for (int i = tid; i < dv; i += 128) { o[i] = s0[i]; o[dv + i] = s1[i]; }
    }
    for (int j = tid; j < in_pad - 2 * dv; j += 128)             // state (not divided: make_sample divides rows >= cf only) | force | zeros
      o[2 * dv + j] = j < 10 ? (float)pose10[fr * 10 + j] : j < 10 + fdo ? forces[fr * Fd + (j - 10)] : 0.f;
  } else if (part == 1) {
    const int pairs = h * 5;
    for (int idx = tid; idx < 2 * pairs; idx += 128) {
      const int which = idx >= pairs, el = 2 * (idx - which * pairs), col = el % 10;
      float* o = (which ? vla_act : expert_act) + (long)b * h * 10 + el;
      float2_t r = {nanv, nanv};
      if (fr >= 0) {
        const double* src = which ? vla + (fr + 1) * Hv * 10 : pose10 + (fr + 1) * 10;      // rows start + cf ..: one contiguous run of h * 10
        double2_t v = *(const double2_t*)(src + el);
        if (col == 8) v.y = v.y / 255.0;                          // the gripper, in fp64 as make_sample divides it
        const float* mn = stats + which * 20;
        r.x = vt_actnorm((float)v.x, mn[col], mn[10 + col], pad, 0);
        r.y = vt_actnorm((float)v.y, mn[col + 1], mn[10 + col + 1], pad, 0);
      }
      *(float2_t*)o = r;
    }
  } else {
    const long f0 = bridge ? fr + 1 : fr;                         // bridge: forces[:, cf:]; LSTM: forces[:, cf - 1:-1]
    for (int j = tid; j < h * Fd; j += 128) forces_out[(long)b * h * Fd + j] = fr >= 0 ? forces[f0 * Fd + j] : nanv;
    if (current_force)
      for (int j = tid; j < Fd; j += 128) current_force[(long)b * Fd + j] = fr >= 0 ? forces[fr * Fd + j] : nanv;
  }
}

}  // namespace

int vt_ctrl_pixsum(const unsigned char* frames, long long P, int n, unsigned long long* sums, vt_stream_t s) {
  if (!frames || !sums) return vt_fail(VT_ERR_ARG, "vt_ctrl_pixsum: null pointer");
  if (P < 1 || n < 1) return vt_fail(VT_ERR_ARG, "vt_ctrl_pixsum: P and n must be >= 1 (got P=%lld n=%d)", P, n);
  hipLaunchKernelGGL(ctrl_pixsum_kernel, dim3(n), dim3(256), 0, (hipStream_t)s, frames, (long)P, sums);
  return vt_check_launch();
}

int vt_ctrl_batch(const double* pose10, const double* vla, const float* forces, const int* ep_off, const float* feat, const unsigned long long* pix_sum,
                  int E, long long rows, int Hv, int Fd, int dv, long long P, const float* stats, float padding_factor, int cf, int h, int layout,
                  int use_force, const int* plan, int B, float* obs_in, int in_pad, float* expert_act, float* vla_act, float* forces_out,
                  float* current_force, float* norm_flags, vt_stream_t s) {
  if (!pose10 || !vla || !forces || !ep_off || !feat || !pix_sum || !stats || !plan || !obs_in || !expert_act || !vla_act || !forces_out || !norm_flags)
    return vt_fail(VT_ERR_ARG, "vt_ctrl_batch: null pointer");
  if (layout != VT_CTRL_BRIDGE && layout != VT_CTRL_LSTM) return vt_fail(VT_ERR_ARG, "vt_ctrl_batch: layout must be VT_CTRL_BRIDGE or VT_CTRL_LSTM, got %d", layout);
  if (layout == VT_CTRL_BRIDGE && !current_force) return vt_fail(VT_ERR_ARG, "vt_ctrl_batch: the bridge layout needs current_force");
  if (E < 1 || rows < 1 || Hv < 1 || Fd < 1 || dv < 1 || P < 1 || cf < 1 || h < 1 || B < 1)
    return vt_fail(VT_ERR_ARG, "vt_ctrl_batch: E, rows, Hv, Fd, dv, P, cf, h and B must be >= 1 (got E=%d rows=%lld Hv=%d Fd=%d dv=%d P=%lld cf=%d h=%d B=%d)", E,
                   rows, Hv, Fd, dv, P, cf, h, B);
  if (h > Hv) return vt_fail(VT_ERR_ARG, "vt_ctrl_batch: h = %d rows are asked of VLA chunks of Hv = %d", h, Hv);
  if (B > (1 << 20) || P > (1ll << 32) || rows > (1ll << 31) - 1 || h > (1 << 20) || Fd > 1024 || cf > (1 << 20))
    return vt_fail(VT_ERR_ARG, "vt_ctrl_batch: B, h, cf <= 2^20, Fd <= 1024, P <= 2^32 and rows < 2^31 (the decision's 64-bit sums and the index arithmetic)");
  const int fdo = layout == VT_CTRL_BRIDGE && use_force ? Fd : 0;
  if ((long long)in_pad < 2ll * dv + 10 + fdo)
    return vt_fail(VT_ERR_ARG, "vt_ctrl_batch: in_pad = %d is smaller than the row 2 * %d + 10 + %d", in_pad, dv, fdo);
  if ((uintptr_t)pose10 % 16 || (uintptr_t)vla % 16 || (uintptr_t)expert_act % 8 || (uintptr_t)vla_act % 8)
    return vt_fail(VT_ERR_ARG, "vt_ctrl_batch: pose10 and vla must be 16-byte aligned, expert_act and vla_act 8-byte aligned");
  const int vec = dv % 4 == 0 && in_pad % 4 == 0 && (uintptr_t)feat % 16 == 0 && (uintptr_t)obs_in % 16 == 0;
  hipLaunchKernelGGL(ctrl_decide_kernel, dim3(1), dim3(256), 0, (hipStream_t)s, (const u64*)pix_sum, ep_off, plan, E, (long)rows, (long)P, cf, h, B, norm_flags);
  hipLaunchKernelGGL(ctrl_batch_kernel, dim3(B, 3), dim3(128), 0, (hipStream_t)s, pose10, vla, forces, ep_off, feat, stats, plan, norm_flags, E, (long)rows,
                     Hv, Fd, dv, padding_factor, cf, h, layout == VT_CTRL_BRIDGE, fdo, vec, obs_in, in_pad, expert_act, vla_act, forces_out, current_force);
  return vt_check_launch();
}
