// vt_rdt_data.hip — one fine-tuning micro-batch out of device-resident episodes (vlatouch/rdt_data.py, `EpisodeStore.assemble`).
// Stands for what the reference does per sample on host workers: UnifiedVLADataset.parse_file (data/unified_vla_dataset_episode.py:314-351:
// the action chunk from action_id = step_id + 2, padded with its last row; the state row; the episode's std / norm; fill_in_state into the
// unified vector), VLAConsumerDataset.__getitem__ (train/dataset.py:327-344: the control frequency, the state noise, the three condition
// masks) and DataCollatorForVLAConsumerDataset (train/dataset.py:502-530: the stacks, the zero-padded language embeddings and their mask).
// The random decisions are made on the host (the plan); the kernels only gather.
//   launch 1, one block per (sample, row), rows = state | H actions | element mask | state norm: every thread PULLS the unified columns
//     a = tid, tid + 128, .. through the inverse column map (-1 = a column the robot does not fill: 0), so nothing scatters.  The noised
//     state is qpos + (0 + (std / c) * z) in fp64 without contraction, the reference's statement; every value is rounded to fp32 once, at
//     its store.  Row 0's first thread writes the sample's control frequency (0 when masked).
//   launch 2, one block per (sample, token): D floats of the episode's instruction embedding (zeros past its length) and the mask byte;
//     128-bit words when D % 4 == 0 and both bases are 16-byte aligned, else scalar.
// No atomics, no reduction, no host read: two calls give the same bits.  A plan entry outside the tables (the host refuses those before the
// launch) reads nothing: its rows are written as NaN.
#include <math.h>
#include "vt_common.h"
#include "vt_host.h"
#include "../../include/vlatouch.h"

namespace {

__global__ __launch_bounds__(128) void rdt_batch_rows_kernel(const double* __restrict__ qpos, const int* __restrict__ ep_off,
                                                             const double* __restrict__ ep_stats, const double* __restrict__ ds_mean,
                                                             const int* __restrict__ col_map, const int* __restrict__ plan,
                                                             const double* __restrict__ z, int E, int S, int A, int H, int ctrl_freq,
                                                             double noise_div, float* __restrict__ states, float* __restrict__ actions,
                                                             float* __restrict__ elem_mask, float* __restrict__ state_norm,
                                                             long long* __restrict__ ctrl_freqs) {
#pragma clang fp contract(off)
  const int r = blockIdx.x, b = blockIdx.y;                      // r: 0 state, 1 .. H actions, H + 1 element mask, H + 2 state norm
  const int e = plan[4 * b], flags = plan[4 * b + 2];
  int step = plan[4 * b + 1];
  float* out = r == 0 ? states + (long)b * A : r <= H ? actions + ((long)b * H + (r - 1)) * A
             : r == H + 1 ? elem_mask + (long)b * A : state_norm + (long)b * A;
  const bool ok = e >= 0 && e < E;
  const int off = ok ? ep_off[e] : 0, n = ok ? ep_off[e + 1] - off : 0;
  if (n < 1) {                                                   // not a row of the tables: visible, and nothing is read
    for (int a = threadIdx.x; a < A; a += 128) out[a] = __builtin_nanf("");
    if (r == 0 && threadIdx.x == 0) ctrl_freqs[b] = 0;
    return;
  }
  step = min(max(step, 0), n - 1);
  if (r == 0 && threadIdx.x == 0) ctrl_freqs[b] = (flags & VT_RDT_MASK_FREQ) ? 0 : (long long)ctrl_freq;
  const double* st = ep_stats + (long)e * 3 * S;                 // [std | mean | norm][S]
  const long row = r == 0 ? off + step : off + min(step + 2 + (r - 1), n - 1);      // action_id = step_id + 2, padded with the last row
  for (int a = threadIdx.x; a < A; a += 128) {
    const int s = col_map[a];
    double v = 0.0;
    if (s >= 0 && s < S) {
      if (r == 0) {
        if (flags & VT_RDT_MASK_STATE) v = ds_mean[s];
        else {
          v = qpos[row * S + s];
          if (flags & VT_RDT_NOISE) v = v + (0.0 + (st[s] / noise_div) * z[(long)b * S + s]);
        }
      } else if (r <= H) v = qpos[row * S + s];
      else if (r == H + 1) v = (flags & VT_RDT_MASK_ELEM) ? 0.0 : 1.0;
      else v = st[2 * S + s];
    }
    out[a] = (float)v;
  }
}

__global__ __launch_bounds__(64) void rdt_batch_lang_kernel(const float* __restrict__ lang, const int* __restrict__ lang_off,
                                                            const int* __restrict__ plan, int E, int D, int Lmax, int vec,
                                                            float* __restrict__ out, unsigned char* __restrict__ mask) {
  const int t = blockIdx.x, b = blockIdx.y;
  const int e = plan[4 * b];
  const bool ok = e >= 0 && e < E;
  const int off = ok ? lang_off[e] : 0, len = ok ? min(max(lang_off[e + 1] - off, 0), Lmax) : 0;
  const bool live = t < len;
  float* o = out + ((long)b * Lmax + t) * D;
  const float* src = lang + ((long)off + t) * D;
  if (vec) {
    const float4_t zero = {0.f, 0.f, 0.f, 0.f};
    for (int i = threadIdx.x; i < D / 4; i += 64) ((float4_t*)o)[i] = live ? ((const float4_t*)src)[i] : zero;
  } else {
    for (int i = threadIdx.x; i < D; i += 64) o[i] = live ? src[i] : 0.f;
  }
  if (threadIdx.x == 0) mask[(long)b * Lmax + t] = live ? 1 : 0;
}

}  // namespace

int vt_rdt_batch(const double* qpos, const int* ep_off, const double* ep_stats, const double* ds_mean, const int* col_map, const float* lang,
                 const int* lang_off, int E, int S, int A, int H, int D, int Lmax, int ctrl_freq, double noise_div, const void* plan, int B,
                 float* states, float* actions, float* elem_mask, float* state_norm, long long* ctrl_freqs, float* lang_out,
                 unsigned char* lang_mask, vt_stream_t s) {
  if (!qpos || !ep_off || !ep_stats || !ds_mean || !col_map || !lang || !lang_off || !plan || !states || !actions || !elem_mask || !state_norm ||
      !ctrl_freqs || !lang_out || !lang_mask)
    return vt_fail(VT_ERR_ARG, "vt_rdt_batch: null pointer");
  if (E < 1 || S < 1 || A < S || H < 1 || D < 1 || Lmax < 1 || B < 1)
    return vt_fail(VT_ERR_ARG, "vt_rdt_batch: E, S, H, D, Lmax and B must be >= 1 and A >= S (got E=%d S=%d A=%d H=%d D=%d Lmax=%d B=%d)", E, S, A, H, D,
                   Lmax, B);
  if (B > 65535 || H + 3 > 65535 || Lmax > 65535) return vt_fail(VT_ERR_ARG, "vt_rdt_batch: B, H + 3 and Lmax must fit a grid dimension (65535)");
  if (!(noise_div > 0.0)) return vt_fail(VT_ERR_ARG, "vt_rdt_batch: noise_div must be > 0 (pass 1 when no sample is noised)");
  if ((uintptr_t)plan % 8) return vt_fail(VT_ERR_ARG, "vt_rdt_batch: plan must be 8-byte aligned");
  const int* hdr = (const int*)plan;
  const double* z = (const double*)((const char*)plan + (size_t)16 * B);
  hipLaunchKernelGGL(rdt_batch_rows_kernel, dim3(H + 3, B), dim3(128), 0, (hipStream_t)s, qpos, ep_off, ep_stats, ds_mean, col_map, hdr, z, E, S, A, H,
                     ctrl_freq, noise_div, states, actions, elem_mask, state_norm, ctrl_freqs);
  const int vec = D % 4 == 0 && (uintptr_t)lang % 16 == 0 && (uintptr_t)lang_out % 16 == 0;
  hipLaunchKernelGGL(rdt_batch_lang_kernel, dim3(Lmax, B), dim3(64), 0, (hipStream_t)s, lang, lang_off, hdr, E, D, Lmax, vec, lang_out, lang_mask);
  return vt_check_launch();
}
