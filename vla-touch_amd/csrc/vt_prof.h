// vt_prof.h — live per-launch timing of the LDS-DMA GEMM kernels (bench.py's roofline leg): while enabled, every launch of
// the selected kernel class is bracketed by HIP events recorded on its launch stream.
//   vt_prof_enable(0) off; (1) every GEMM class; (2) only the 256-square tiles (gemm_pp256d_kernel, gemm_pt_kernel: vt_gemm_pp.hip,
//   vt_gemm_pt.hip); (3) only the 128- / 160-column tiles (vt_gemm_fast.hip, vt_gemm_ppk.hip, vt_gemm_pw.hip, vt_gemm_pws.hip);
//   (4) only the cached cross-attention (vt_attn_kvt.hip); (5) only the register-staged GEMMs (vt_gemm.hip, vt_gemm_f32r.hip);
//   (6) only the fused U-Net convolution (vt_uconv.hip)
// A launcher opens a VtProfScope around its launch; the state and vt_prof_enable / vt_prof_collect are defined in vt_api.hip.  Profiling only: which kernel
// takes a launch is vt_gemm_route.h's business.
#pragma once
#include <hip/hip_runtime.h>
#include "vt_common.h"
#include "vt_gemm.h"

struct VtProfState {
  bool on = false;
  int mode = 1;
  static constexpr int MAXEV = 8192;
  hipEvent_t ev[2 * MAXEV];
  int created = 0, used = 0;
  double flops = 0.0, bytes = 0.0;
};
extern VtProfState g_vt_prof;

struct VtProfScope {
  bool active; hipStream_t s; int idx;
  VtProfScope(int cls, const VtGemmParams& p, hipStream_t st) : active(g_vt_prof.on && (g_vt_prof.mode == 1 || g_vt_prof.mode == cls) && g_vt_prof.used < VtProfState::MAXEV), s(st), idx(0) {
    if (!active) return;
    idx = g_vt_prof.used++;
    while (g_vt_prof.created < 2 * (idx + 1)) (void)hipEventCreate(&g_vt_prof.ev[g_vt_prof.created++]);
    g_vt_prof.flops += 2.0 * p.M * (double)p.N * p.K * p.groups;
    g_vt_prof.bytes += ((double)p.M * p.K + (double)p.N * p.K) * 2.0 * p.groups + (double)p.M * p.N * p.groups * (p.c_dtype == VT_F32 ? 4.0 : 2.0);
    (void)hipEventRecord(g_vt_prof.ev[2 * idx], s);
  }
  // a kernel that is not a GEMM: the caller states its algorithmic flops / bytes (class 4 = cached cross-attention, HBM-bound)
  VtProfScope(int cls, double flops, double bytes, hipStream_t st) : active(g_vt_prof.on && g_vt_prof.mode == cls && g_vt_prof.used < VtProfState::MAXEV), s(st), idx(0) {
    if (!active) return;
    idx = g_vt_prof.used++;
    while (g_vt_prof.created < 2 * (idx + 1)) (void)hipEventCreate(&g_vt_prof.ev[g_vt_prof.created++]);
    g_vt_prof.flops += flops; g_vt_prof.bytes += bytes;
    (void)hipEventRecord(g_vt_prof.ev[2 * idx], s);
  }
  ~VtProfScope() { if (active) (void)hipEventRecord(g_vt_prof.ev[2 * idx + 1], s); }
};
