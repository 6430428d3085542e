// vt_gemm_route.hip — the GEMM dispatch policy: vt_gemm_route() decides which of the nine kernels takes a parameter block, vt_gemm_launch() runs
// that decision.  Drivers that plan around a kernel (the RMSNorm hand-off and the prefetch hint of vt_rdt.hip, DINO's fc1 in vt_models.hip) and the
// tests (vt_gemm_route_of, include/vlatouch.h) ask the same function; nothing else in the library chooses a GEMM kernel.
//
// Order of the decision (first match wins):
//   1. argument checks                                                                   -> BAD_ARG
//   2. RMSNorm hand-off fields set (xn_out / rs_part): only the weights-in-registers tile has them  -> PW, else UNSUPPORTED
//   3. packed weights and (M <= 192 or outside the LDS-DMA family)                       -> PWS
//   4. inside the LDS-DMA family (vt_gemm_lds_fits):  PW;  ROWSPLIT;  PT / PP;  PPK;  GLDS
//   5. head norm / tile-stream output requested outside that family                      -> UNSUPPORTED
//   6. 16-bit (and fp32 x bf16) products                                                 -> REG
//   7. exact fp32 / split-bf16 with few blocks per CU                                    -> F32R
//   8. fp32, split-bf16                                                                  -> REG
#include "vt_common.h"
#include "vt_gemm_route.h"
#include "vt_kernels.h"

static int g_pw_on = 1;      // vt_tune(2, 0): nothing routes to PW (A/B against gemm_ppk_kernel / gemm_pp256d_kernel)
static int g_pt_on = 1;      // vt_tune(8, 0): every PT becomes PP

void vt_gemm_route_tune(int knob, int value) { (knob == 2 ? g_pw_on : g_pt_on) = value != 0; }

// p runs on the 256-square family (p inside the LDS-DMA family): the shapes gemm_pp256d_kernel is good at, plus the one-round shapes of the persistent kernel
static bool sq256(const VtGemmParams& p) { return vt_gemm_pp_fits(p) || (g_pt_on && vt_gemm_pt_one_round(p)); }
static VtGemmRoute sq256_route(const VtGemmParams& p) { return g_pt_on && vt_gemm_pt_fits(p) ? VT_GEMM_PT : VT_GEMM_PP; }

// A ragged last row block that costs a whole extra round of 256-square tiles (DINOv2-base: 64 images x 257 tokens = 64 x 256 + 64 rows; fc1's
// 65 x 12 = 780 tiles are 3.05 rounds of the 256 CUs): the full row blocks go to the 256-square family, the <= 64 remaining rows to a second small
// launch (rows are independent: an exact row split).  Returns the number of rows of the head, 0 = no split.
static int rowsplit_rows(const VtGemmParams& p) {
  if (p.cmap != 0 || p.groups != 1 || p.hn_w0 || p.hn_w1 || p.M % 256 == 0 || p.M % 256 > 64 || !sq256(p)) return 0;
  const long tm = (p.M + 255) / 256, tn = (p.N + 255) / 256;
  if (tm <= 1 || (tm * tn + 255) / 256 <= ((tm - 1) * tn + 255) / 256) return 0;
  VtGemmParams a = p;
  a.M = (int)((tm - 1) * 256);
  return vt_gemm_lds_fits(a) && sq256(a) ? a.M : 0;
}

VtGemmRoute vt_gemm_rowsplit(const VtGemmParams& p, VtGemmParams& head, VtGemmParams& tail) {
  head = p; tail = p;
  head.M = rowsplit_rows(p);
  const size_t ea = p.a_dtype == VT_F32 ? 4 : 2, ec = p.c_dtype == VT_F32 ? 4 : 2;
  tail.M = p.M - head.M;
  tail.A = (const char*)p.A + (size_t)head.M * p.lda * ea;
  tail.C = (char*)p.C + (size_t)head.M * p.ldc * ec;
  if (p.residual) tail.residual = (const char*)p.residual + (size_t)head.M * p.ldr * ec;
  return sq256_route(head);
}

VtGemmRoute vt_gemm_route(const VtGemmParams& p) {
  // 1. arguments
  if (p.M <= 0 || p.N <= 0 || p.K <= 0) return VT_GEMM_BAD_ARG;
  const int epc = p.w_dtype == VT_F32 ? 4 : 8;   // k elements per staged 16-B chunk (bf16 and split-bf16: 8); A chunks are loaded in units of the compute type's chunk
  if (p.K % epc || p.ldw % epc || p.lda % epc) return VT_GEMM_BAD_ARG;
  if (p.taps && (p.cin % epc || p.K != p.taps * p.cin)) return VT_GEMM_BAD_ARG;
  if (p.splitk < 1 || p.groups < 1) return VT_GEMM_BAD_ARG;
  if (p.splitk > 1 && p.c_dtype != VT_F32) return VT_GEMM_BAD_ARG;
  if (p.pf_ptr && p.pf_bytes >= (1ul << 31)) return VT_GEMM_BAD_ARG;      // prefetch hint: 32-bit byte arithmetic in the kernel
  const bool hn = p.hn_w0 || p.hn_w1;
  const bool lds = vt_gemm_lds_fits(p);
  const bool pw = lds && g_pw_on && vt_gemm_pw_fits(p);
  // 2. fused RMSNorm hand-off: only the weights-in-registers tile implements it
  if (p.xn_out || p.rs_part) {
    if (p.groups != 1 || (p.xn_out && (!p.xn_gain || !p.xn_part || p.c_dtype != VT_F32 || !p.residual || p.act != VT_ACT_NONE || hn || p.xn_ld % 4)) ||
        (p.rs_part && (p.rs_n < 4 || p.rs_n > 32 || p.rs_n % 4)) || !pw)
      return VT_GEMM_UNSUPPORTED;
    return VT_GEMM_PW;
  }
  // 3. small M, frozen packed weights
  if (vt_gemm_pws_fits(p) && (p.M <= 192 || !lds)) return VT_GEMM_PWS;
  // 4. large 16-bit GEMMs: the LDS-DMA family
  if (lds) {
    if (pw) return VT_GEMM_PW;                           // frozen, fragment-packed weights: W never touches LDS
    if (rowsplit_rows(p)) return VT_GEMM_ROWSPLIT;
    if (sq256(p)) return sq256_route(p);                 // several rounds of 256-square tiles: half the L2 -> LDS bytes per flop of the 128-column tile
    if (vt_gemm_ppk_fits(p)) return VT_GEMM_PPK;
    return VT_GEMM_GLDS;
  }
  // 5. fused head-norm / tile-stream output exist only in that family
  if (hn || p.cmap) return VT_GEMM_UNSUPPORTED;
  // 6. register-staged 16-bit products
  const int a = p.a_dtype, w = p.w_dtype, c = p.c_dtype;
  if (a == VT_BF16 && w == VT_BF16) return c == VT_BF16 || c == VT_F32 ? VT_GEMM_REG : VT_GEMM_UNSUPPORTED;
  if (a == VT_F16 && w == VT_F16) return c == VT_F16 || c == VT_F32 ? VT_GEMM_REG : VT_GEMM_UNSUPPORTED;
  if (a == VT_F32 && w == VT_BF16) return VT_GEMM_REG;
  // 7. exact fp32, few blocks per CU: LDS-DMA ring
  if (vt_gemm_f32r_fits(p)) return VT_GEMM_F32R;
  // 8. exact fp32 and split-bf16 on the register-staged kernel
  if (a == VT_F32 && (w == VT_F32 || w == VT_F32X3) && c == VT_F32) return VT_GEMM_REG;
  return VT_GEMM_UNSUPPORTED;
}

// Host entry used by every driver in the library (and exported through vt_gemm in vt_api.hip).
int vt_gemm_launch(const VtGemmParams& p, hipStream_t s) {
  switch (vt_gemm_route(p)) {
    case VT_GEMM_BAD_ARG: return VT_ERR_ARG;
    case VT_GEMM_UNSUPPORTED: return VT_ERR_UNSUPPORTED;
    case VT_GEMM_REG: return vt_gemm_reg_launch(p, s);
    case VT_GEMM_F32R: return vt_gemm_f32r_launch(p, s);
    case VT_GEMM_GLDS: return vt_gemm_fast_launch(p, s);
    case VT_GEMM_PP: return vt_gemm_pp_launch(p, s);
    case VT_GEMM_PT: return vt_gemm_pt_launch(p, s);
    case VT_GEMM_PPK: return vt_gemm_ppk_launch(p, s);
    case VT_GEMM_PW: return vt_gemm_pw_launch(p, s);
    case VT_GEMM_PWS: return vt_gemm_pws_launch(p, s);
    case VT_GEMM_ROWSPLIT: {
      VtGemmParams head, tail;
      const int rc = vt_gemm_rowsplit(p, head, tail) == VT_GEMM_PT ? vt_gemm_pt_launch(head, s) : vt_gemm_pp_launch(head, s);
      return rc != VT_OK ? rc : vt_gemm_launch(tail, s);
    }
  }
  return VT_ERR_UNSUPPORTED;
}
