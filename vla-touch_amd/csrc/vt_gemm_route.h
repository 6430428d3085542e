// vt_gemm_route.h — which kernel takes a GEMM launch.  vt_gemm_route() (vt_gemm_route.hip) is the ONE place that decides; the kernel files
// only say what their kernel can compute (vt_gemm_*_fits) and launch it (vt_gemm_*_launch: each launches its own kernel and nothing else).
#pragma once
#include <hip/hip_runtime.h>
#include "vt_gemm.h"

// Codes are part of the C ABI (include/vlatouch.h, vt_gemm_route_of: VT_ROUTE_*).
enum VtGemmRoute : int {
  VT_GEMM_UNSUPPORTED = 0,   // no kernel takes this block (vt_gemm_launch returns VT_ERR_UNSUPPORTED)
  VT_GEMM_BAD_ARG = 1,       // sizes / alignment rejected (VT_ERR_ARG)
  VT_GEMM_REG = 2,           // register-staged gemm_kernel                      vt_gemm.hip
  VT_GEMM_F32R = 3,          // exact-fp32 LDS-DMA ring                          vt_gemm_f32r.hip
  VT_GEMM_GLDS = 4,          // 128-column LDS-DMA tile                          vt_gemm_fast.hip
  VT_GEMM_PP = 5,            // 256-square ping-pong tile                        vt_gemm_pp.hip
  VT_GEMM_PT = 6,            // the same tile, persistent                        vt_gemm_pt.hip
  VT_GEMM_PPK = 7,           // 160 x 128 tile, in-block split-K                 vt_gemm_ppk.hip
  VT_GEMM_PW = 8,            // 160 x 128 tile, weights in registers             vt_gemm_pw.hip
  VT_GEMM_PWS = 9,           // small-M packed tile                              vt_gemm_pws.hip
  VT_GEMM_ROWSPLIT = 10,     // two launches: full 256-row blocks on the 256-square family + the <= 64 remaining rows (vt_gemm_rowsplit)
};

// The decision, in the order vt_gemm_launch has always evaluated it.  Pure host code: no HIP call, no launch.
VtGemmRoute vt_gemm_route(const VtGemmParams& p);
// The two launches of a VT_GEMM_ROWSPLIT block: `head` = the full 256-row blocks, which go STRAIGHT to the 256-square family (the return value,
// VT_GEMM_PT or VT_GEMM_PP: head is not routed afresh — with its other M the weights-in-registers tile could claim it); `tail` = the remaining rows,
// an ordinary launch of its own (vt_gemm_route(tail)).
VtGemmRoute vt_gemm_rowsplit(const VtGemmParams& p, VtGemmParams& head, VtGemmParams& tail);
void vt_gemm_route_tune(int knob, int value);   // vt_tune(2, .): weights-in-registers tile on / off; vt_tune(8, .): persistent tile on / off (-> VT_GEMM_PP)

// What each kernel can compute (and, where its tile sizes say so, the grids it is good at).  vt_gemm_lds_fits is the contract of the whole LDS-DMA family
// (GLDS / PP / PT / PPK / PW: 16-bit operands, K % 64, M >= 128, >= 96 tiles of 128 x 128); the other predicates of that family assume it holds.
bool vt_gemm_lds_fits(const VtGemmParams& p);              // vt_gemm_fast.hip
bool vt_gemm_can_fuse_headnorm(const VtGemmParams& p);     // vt_gemm_fast.hip: the family's fused per-head RMSNorm epilogue is available
bool vt_gemm_pp_fits(const VtGemmParams& p);               // vt_gemm_pp.hip: one well-filled round or >= 2 rounds of 256-square tiles
bool vt_gemm_pt_fits(const VtGemmParams& p);               // vt_gemm_pt.hip: the epilogue kinds the persistent kernel has
bool vt_gemm_pt_one_round(const VtGemmParams& p);          // vt_gemm_pt.hip: pt_fits and one round of 160 .. 256 tiles at K >= 512, which only the persistent kernel takes
bool vt_gemm_ppk_fits(const VtGemmParams& p);              // vt_gemm_ppk.hip: one round of 160 x 128 tiles
bool vt_gemm_pw_fits(const VtGemmParams& p);               // vt_gemm_pw.hip: packed weights, full rounds of 160 x 128 tiles
bool vt_gemm_pws_fits(const VtGemmParams& p);              // vt_gemm_pws.hip: packed weights, M <= 512 (does not need vt_gemm_lds_fits)
bool vt_gemm_f32r_fits(const VtGemmParams& p);             // vt_gemm_f32r.hip: exact fp32, fewer than 1024 tiles of 128 x 128

int vt_gemm_reg_launch(const VtGemmParams& p, hipStream_t s);    // gemm_kernel; VT_ERR_UNSUPPORTED for a dtype triple it has no instance of
int vt_gemm_f32r_launch(const VtGemmParams& p, hipStream_t s);   // gemm_f32r_kernel
int vt_gemm_fast_launch(const VtGemmParams& p, hipStream_t s);   // gemm_glds_kernel
int vt_gemm_pp_launch(const VtGemmParams& p, hipStream_t s);     // gemm_pp256d_kernel
int vt_gemm_pt_launch(const VtGemmParams& p, hipStream_t s);     // gemm_pt_kernel
int vt_gemm_ppk_launch(const VtGemmParams& p, hipStream_t s);    // gemm_ppk_kernel
int vt_gemm_pw_launch(const VtGemmParams& p, hipStream_t s);     // gemm_pw_kernel
int vt_gemm_pws_launch(const VtGemmParams& p, hipStream_t s);    // gemm_pws_kernel

// What the launchers of the 16-bit tiles share.  Template arguments from the block's types: the statement is compiled once per case with T16 = the
// operand type (a_dtype: VT_BF16, else IEEE half; the router admits nothing else here) and, in the second form, TC = T16 or float (fp32 C).
// (bf16_t, half_t and the dtype codes are vt_common.h's, which every launcher includes ahead of this file.)
#define VT_DISPATCH_A16(p, T16, ...) \
  if ((p).a_dtype == VT_BF16) { using T16 = bf16_t; __VA_ARGS__; } else { using T16 = half_t; __VA_ARGS__; }
#define VT_DISPATCH_T16_TC(p, T16, TC, ...) \
  VT_DISPATCH_A16(p, T16, if ((p).c_dtype != VT_F32) { using TC = T16; __VA_ARGS__; } else { using TC = float; __VA_ARGS__; })
// BM x BN tiles over the output: of all groups (of one group: groups = false) for the *_fits predicates, and as a launcher passes them to its kernel
inline long vt_tile_count(const VtGemmParams& p, int BM, int BN, bool groups = true) {
  return (long)((p.M + BM - 1) / BM) * ((p.N + BN - 1) / BN) * (groups ? p.groups : 1);
}
struct VtTiles { int n, m, per_group, total; };
inline VtTiles vt_tiles(const VtGemmParams& p, int BM, int BN) {
  VtTiles t;
  t.n = (p.N + BN - 1) / BN; t.m = (p.M + BM - 1) / BM;
  t.per_group = t.n * t.m; t.total = t.per_group * p.groups;
  return t;
}
// the 256-square tiles (PP, PT) address a 256-row block of A / W through a buffer resource with 32-bit byte offsets
inline bool vt_gemm_sq256_offsets_fit(const VtGemmParams& p) { return p.lda < (1 << 21) && p.ldw < (1 << 21) && p.K < (1 << 24); }

// launch details, not routing
void vt_gemm_pw_tune(int ring);                            // vt_tune(1, .): ring depth 4 | 8, 0 = default
void vt_gemm_pws_tune(int split);                          // vt_tune(4, .): split factor (0 = none, -1 = choose)
