// vt_gemm_fast.hip — the large-GEMM path: 16-bit x 16-bit -> fp32 accumulate on v_mfma_f32_16x16x32_{bf16,f16}, for every
// big Linear of RDT (bf16) and DINOv2 (IEEE fp16) (C = epilogue(A[M,K] W[N,K]^T), K % 64 == 0).
//
// Structure: BM x 128 x 64 block tile (BM = 128 or 64), 256 threads = 4 waves (2x2), each wave (BM/2) x 64 output =
// (BM/32) x 4 MFMA tiles.  Operand tiles go HBM/L2 -> LDS by DMA (`global_load_lds_dwordx4`, 16 B per lane, no VGPR
// round trip): a wave instruction fills 1 KiB = 8 rows x 128 B of the tile; the LDS image is lane-linear, so the XOR
// chunk swizzle that makes the 16-row fragment reads (ds_read_b128) bank-conflict-free is applied to the SOURCE
// address of each lane and again on the read (same involution both sides).  Two pipelining variants (picked per launch
// from the grid size, see vt_gemm_fast_launch): ONE LDS stage with 4 co-resident blocks per CU (latency hidden across
// blocks; the default whenever the grid fills the 1024 block slots) or TWO stages at 2 blocks/CU (DMA of k-tile t+1 issued
// before the MFMAs of tile t).  Blocks are dealt to XCDs in contiguous bands of tiles, and inside a band in super-rows of
// GM m-tiles, so neighbouring tiles share operand panels in that XCD's private L2 (vt_tile_of, vt_gemm_tile.h: the family's one tile order).
// Operands are swapped (D = W_tile A_tile^T) so a lane ends with 4 consecutive n of one row m.
// Epilogue: vt_gemm_epilogue.h (shared with the ping-pong kernels vt_gemm_pp.hip / vt_gemm_ppk.hip).
// Dispatch: this file launches gemm_glds_kernel only.  Which large 16-bit GEMMs land here is decided in vt_gemm_route.hip (VT_GEMM_GLDS: what
// none of the other tiles of the family claims); vt_gemm_lds_fits below is the contract of the whole family.
#include "vt_common.h"
#include "vt_gemm_route.h"
#include "vt_gemm_epilogue.h"
#include "vt_gemm_tile.h"
#include "vt_prof.h"

namespace {


constexpr int BK = 64;

// NS = LDS stages: 2 = the DMA of k-tile t+1 overlaps the MFMAs of tile t inside the block (2 blocks/CU);
//                 1 = no overlap inside a block, latency is hidden by MINW (3-4) co-resident blocks per CU instead.
// Block tile BM x BN: 2 x (BN/64) waves, each (BM/2) x 64 -> 128-col tiles run 4 waves (256 threads), 256-col tiles 8 waves.
// MINW = co-resident blocks per CU the register budget is sized for.
template <typename T16, typename TC, int BM, int BN, int NS, int MINW, int CMAP>
__global__ __launch_bounds__(2 * BN, MINW * (BN / 128)) void gemm_glds_kernel(const VtGemmParams p, const int tiles_n, const int tiles_per_group, const int total_tiles, const int GM) {
  constexpr int WN = BN / 64, NW = 2 * WN;  // waves along N, waves per block (blockDim.x = 64 * NW = 2 * BN)
  constexpr int STAGE_BYTES = (BM + BN) * 128;
  constexpr int TM = BM / 32;               // 16-row MFMA tiles per wave along M
  constexpr int QA = BM / 8 / NW;           // A-tile DMA instructions per wave (8 rows x 128 B each)
  constexpr int QB = BN / 8 / NW;           // W-tile DMA instructions per wave
  constexpr int SMEM = NS * STAGE_BYTES > NW * EP_BYTES ? NS * STAGE_BYTES : NW * EP_BYTES;   // operand stages, reused by the epilogue patches
  __shared__ __attribute__((aligned(16))) char smem[SMEM];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;
  const int g = lane >> 4, l15 = lane & 15;

  const VtTile t = vt_tile_of(blockIdx.x, total_tiles, tiles_n, tiles_per_group, GM);
  const int grp = t.grp, m0 = t.tm * BM, n0 = t.tn * BN;

  const uint16_t* A = reinterpret_cast<const uint16_t*>(p.A) + (long)grp * p.a_gs;
  const uint16_t* W = reinterpret_cast<const uint16_t*>(p.W) + (long)grp * p.w_gs;

  // DMA sources (vt_dma_src): instruction q of this wave fills 8 LDS rows
  const uint16_t* a_src[QA];
  const uint16_t* b_src[QB];
#pragma unroll
  for (int q = 0; q < QA; ++q) {
    a_src[q] = vt_dma_src(A, m0, (wave * QA + q) * 8 + (lane >> 3), p.M, p.lda, lane);
  }
#pragma unroll
  for (int q = 0; q < QB; ++q) {
    b_src[q] = vt_dma_src(W, n0, (wave * QB + q) * 8 + (lane >> 3), p.N, p.ldw, lane);
  }
  auto stage = [&](int buf, int kt) {
    char* base = smem + buf * STAGE_BYTES;
#pragma unroll
    for (int q = 0; q < QA; ++q)
      __builtin_amdgcn_global_load_lds((glb_void*)(a_src[q] + (long)kt * BK), (lds_void*)(base + (wave * QA + q) * 1024), 16, 0, 0);
#pragma unroll
    for (int q = 0; q < QB; ++q)
      __builtin_amdgcn_global_load_lds((glb_void*)(b_src[q] + (long)kt * BK), (lds_void*)(base + BM * 128 + (wave * QB + q) * 1024), 16, 0, 0);
  };

  float4_t acc[4][TM];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < TM; ++j) acc[i][j] = (float4_t){0.f, 0.f, 0.f, 0.f};

  const int nk = p.K / BK;
  if constexpr (NS == 2) {
    stage(0, 0);
    __syncthreads();        // drains the DMA (vmcnt) and publishes stage 0
  }
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = NS == 2 ? (kt & 1) : 0;
    if constexpr (NS == 2) {
      if (kt + 1 < nk) stage(cur ^ 1, kt + 1);
    } else {
      stage(0, kt);
      __syncthreads();      // tile landed
    }
    const char* As = smem + cur * STAGE_BYTES;
    const char* Bs = As + BM * 128;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      Frag<T16> af[TM], wf[4];
#pragma unroll
      for (int j = 0; j < TM; ++j) lds_frag(af[j], As, wm * (BM / 2) + j * 16 + l15, ks * 4 + g);
#pragma unroll
      for (int i = 0; i < 4; ++i) lds_frag(wf[i], Bs, wn * 64 + i * 16 + l15, ks * 4 + g);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < TM; ++j) mma16(acc[i][j], wf[i], af[j]);
    }
    __syncthreads();        // next stage landed (vmcnt(0) inside) and everyone is done reading `cur`
  }

  // ---------------- epilogue (vt_gemm_epilogue.h); the stages are reused as the waves' private patches
  vt_gemm_epilogue<TC, TM, CMAP>(p, acc, reinterpret_cast<float*>(smem + wave * EP_BYTES), grp, m0 + wm * (BM / 2), n0 + wn * 64, lane);
}

}  // namespace

// what the LDS-DMA family (this kernel and the tiles of vt_gemm_pp / pt / ppk / pw.hip) computes, and the smallest grid worth its pipeline
bool vt_gemm_lds_fits(const VtGemmParams& p) {
  if ((p.a_dtype != VT_BF16 && p.a_dtype != VT_F16) || p.w_dtype != p.a_dtype || p.taps != 0 || p.splitk != 1) return false;
  if (p.c_dtype != p.a_dtype && p.c_dtype != VT_F32) return false;
  if (p.K % BK || p.lda % 8 || p.ldw % 8 || p.N % 4 || p.ldc % 4 || (p.residual && p.ldr % 4)) return false;
  if (p.M < 128) return false;
  if (p.cmap && ((p.a_dtype != VT_BF16 && !(p.a_dtype == VT_F16 && p.cmap == 3)) || p.c_dtype == VT_F32 || p.N % 64 || p.residual || p.groups != 1 || (long)p.cmap_T * 64 < p.M)) return false;
  if (p.cmap == 3 && (p.N % 128)) return false;      // fused K|V: two halves of whole heads
  return vt_tile_count(p, 128, 128) >= 96;
}

bool vt_gemm_can_fuse_headnorm(const VtGemmParams& p) { return vt_gemm_lds_fits(p) && (p.N % 64) == 0; }

template <typename T16, typename TC, int BM, int CMAP>
static void launch_variant(int variant, dim3 grid, hipStream_t s, const VtGemmParams& p, int tiles_n, int per_group, int total) {
  // super-row height (measured): tall-skinny outputs (few n-tiles, many m-tiles: the condition K/V projections) like 16,
  // everything else 4
  const int gm = (tiles_n <= 16 && per_group / tiles_n >= 128) ? 16 : 4;
  if (variant == 14) hipLaunchKernelGGL((gemm_glds_kernel<T16, TC, BM, 128, 1, 4, CMAP>), grid, dim3(256), 0, s, p, tiles_n, per_group, total, gm);
  else hipLaunchKernelGGL((gemm_glds_kernel<T16, TC, BM, 128, 2, 2, CMAP>), grid, dim3(256), 0, s, p, tiles_n, per_group, total, gm);
}

int vt_gemm_fast_launch(const VtGemmParams& p, hipStream_t s) {
  const long tiles128 = vt_tile_count(p, 128, 128);
  // Measured on MI355X (tools/gemm_bench.py).  128-column tiles: one LDS stage with 4 co-resident blocks per CU (1024 block
  // slots) beats in-block double buffering at 2 blocks/CU on every shape of this path (cond-K/V 561 -> 854 TF/s, K=768 DINOv2
  // GEMMs 330 -> 490) except when the grid cannot fill the slots, where the two-stage kernel hides latency inside the block;
  // 128-row tiles when they fill the slots, else 64-row tiles.
  const int bm = tiles128 < 1024 ? 64 : 128;
  const VtTiles t = vt_tiles(p, bm, 128);
  const int variant = t.total < 768 ? 22 : 14;   // 22 = two stages, 2 blocks/CU; 14 = one stage, 4 blocks/CU
  VtProfScope prof(3, p, s);
#define VT_FAST_GO(T16, TC, BMv, CM) launch_variant<T16, TC, BMv, CM>(variant, dim3(t.total), s, p, t.n, t.per_group, t.total)
#define VT_FAST_GO3(T16, TC) \
  { if (bm == 128) VT_FAST_GO(T16, TC, 128, 0); else VT_FAST_GO(T16, TC, 64, 0); }
#define VT_FAST_GO_CMAP(BMv) \
  { if (p.a_dtype == VT_F16) VT_FAST_GO(half_t, half_t, BMv, 3);      /* fp16: the fused K|V form only */ \
    else if (p.cmap == 1) VT_FAST_GO(bf16_t, bf16_t, BMv, 1); \
    else if (p.cmap == 2) VT_FAST_GO(bf16_t, bf16_t, BMv, 2); \
    else VT_FAST_GO(bf16_t, bf16_t, BMv, 3); }
  if (p.cmap) {
    if (bm == 128) VT_FAST_GO_CMAP(128) else VT_FAST_GO_CMAP(64)
  } else {
    VT_DISPATCH_T16_TC(p, T16, TC, VT_FAST_GO3(T16, TC))
  }
#undef VT_FAST_GO
#undef VT_FAST_GO3
#undef VT_FAST_GO_CMAP
  return vt_check_launch();
}
