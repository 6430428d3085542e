// vt_gemm_tile.h — what the tiles of the LDS-DMA GEMM family (vt_gemm_fast / pp / pt / ppk / pw / pws / f32r.hip) share on the device, stated once:
// the block -> tile order, the swizzled and row-clamped source of an LDS-DMA piece, and the weight loads of a k-tile of the two packed-weights tiles.  Included by the family's kernel files only.
// A helper is used where it leaves the kernel's device code as it was (tools/isa_diff.sh is the referee); DESIGN.md names the kernels that keep
// their own spelling of one.
#pragma once
#include "vt_common.h"

// ---------------------------------------------------------------------------------------------------------------- block -> tile
// Tile order inside a group: super-rows of GM m-tiles; within a super-row n advances slowly and m fastest, so GM consecutive blocks share one
// W tile and the GM A panels stay L2-resident across all n (W is re-read tiles_m/GM times instead of tiles_m times; PMC FETCH showed 2.5x the
// algorithmic bytes with the plain n-fastest order).  The last super-row may hold fewer than GM m-tiles.
struct VtTileMN { int tm, tn; };
__device__ __forceinline__ VtTileMN vt_tile_mn(const int t_in, const int tiles_m, const int tiles_n, const int GM) {
  const int sr = t_in / (GM * tiles_n);
  const int gmr = min(GM, tiles_m - sr * GM);
  const int r_in = t_in - sr * GM * tiles_n;
  const int tn = r_in / gmr;
  return VtTileMN{sr * GM + (r_in - tn * gmr), tn};
}
// Block `bid` of a launch of total_tiles = groups x tiles_per_group blocks.  Blocks are dealt round-robin to the 8 XCDs, each with a private L2:
// XCD b % 8 gets a contiguous band of the order above (when the tile count divides by 8), so neighbouring tiles share operand panels in one L2.
struct VtTile { int grp, tm, tn; };
__device__ __forceinline__ VtTile vt_tile_of(int bid, const int total_tiles, const int tiles_n, const int tiles_per_group, const int GM) {
  if ((total_tiles & 7) == 0) bid = (bid & 7) * (total_tiles >> 3) + (bid >> 3);
  const int grp = bid / tiles_per_group;
  const VtTileMN t = vt_tile_mn(bid - grp * tiles_per_group, tiles_per_group / tiles_n, tiles_n, GM);
  return VtTile{grp, t.tm, t.tn};
}

// ---------------------------------------------------------------------------------------------------------------- LDS-DMA piece source
// A piece = one wave instruction = 8 tile rows x 128 B, lane -> (row r = piece row + lane / 8, chunk position lane & 7).  The LDS image is
// lane-linear, so the lane fetches the chunk whose swizzled position is its own (swz of vt_common.h, the involution the fragment reads apply
// again); tile rows beyond the matrix are clamped to its last row (computed, never stored).
__device__ __forceinline__ int vt_dma_chunk(const int r, const int lane) { return swz(r, lane & 7); }
// pointer form (global_load_lds): row r of the tile whose first row is r0, `rows` rows of `ld` elements in the matrix
template <typename T>
__device__ __forceinline__ const T* vt_dma_src(const T* base, const int r0, const int r, const int rows, const long ld, const int lane) {
  const int c = vt_dma_chunk(r, lane);
  return base + (long)min(r0 + r, rows - 1) * ld + c * (16 / (int)sizeof(T));
}
// byte-offset form (buffer resource based at row r0 of a 16-bit matrix); c = vt_dma_chunk(r, lane), taken by the caller first: the 256-square
// kernels choose between their A and W operands per piece, and hipcc's code for them depends on the chunk being computed ahead of that choice
__device__ __forceinline__ int vt_dma_off(const int r0, const int r, const int rows, const long ld, const int c) {
  return (int)(((long)(min(r0 + r, rows - 1) - r0) * ld + c * 8) * 2);
}

// ---------------------------------------------------------------------------------------------------------------- packed-weights tiles
// gemm_pw_kernel and gemm_pws_kernel: the four weight fragments (4 KiB, back to back at sb) of one k-tile -> w[O] .. w[O + 3]
template <int O, int N>
__device__ __forceinline__ void vt_pw_wload4(int4_t (&w)[N], const unsigned voff, const char* sb) {
  wload<0, true>(w[O], voff, sb);
  wload<1024, false>(w[O + 1], voff, sb);
  wload<2048, false>(w[O + 2], voff, sb);
  wload<3072, false>(w[O + 3], voff, sb);
}
