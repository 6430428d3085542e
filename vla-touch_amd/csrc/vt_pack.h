// vt_pack.h — the MFMA fragment order of the packed-weight GEMM tiles (vt_gemm_pw.hip, vt_gemm_pws.hip), stated once for the kernels that write
// it: pack_w32_kernel (vt_gemm_pw.hip: the load-time packing of frozen weights) and refresh16_kernel (vt_refresh16.hip: the trainer's refresh).
//
// A 16-bit matrix [R][Cn] (R % 32 == 0, Cn % 16 == 0) is stored as [R / 32][Cn / 16][64 lanes][8 elements]: one 1-KiB fragment per 32 rows x 16
// columns; lane = (column half of 8) * 32 + (row in the band of 32), and a lane's 8 elements are 8 consecutive columns.  The unit that moves is
// therefore the 16-byte chunk (row r, columns 8 c8 .. 8 c8 + 7), the same bytes as a 16-byte chunk of the row-major matrix.
#pragma once

// the shapes the layout exists for (vt_pack_w32's argument check, and what vt_refresh16 accepts for a packed output)
static inline bool vt_pack_w32_shape_ok(int R, int Cn) { return R > 0 && Cn > 0 && R % 32 == 0 && Cn % 16 == 0; }

// element offset, in the packed copy of [R][Cn], of the chunk (row r, columns 8 c8 .. + 7)
__host__ __device__ __forceinline__ long vt_pack_w32_chunk(int r, int c8, int Cn) {
  return ((((long)(r >> 5) * (Cn >> 4) + (c8 >> 1)) * 64) + (c8 & 1) * 32 + (r & 31)) * 8;
}
