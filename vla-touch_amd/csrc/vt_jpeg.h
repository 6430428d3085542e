// vt_jpeg.h — what the two JPEG translation units share (vt_jpegmap.hip: the pixel mapping of a round trip; vt_jpegdec.hip: the decoder of
// stored files), stated once: libjpeg's islow inverse DCT pass (jidctint.c) with the odd part it shares with jfdctint.c, the decoded-plane
// layout of a 4:2:0 frame, the YCbCr -> RGB conversion (jdcolor.c) and the fancy h2v2 up-sampling + conversion item (jdsample.c).  int32
// arithmetic throughout.
#pragma once
#include <stdint.h>
#include "vt_pixel.h"

constexpr int kJpegHalf = 32768;       // ONE_HALF of the 16-bit fixed-point colour conversions
constexpr int kJpegMaxSide = 32768;    // the largest frame side the drivers take
constexpr int kJpegSwapRB = 1;         // flag bit of the conversions: channel 0 of the array plays blue's role (VT_JPEGMAP_CV2_ORDER)

__device__ __forceinline__ int descale(const int x, const int n) { return (x + (1 << (n - 1))) >> n; }

// the odd part that jfdctint and jidctint share: (t4, t5, t6, t7) -> the sums of out7 / 5 / 3 / 1 (forward) or tmp0..3 (inverse)
__device__ __forceinline__ void odd_part(int& t4, int& t5, int& t6, int& t7) {
  int z1 = t4 + t7, z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const int z5 = (z3 + z4) * 9633;
  t4 *= 2446; t5 *= 16819; t6 *= 25172; t7 *= 12299;
  z1 *= -7373; z2 *= -20995; z3 = z3 * -16069 + z5; z4 = z4 * -3196 + z5;
  t4 += z1 + z3; t5 += z2 + z4; t6 += z2 + z3; t7 += z1 + z4;
}

// one pass of jidctint on c[0..8), descaled by N bits
template <int N> __device__ __forceinline__ void idct8(int c[8]) {
  const int z1 = (c[2] + c[6]) * 4433;
  const int t2 = z1 - c[6] * 15137, t3 = z1 + c[2] * 6270;
  const int t0 = (c[0] + c[4]) << 13, t1 = (c[0] - c[4]) << 13;
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  int o0 = c[7], o1 = c[5], o2 = c[3], o3 = c[1];
  odd_part(o0, o1, o2, o3);
  c[0] = descale(t10 + o3, N); c[7] = descale(t10 - o3, N);
  c[1] = descale(t11 + o2, N); c[6] = descale(t11 - o2, N);
  c[2] = descale(t12 + o1, N); c[5] = descale(t12 - o1, N);
  c[3] = descale(t13 + o0, N); c[4] = descale(t13 - o0, N);
}

// the decoded planes of a 4:2:0 frame: Y' [H16][W16], Cb' and Cr' [H16 / 2][W16 / 2] of the frame padded to whole 16 x 16 MCUs
struct PlaneGeom {
  int H16, W16;       // the frame padded to whole MCUs
  long cb, cr;        // byte offsets of the chroma planes behind the frame's ws_off
};
__host__ __device__ inline PlaneGeom plane_geom(const int h, const int w) {
  PlaneGeom g;
  g.H16 = (h + 15) & ~15; g.W16 = (w + 15) & ~15;
  g.cb = (long)g.H16 * g.W16;
  g.cr = g.cb + g.cb / 4;
  return g;
}

// jdcolor.c: (Y, Cb - 128, Cr - 128) -> r | g << 8 | b << 16 (red and blue swapped under kJpegSwapRB)
__device__ __forceinline__ uint32_t ycc_px(const int Y, const int cb, const int cr, const int flags) {
  int R = clip8(Y + ((91881 * cr + kJpegHalf) >> 16));
  const int G = clip8(Y + ((-22554 * cb + kJpegHalf - 46802 * cr) >> 16));
  int B = clip8(Y + ((116130 * cb + kJpegHalf) >> 16));
  if (flags & kJpegSwapRB) { const int t = R; R = B; B = t; }
  return (uint32_t)R | ((uint32_t)G << 8) | ((uint32_t)B << 16);
}

// items of the up-sampling launch of an h x w frame: one item = 2 rows x 4 columns of the output
__host__ __device__ inline long jpeg_upsample_items(const int h, const int w) { return (long)((h + 1) >> 1) * ((((w + 1) >> 1) + 1) >> 1); }

// item `it` of a 4:2:0 frame whose decoded planes lie at `base` (plane_geom layout): Y', the clamped 3 x 4 neighbourhood of Cb' and Cr', the
// triangle filter, the conversion, 12 bytes per row to the tight h x w x 3 frame at `outp`
__device__ __forceinline__ void jpeg_upsample_item(const uint8_t* __restrict__ base, const int h, const int w, const int flags, const long it,
                                                   uint8_t* __restrict__ outp) {
  const PlaneGeom g = plane_geom(h, w);
  const int ch = (h + 1) >> 1, cw = (w + 1) >> 1;
  const int ipr = (cw + 1) >> 1;                     // items per chroma row: two chroma columns = four pixels each
  if (it >= (long)ch * ipr) return;
  const int j = (int)(it / ipr), i0 = (int)(it - (long)j * ipr) * 2;
  const int cpitch = g.W16 >> 1;
  const bool fancy = cw > 2;                         // jdsample.c: narrower components are replicated
  const int jr[3] = {max(j - 1, 0), j, min(j + 1, ch - 1)};
  int up[2][2][4];                                   // [Cb | Cr][row 2j + v][column 2 i0 + k]
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const uint8_t* pl = base + (c ? g.cr : g.cb);
    int C[3][4];                                     // rows j - 1, j, j + 1; columns i0 - 1 .. i0 + 2, all clamped into the ch x cw component
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int k = 0; k < 4; ++k) C[r][k] = pl[(long)jr[r] * cpitch + min(max(i0 - 1 + k, 0), cw - 1)];
#pragma unroll
    for (int v = 0; v < 2; ++v) {
      int s[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) s[k] = 3 * C[1][k] + C[v ? 2 : 0][k];
#pragma unroll
      for (int q = 0; q < 2; ++q) {                  // chroma column i0 + q sits at C[.][q + 1]
        up[c][v][2 * q] = fancy ? (3 * s[q + 1] + s[q] + 8) >> 4 : C[1][q + 1];
        up[c][v][2 * q + 1] = fancy ? (3 * s[q + 1] + s[q + 2] + 7) >> 4 : C[1][q + 1];
      }
    }
  }
  const int x0 = i0 * 2, npx = min(4, w - x0);
#pragma unroll
  for (int v = 0; v < 2; ++v) {
    const int y = 2 * j + v;
    if (y >= h) break;
    const uint32_t yw = *(const uint32_t*)(base + (long)y * g.W16 + x0);      // x0 is a multiple of 4 inside the padded plane
    uint32_t px[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) px[k] = ycc_px((yw >> (8 * k)) & 255, up[0][v][k] - 128, up[1][v][k] - 128, flags);
    store_px4(outp + ((long)y * w + x0) * 3, px, npx);
  }
}
