// vt_jpegmap.hip — the pixel mapping of a baseline JPEG round trip (residual_controller/frank_inference_eef.py:84-87,
// data/create_controller_dataset_episode.py:54-62: cv2.imencode('.jpg') -> cv2.imdecode of every camera frame, "to align with training") on the
// device, bit-identical to libjpeg with jpeg_set_defaults: quality scaling of the Annex K tables, 4:2:0, the islow DCT, fancy up-sampling.
// The entropy coder is lossless and is not run: what changes pixels is colour conversion, down-sampling, forward DCT, quantise / dequantise,
// inverse DCT, up-sampling and the conversion back, all of it int32 arithmetic as in libjpeg (jccolor.c, jcsample.c, jfdctint.c, jcdctmgr.c,
// jidctint.c, jdsample.c, jdcolor.c).  uint8 HWC in (pitched views allowed), uint8 HWC out (tight), as vt_colorjitter.
//
// Launches of one vt_jpegmap call, over all frames at once:
//   jpegmap_mcu_kernel     one wave = one 16 x 16 MCU.  Every lane loads 4 pixels of a row (edge pixels replicated), Y and the horizontal
//                          chroma pair sums go to LDS, 64 lanes finish the 8 x 8 Cb / Cr samples, then lanes 0..47 each own one 8-vector of the
//                          6 blocks per pass: forward rows | forward columns, quantise, dequantise, inverse columns (in registers: the same
//                          vector) | inverse rows -> 8 decoded bytes of Y', Cb' or Cr' in the workspace.  Blocks are [8][9] int32 in LDS, 72
//                          words apart: a row pass has lane (b, r) at word 72 b + 9 r + k and a column pass lane (b, c) at 72 b + 9 k + c,
//                          both a permutation of the 32 banks over each 32-lane group.
//   jpegmap_upsample_kernel  one lane = 2 rows x 4 columns of the output: Y', the clamped 3 x 4 neighbourhood of Cb' and Cr', the triangle
//                          filter, the conversion, 12 bytes per row.  A launch of its own: the filter reads decoded chroma of neighbouring MCUs.
// The inverse DCT pass, the plane layout and the up-sampling item are vt_jpeg.h's, shared with the decoder of stored files (vt_jpegdec.hip).
// Workspace: per frame the planes Y' [H16][W16], Cb' and Cr' [H16 / 2][W16 / 2] of the frame padded to multiples of 16 (1.5 bytes per pixel).
#include <stdint.h>
#include "vt_common.h"
#include "vt_frames.h"
#include "vt_jpeg.h"
#include "vt_pixel.h"
#include "../../include/vlatouch.h"

namespace {
constexpr int kRow = 9;            // words per row of a block in LDS
constexpr int kBlk = 8 * kRow;     // words per block
constexpr int kNT = 256;           // threads per block of the up-sampling launch

// Annex K of ITU-T T.81, natural order
__device__ const unsigned char kBase[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

// one pass of jfdctint on d[0..8): FIRST = the row pass (PASS1_BITS up-scaling), else the column pass
template <bool FIRST> __device__ __forceinline__ void fdct8(int d[8]) {
  const int t0 = d[0] + d[7], t1 = d[1] + d[6], t2 = d[2] + d[5], t3 = d[3] + d[4];
  int t7 = d[0] - d[7], t6 = d[1] - d[6], t5 = d[2] - d[5], t4 = d[3] - d[4];
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  constexpr int n = FIRST ? 11 : 15;
  d[0] = FIRST ? (t10 + t11) << 2 : descale(t10 + t11, 2);
  d[4] = FIRST ? (t10 - t11) << 2 : descale(t10 - t11, 2);
  const int z1 = (t12 + t13) * 4433;
  d[2] = descale(z1 + t13 * 6270, n);
  d[6] = descale(z1 - t12 * 15137, n);
  odd_part(t4, t5, t6, t7);
  d[7] = descale(t4, n); d[5] = descale(t5, n); d[3] = descale(t6, n); d[1] = descale(t7, n);
}

__global__ void __launch_bounds__(64) jpegmap_mcu_kernel(const vt_jpegmap_frame* __restrict__ frames, const int scale, const int flags,
                                                         uint8_t* __restrict__ ws) {
  const vt_jpegmap_frame f = frames[blockIdx.y];
  const PlaneGeom g = plane_geom(f.h, f.w);
  const int mw = g.W16 >> 4;
  if ((int)blockIdx.x >= mw * (g.H16 >> 4)) return;      // block-uniform
  const int my = blockIdx.x / mw, mx = blockIdx.x - my * mw;
  const int lane = threadIdx.x;
  __shared__ int blk[6 * kBlk];
  __shared__ int hsum[2][16][8];      // Cb | Cr: the sum of each horizontal pixel pair of the MCU's 16 rows

  {  // pixels [x0, x0 + 4) of MCU row r; past the frame's edge the last row / column repeats
    const int r = lane >> 2, xq = (lane & 3) << 2;
    const int y = min(my * 16 + r, f.h - 1), x0 = mx * 16 + xq;
    const uint8_t* rowp = (const uint8_t*)f.src + (long)y * f.pitch;
    uint32_t px[4];
    const uint8_t* sp = rowp + 3L * x0;
    if (x0 + 4 <= f.w && ((uintptr_t)sp & 3) == 0) load_px4(sp, px);
    else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const uint8_t* p = rowp + 3L * min(x0 + j, f.w - 1);
        px[j] = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
      }
    }
    int cbv[4], crv[4];
    int* yb = blk + ((r >> 3) * 2 + (xq >> 3)) * kBlk + (r & 7) * kRow + (xq & 7);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      int R = px[j] & 255, G = (px[j] >> 8) & 255, B = px[j] >> 16;
      if (flags & VT_JPEGMAP_CV2_ORDER) { const int t = R; R = B; B = t; }
      yb[j] = ((19595 * R + 38470 * G + 7471 * B + kJpegHalf) >> 16) - 128;      // luma8(R, G, B) written out: through the helper this kernel came out 20 bytes shorter, and it is held to its size
      cbv[j] = (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + kJpegHalf - 1) >> 16;
      crv[j] = (32768 * R - 27439 * G - 5329 * B + (128 << 16) + kJpegHalf - 1) >> 16;
    }
    hsum[0][r][xq >> 1] = cbv[0] + cbv[1]; hsum[0][r][(xq >> 1) + 1] = cbv[2] + cbv[3];
    hsum[1][r][xq >> 1] = crv[0] + crv[1]; hsum[1][r][(xq >> 1) + 1] = crv[2] + crv[3];
  }
  __syncthreads();
  {  // chroma sample (j, i) of the MCU: libjpeg repeats the last down-sampled ROW below the frame, not the last pixel row
    const int j = lane >> 3, i = lane & 7;
    const int jc = min(my * 8 + j, ((f.h + 1) >> 1) - 1);
    const int ra = 2 * jc - my * 16, rb = min(2 * jc + 1, f.h - 1) - my * 16;      // both inside this MCU: it holds row h - 1 whenever it clamps
    const int bias = 1 + (i & 1);
    blk[4 * kBlk + j * kRow + i] = ((hsum[0][ra][i] + hsum[0][rb][i] + bias) >> 2) - 128;
    blk[5 * kBlk + j * kRow + i] = ((hsum[1][ra][i] + hsum[1][rb][i] + bias) >> 2) - 128;
  }
  __syncthreads();
  const int b = lane >> 3, v = lane & 7;
  int d[8];
  if (lane < 48) {   // forward rows
    int* p = blk + b * kBlk + v * kRow;
#pragma unroll
    for (int k = 0; k < 8; ++k) d[k] = p[k];
    fdct8<true>(d);
#pragma unroll
    for (int k = 0; k < 8; ++k) p[k] = d[k];
  }
  __syncthreads();
  if (lane < 48) {   // forward columns, quantise, dequantise, inverse columns
    int* p = blk + b * kBlk + v;
#pragma unroll
    for (int k = 0; k < 8; ++k) d[k] = p[k * kRow];
    fdct8<false>(d);
    const unsigned char* base = kBase[b >= 4 ? 1 : 0];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      int t = ((int)base[k * 8 + v] * scale + 50) / 100;
      t = t < 1 ? 1 : (t > 255 ? 255 : t);
      const int dv = 8 * t;        // jfdctint leaves the coefficients scaled by 8
      const int a = ((d[k] < 0 ? -d[k] : d[k]) + (dv >> 1)) / dv;
      d[k] = (d[k] < 0 ? -a : a) * t;
    }
    idct8<11>(d);
#pragma unroll
    for (int k = 0; k < 8; ++k) p[k * kRow] = d[k];
  }
  __syncthreads();
  if (lane < 48) {   // inverse rows -> 8 decoded samples
    const int* p = blk + b * kBlk + v * kRow;
#pragma unroll
    for (int k = 0; k < 8; ++k) d[k] = p[k];
    idct8<18>(d);
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      lo |= (uint32_t)clip8(d[k] + 128) << (8 * k);
      hi |= (uint32_t)clip8(d[k + 4] + 128) << (8 * k);
    }
    uint8_t* base = ws + f.ws_off;
    uint8_t* dp;
    if (b < 4) dp = base + (long)(my * 16 + (b >> 1) * 8 + v) * g.W16 + mx * 16 + (b & 1) * 8;
    else dp = base + (b == 4 ? g.cb : g.cr) + (long)(my * 8 + v) * (g.W16 >> 1) + mx * 8;
    *(uint2*)dp = make_uint2(lo, hi);     // 8-byte aligned: ws_off is a multiple of 256, W16 of 16
  }
}

__global__ void __launch_bounds__(kNT) jpegmap_upsample_kernel(const vt_jpegmap_frame* __restrict__ frames, const int flags,
                                                               const uint8_t* __restrict__ ws, uint8_t* __restrict__ out) {
  const vt_jpegmap_frame f = frames[blockIdx.y];
  jpeg_upsample_item(ws + f.ws_off, f.h, f.w, flags, (long)blockIdx.x * kNT + threadIdx.x, out + f.out_off);
}

// the checks of one record that both entry points make; 0 or VT_ERR_ARG with the message set
int check_frame(const char* fn, const vt_jpegmap_frame& f, const int i) {
  CK(vt_frame_check(fn, f, i));
  return (f.h > kJpegMaxSide || f.w > kJpegMaxSide) ? vt_fail(VT_ERR_ARG, "%s: frame %d of %d x %d is too large (at most %d a side)", fn, i, f.h, f.w, kJpegMaxSide) : VT_OK;
}
inline size_t frame_ws_bytes(const vt_jpegmap_frame& f) {
  const PlaneGeom g = plane_geom(f.h, f.w);
  return (size_t)g.cb * 3 / 2;
}
}  // namespace

extern "C" size_t vt_jpegmap_workspace_bytes(vt_jpegmap_frame* frames_host, int n) {
  if (vt_frames_table_check("vt_jpegmap_workspace_bytes", frames_host, n)) return 0;
  VtCarver ws;
  for (int i = 0; i < n; ++i) {
    if (check_frame("vt_jpegmap_workspace_bytes", frames_host[i], i)) return 0;
    frames_host[i].ws_off = (long)ws.take(frame_ws_bytes(frames_host[i]));
  }
  return ws.o;
}

extern "C" int vt_jpegmap(const vt_jpegmap_frame* frames_host, const void* frames_dev, int n, int quality, int flags, void* out, void* ws,
                          size_t ws_bytes, vt_stream_t stream) {
  CK(vt_frames_call_check("vt_jpegmap", frames_host, n, flags, VT_JPEGMAP_CV2_ORDER));
  if (quality < 1 || quality > 100) return vt_fail(VT_ERR_ARG, "vt_jpegmap: quality %d is not in 1..100", quality);
  long max_mcus = 1, max_items = 1;
  VtCarver need;
  for (int i = 0; i < n; ++i) {
    const vt_jpegmap_frame& f = frames_host[i];
    CK(check_frame("vt_jpegmap", f, i));
    // the layout vt_jpegmap_workspace_bytes wrote: the kernels store at ws_off, so a table that did not pass through it is refused
    if (f.ws_off != (long)need.take(frame_ws_bytes(f)))
      return vt_fail(VT_ERR_ARG, "vt_jpegmap: frame %d: ws_off %ld is not the one vt_jpegmap_workspace_bytes writes", i, f.ws_off);
    const PlaneGeom g = plane_geom(f.h, f.w);
    const long mcus = (long)(g.H16 >> 4) * (g.W16 >> 4);
    const long items = jpeg_upsample_items(f.h, f.w);
    max_mcus = mcus > max_mcus ? mcus : max_mcus;
    max_items = items > max_items ? items : max_items;
  }
  CK(vt_frames_buffers_check("vt_jpegmap", frames_dev, out, ws, ws_bytes, need.o, true));
  const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;      // jpeg_quality_scaling
  hipStream_t st = (hipStream_t)stream;
  const vt_jpegmap_frame* fd = (const vt_jpegmap_frame*)frames_dev;
  hipLaunchKernelGGL(jpegmap_mcu_kernel, dim3((unsigned)max_mcus, n), dim3(64), 0, st, fd, scale, flags, (uint8_t*)ws);
  hipLaunchKernelGGL(jpegmap_upsample_kernel, dim3((unsigned)((max_items + kNT - 1) / kNT), n), dim3(kNT), 0, st, fd, flags, (const uint8_t*)ws,
                     (uint8_t*)out);
  return vt_frames_launched("vt_jpegmap");
}
