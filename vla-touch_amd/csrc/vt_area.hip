// vt_area.hip — the reference's first camera-frame stage on the device: `pad_and_resize_for_siglip` (scripts/utils_eef.py:5-77), a zero pad to
// a centred square of side m = max(h, w) followed by cv2.resize(..., (target, target), interpolation=cv2.INTER_AREA).  Restated from OpenCV 4.x
// modules/imgproc/src/resize.cpp (UNPINNED against cv2: vlatouch/imgprep.py), bit-identical to the numpy statement
// `vlatouch.imgprep.pad_and_resize_for_siglip`.  uint8 HWC in (pitched views allowed), uint8 HWC out (tight), as vt_jpegmap.
//
// One launch for all frames of a call, one output pixel (three channels) per lane.  The padded square is never made: a lane addresses the
// m x m canvas, clamps the position into it and reads 0 where it lies in the border.  Two forms, chosen by the driver as cv2 chooses:
//   the integer scale (resizeAreaFast_): the exact sum s of the iscale x iscale cell; iscale 1 copies, iscale 2 gives (s + 2) >> 2, any other
//     float(s) * float(1.0f / (iscale * iscale)) rounded to nearest-even;
//   the fractional scale (resizeArea_<uchar, float>): the host's tap table of an axis, [ntaps][target] pairs (source index, fp32 weight), the
//     shorter lists padded with zero weights.  Per vertical tap the row value buf = sum of S * alpha over the horizontal taps in table
//     order, then sum = beta * buf for the first vertical tap and sum += beta * buf for the others, every product and every sum rounded to
//     fp32 on its own (what an x86-64 build without FMA does), the result rounded to nearest-even and clamped.
// hipcc contracts a * b + c into an FMA in device code by default: contraction is off for this file (the pragma below), and the arithmetic
// is written with plain operators, which the pragma governs; a product and a sum out of the header intrinsics (__fmul_rn, __fadd_rn) are
// compiled in front of the pragma and fuse all the same (vt_colorjitter.hip met this first).
#include <float.h>
#include <math.h>
#include <stdint.h>
#include "vt_common.h"
#include "vt_frames.h"
#include "vt_pixel.h"
#include "../../include/vlatouch.h"

#pragma clang fp contract(off)   // after the includes: it governs every expression of this file, and only those

namespace {
constexpr int kNT = 256;           // threads per block
constexpr int kMaxSide = 32768;

struct AreaTap { int si; float alpha; };      // one entry of a tap table

// the three bytes at canvas position (sy, sx) of frame f, clamped into the m x m canvas; 0 in the zero border
__device__ __forceinline__ void canvas_px(const vt_area_frame& f, const int m, const int top, const int left, int sy, int sx, int v[3]) {
  sy = min(max(sy, 0), m - 1) - top;
  sx = min(max(sx, 0), m - 1) - left;
  if (sy < 0 || sy >= f.h || sx < 0 || sx >= f.w) { v[0] = v[1] = v[2] = 0; return; }
  const uint8_t* p = (const uint8_t*)f.src + (long)sy * f.pitch + 3L * sx;
  v[0] = p[0]; v[1] = p[1]; v[2] = p[2];
}

__global__ void __launch_bounds__(kNT) area_resize_kernel(const vt_area_frame* __restrict__ frames, const uint8_t* __restrict__ tabs,
                                                          uint8_t* __restrict__ out) {
  const vt_area_frame f = frames[blockIdx.y];
  const int T = f.target;
  const int it = (int)(blockIdx.x * kNT + threadIdx.x);      // T <= 32768: T * T and the grid's last thread fit an int
  if (it >= T * T) return;
  const int dy = it / T, dx = it - dy * T;
  const int m = max(f.h, f.w), top = (m - f.h) >> 1, left = (m - f.w) >> 1;
  int r[3];
  if (f.ntaps == 0) {                                  // integer scale: m == k * T
    const int k = m / T;
    int s[3] = {0, 0, 0}, v[3];
    for (int j = 0; j < k; ++j)
      for (int i = 0; i < k; ++i) {
        canvas_px(f, m, top, left, dy * k + j, dx * k + i, v);
        s[0] += v[0]; s[1] += v[1]; s[2] += v[2];
      }
    // 1.0f / (k * k) through double: a quotient of two fp32 values rounded to 53 bits and then to 24 is the correctly rounded fp32 quotient
    const float inv = (float)(1.0 / (double)(k * k));
#pragma unroll
    for (int c = 0; c < 3; ++c) r[c] = k == 1 ? s[c] : (k == 2 ? (s[c] + 2) >> 2 : clip8(__float2int_rn((float)s[c] * inv)));
  } else {
    const AreaTap* tx = (const AreaTap*)(tabs + f.tab_x);
    const AreaTap* ty = (const AreaTap*)(tabs + f.tab_y);
    float sum[3] = {0.f, 0.f, 0.f};
    for (int ky = 0; ky < f.ntaps; ++ky) {
      const AreaTap b = ty[(long)ky * T + dy];
      float buf[3] = {0.f, 0.f, 0.f};
      int v[3];
      for (int kx = 0; kx < f.ntaps; ++kx) {
        const AreaTap a = tx[(long)kx * T + dx];
        canvas_px(f, m, top, left, b.si, a.si, v);
#pragma unroll
        for (int c = 0; c < 3; ++c) buf[c] = buf[c] + (float)v[c] * a.alpha;
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) sum[c] = ky == 0 ? b.alpha * buf[c] : sum[c] + b.alpha * buf[c];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) r[c] = clip8(__float2int_rn(sum[c]));
  }
  uint8_t* dp = out + f.out_off + 3L * it;
  dp[0] = (uint8_t)r[0]; dp[1] = (uint8_t)r[1]; dp[2] = (uint8_t)r[2];
}

// cv2::resize's choice of form for an axis of m -> target: inv_scale = (double)dsize / ssize, scale = 1. / inv_scale, iscale = the truncated
// scale; below 1 the up-scale (not built), within DBL_EPSILON of an integer the cell sums, otherwise the tap table
enum AreaForm { kUpscale, kFast, kTable };
AreaForm area_form(const int m, const int target, int* iscale) {
  const double inv = (double)target / (double)m, scale = 1.0 / inv;
  *iscale = (int)scale;
  if (scale < 1.0) return kUpscale;
  return fabs(scale - *iscale) < DBL_EPSILON ? kFast : kTable;
}
}  // namespace

extern "C" int vt_area_resize(const vt_area_frame* frames_host, const void* frames_dev, int n, void* out, const void* tabs, size_t tabs_bytes,
                              vt_stream_t stream) {
  const char* fn = "vt_area_resize";
  CK(vt_frames_call_check(fn, frames_host, n, 0, 0));
  if (!frames_dev || !out) return vt_fail(VT_ERR_ARG, "%s: null device frame table or output", fn);
  int max_target = 1;
  for (int i = 0; i < n; ++i) {
    const vt_area_frame& f = frames_host[i];
    CK(vt_frame_check(fn, f, i));
    if (f.h > kMaxSide || f.w > kMaxSide) return vt_fail(VT_ERR_ARG, "%s: frame %d of %d x %d is too large (at most %d a side)", fn, i, f.h, f.w, kMaxSide);
    if (f.target < 1) return vt_fail(VT_ERR_ARG, "%s: frame %d: target size %d", fn, i, f.target);
    const int m = f.h > f.w ? f.h : f.w;
    int iscale = 0;
    const AreaForm form = area_form(m, f.target, &iscale);
    if (form == kUpscale)
      return vt_fail(VT_ERR_ARG, "%s: frame %d of %d x %d is smaller than the target %d: cv2's bilinear up-scale emulation is not built", fn, i, f.h,
                     f.w, f.target);
    if (form == kFast) {
      if (f.ntaps != 0) return vt_fail(VT_ERR_ARG, "%s: frame %d: %d -> %d is an integer scale and takes no tap table (ntaps %d)", fn, i, m, f.target, f.ntaps);
      if (iscale > VT_AREA_MAX_ISCALE)
        return vt_fail(VT_ERR_ARG, "%s: frame %d: a reduction by %d (at most %d: the cell sum is an int)", fn, i, iscale, VT_AREA_MAX_ISCALE);
    } else {
      if (f.ntaps < 1 || f.ntaps > iscale + 3)      // an output reaches over at most ceil(scale) + 2 source positions
        return vt_fail(VT_ERR_ARG, "%s: frame %d: %d -> %d takes a tap table of 1 .. %d taps an output, got %d", fn, i, m, f.target, iscale + 3, f.ntaps);
      if (!tabs) return vt_fail(VT_ERR_ARG, "%s: frame %d needs a tap table and the table area is null", fn, i);
      const size_t bytes = (size_t)f.ntaps * f.target * sizeof(AreaTap);
      for (const long off : {f.tab_x, f.tab_y})
        if (off < 0 || (off & 7) || (size_t)off + bytes > tabs_bytes)
          return vt_fail(VT_ERR_ARG, "%s: frame %d: a tap table of %zu bytes at %ld is misaligned or outside the %zu table bytes", fn, i, bytes, off,
                         tabs_bytes);
    }
    max_target = f.target > max_target ? f.target : max_target;
  }
  if (tabs && ((uintptr_t)tabs & 7)) return vt_fail(VT_ERR_ARG, "%s: the table area must be 8-byte aligned", fn);
  const long px = (long)max_target * max_target;      // target <= m <= 32768: at most 2^22 blocks
  hipLaunchKernelGGL(area_resize_kernel, dim3((unsigned)((px + kNT - 1) / kNT), n), dim3(kNT), 0, (hipStream_t)stream,
                     (const vt_area_frame*)frames_dev, (const uint8_t*)tabs, (uint8_t*)out);
  return vt_frames_launched(fn);
}
