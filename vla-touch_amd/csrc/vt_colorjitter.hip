// vt_colorjitter.hip — the training-time colour augmentation of camera frames (train/dataset.py:379-391: brightness lift, then
// transforms.ColorJitter on PIL images) on the device, bit-identical to PIL: ImageEnhance.Brightness / Contrast / Color are Image.blend
// against black / the rounded mean of L / the pixel's L, the hue step is Pillow's RGB -> HSV -> RGB (Convert.c) with a byte added to H.
// uint8 HWC RGB in (pitched views allowed), uint8 HWC RGB out (tight), so the stage sits in front of vt_imgprep.
//
// Launches of one vt_colorjitter call, over all frames at once:
//   colorjitter_sum_kernel    exact integer sums of every frame that needs one, one uint64 partial per block -> ws[n][3][64]: the byte sum
//                             (VT_COLORJITTER_LIFT: the lift decision) and, for a frame whose order holds contrast, the sum of L after the
//                             operations in front of contrast, formed for the unlifted and for the lifted pixel so that the consumer
//                             chooses.  Skipped when no frame needs a sum.
//   colorjitter_apply_kernel  one thread = 4 pixels of a row (three 32-bit words in, three out where both addresses are 4-byte aligned,
//                             bytes otherwise): adds the partials, takes the lift decision and the contrast mean, applies the slots in order.
// PIL's x86-64 build rounds every multiply and add separately, hipcc contracts a * b + c into an FMA in device code by default: contraction
// is off for this file (the pragma below), and the arithmetic is written with plain operators, which the pragma governs.  The header
// intrinsics (__fmul_rn, __fadd_rn, ...) are inline functions compiled in front of the pragma: a product and a sum that come out of them
// both carry the contract flag and are fused all the same, which moved one byte in half of the contrast test's frames.  Divisions are the
// correctly rounded ones (hipcc's default for fp32 `/`).  The sums are integers: every result is a pure function of the inputs.
#include <stdint.h>
#include <limits.h>
#include "vt_common.h"
#include "vt_frames.h"
#include "vt_pixel.h"
#include "../../include/vlatouch.h"

#pragma clang fp contract(off)   // after the includes: it governs every expression of this file, and only those

namespace {
constexpr int kSumBlocks = 64;   // blocks per frame of colorjitter_sum_kernel = lanes of a wave (the consumer adds them with one shuffle tree)
constexpr int kSums = 3;         // per frame: byte sum, sum of L (unlifted), sum of L (lifted)
constexpr int kNT = 256;

// Image.blend(a, b, f) of one byte; for 0 <= f <= 1 PIL truncates without clipping, where t lies in [0, 255] anyway
__device__ __forceinline__ int blend8(const int a, const int b, const float f) {
  const float t = (float)a + f * (float)(b - a);
  return t <= 0.f ? 0 : (t >= 255.f ? 255 : (int)t);
}

// Pillow's rgb2hsv, H += shift (mod 256), hsv2rgb
__device__ __forceinline__ void hue_px(int& r, int& g, int& b, const int shift) {
  const int mx = max(r, max(g, b)), mn = min(r, min(g, b));
  int H = 0, S = 0;
  const int V = mx;
  if (mx != mn) {
    const float mxf = (float)mx, cr = (float)(mx - mn);
    const float s = cr / mxf;
    const float rc = (float)(mx - r) / cr, gc = (float)(mx - g) / cr, bc = (float)(mx - b) / cr;
    float h;
    if (r == mx) h = bc - gc;
    else if (g == mx) h = (float)((2.0 + (double)rc) - (double)bc);      // double literals: formed in double, rounded once
    else h = (float)((4.0 + (double)gc) - (double)rc);
    double x = (double)h / 6.0 + 1.0;                                           // fmod(x, 1.0) for 0 <= x < 2, exact
    if (x >= 1.0) x = x - 1.0;
    const float hf = (float)x;
    H = clip8((int)((double)hf * 255.0));
    S = clip8((int)((double)s * 255.0));
  }
  H = (H + shift) & 255;
  if (S == 0) { r = g = b = V; return; }
  const double hh = (double)H * 6.0 / 255.0;
  const int i = (int)floor(hh);
  const double f = (double)(float)(hh - (double)(float)i);
  const double fs = (double)(float)((double)S / 255.0);
  const double v = (double)V;
  const int p = clip8((int)round(v * (1.0 - fs)));
  const int q = clip8((int)round(v * (1.0 - fs * f)));
  const int t = clip8((int)round(v * (1.0 - fs * (1.0 - f))));
  switch (i % 6) {
    case 0: r = V; g = t; b = p; break;
    case 1: r = q; g = V; b = p; break;
    case 2: r = p; g = V; b = t; break;
    case 3: r = p; g = q; b = V; break;
    case 4: r = t; g = p; b = V; break;
    default: r = V; g = p; b = q; break;
  }
}

// slots [0, nslots) of a frame's order on one pixel; `mean` is read only by a contrast slot
__device__ __forceinline__ void apply_slots(const vt_colorjitter_frame& f, const int nslots, const int mean, int& r, int& g, int& b) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {       // static indices: the record stays in registers
    if (k >= nslots) break;
    switch (f.order[k]) {
      case VT_COLORJITTER_BRIGHTNESS: r = blend8(0, r, f.brightness); g = blend8(0, g, f.brightness); b = blend8(0, b, f.brightness); break;
      case VT_COLORJITTER_CONTRAST: r = blend8(mean, r, f.contrast); g = blend8(mean, g, f.contrast); b = blend8(mean, b, f.contrast); break;
      case VT_COLORJITTER_SATURATION: { const int l = luma8(r, g, b); r = blend8(l, r, f.saturation); g = blend8(l, g, f.saturation); b = blend8(l, b, f.saturation); break; }
      case VT_COLORJITTER_HUE: hue_px(r, g, b, f.hue_shift); break;
      default: break;
    }
  }
}

__device__ __forceinline__ int contrast_slot(const vt_colorjitter_frame& f) {
  int slot = -1;
#pragma unroll
  for (int k = 3; k >= 0; --k)
    if (f.order[k] == VT_COLORJITTER_CONTRAST) slot = k;
  return slot;
}

// item `it` of a frame = pixels [x0, x0 + npx) of row `row`, npx <= 4; returns npx and the 12 (or fewer) bytes as px[j] = r | g << 8 | b << 16
__device__ __forceinline__ int load_run(const vt_colorjitter_frame& f, const int it, int& row, int& x0, uint32_t px[4]) {
  const int rpr = (f.w + 3) >> 2;
  row = it / rpr;
  x0 = (it - row * rpr) << 2;
  const int npx = f.w - x0 < 4 ? f.w - x0 : 4;
  const uint8_t* sp = (const uint8_t*)f.src + (long)row * f.pitch + 3L * x0;
  if (npx == 4 && ((uintptr_t)sp & 3) == 0) load_px4(sp, px);
  else {
    for (int j = 0; j < 4; ++j) {
      px[j] = 0;
      if (j < npx) px[j] = (uint32_t)sp[3 * j] | ((uint32_t)sp[3 * j + 1] << 8) | ((uint32_t)sp[3 * j + 2] << 16);
    }
  }
  return npx;
}

__global__ void __launch_bounds__(kNT) colorjitter_sum_kernel(const vt_colorjitter_frame* __restrict__ frames, const int flags,
                                                              unsigned long long* __restrict__ sums) {
  const vt_colorjitter_frame f = frames[blockIdx.y];
  const bool lift = flags & VT_COLORJITTER_LIFT;
  const int cs = contrast_slot(f);
  if (!lift && cs < 0) return;        // this frame's partials are never read
  const int items = f.h * ((f.w + 3) >> 2);
  unsigned long long tot[kSums] = {0, 0, 0};
  for (int it = blockIdx.x * kNT + threadIdx.x; it < items; it += kSumBlocks * kNT) {
    int row, x0;
    uint32_t px[4];
    const int npx = load_run(f, it, row, x0, px);
    uint32_t s0 = 0, s1 = 0, s2 = 0;
    for (int j = 0; j < npx; ++j) {
      const int r = px[j] & 255, g = (px[j] >> 8) & 255, b = px[j] >> 16;
      s0 += r + g + b;
      if (cs >= 0) {
        int r1 = r, g1 = g, b1 = b;
        apply_slots(f, cs, 0, r1, g1, b1);
        s1 += luma8(r1, g1, b1);
        if (lift) {
          int r2 = lift8(r), g2 = lift8(g), b2 = lift8(b);
          apply_slots(f, cs, 0, r2, g2, b2);
          s2 += luma8(r2, g2, b2);
        }
      }
    }
    tot[0] += s0; tot[1] += s1; tot[2] += s2;
  }
  block_sums_store(tot, sums + (long)blockIdx.y * kSums * kSumBlocks + blockIdx.x, kSumBlocks);
}

// the frame's sum k: every lane of the wave adds one block's partial
__device__ __forceinline__ unsigned long long frame_sum(const unsigned long long* sums, const int i, const int k) {
  unsigned long long v = __hip_atomic_load(&sums[((long)i * kSums + k) * kSumBlocks + (threadIdx.x & 63)], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ void __launch_bounds__(kNT) colorjitter_apply_kernel(const vt_colorjitter_frame* __restrict__ frames, const int flags,
                                                                const unsigned long long* __restrict__ sums, uint8_t* __restrict__ out) {
  const int i = blockIdx.y;
  const vt_colorjitter_frame f = frames[i];
  const int items = f.h * ((f.w + 3) >> 2);
  if ((long)blockIdx.x * kNT >= items) return;         // block-uniform: the shuffles below see whole waves
  const bool lift = (flags & VT_COLORJITTER_LIFT) && lift_decision(frame_sum(sums, i, 0), f.h, f.w);
  int mean = 0;
  if (contrast_slot(f) >= 0)                           // ImageEnhance.Contrast: int(ImageStat.Stat(image.convert("L")).mean[0] + 0.5)
    mean = (int)((double)frame_sum(sums, i, lift ? 2 : 1) / (double)((long)f.h * f.w) + 0.5);
  const int it = blockIdx.x * kNT + threadIdx.x;
  if (it >= items) return;
  int row, x0;
  uint32_t px[4];
  const int npx = load_run(f, it, row, x0, px);
  for (int j = 0; j < 4; ++j) {
    int r = px[j] & 255, g = (px[j] >> 8) & 255, b = px[j] >> 16;
    if (lift) { r = lift8(r); g = lift8(g); b = lift8(b); }
    apply_slots(f, 4, mean, r, g, b);
    px[j] = (uint32_t)r | ((uint32_t)g << 8) | ((uint32_t)b << 16);
  }
  store_px4(out + f.out_off + ((long)row * f.w + x0) * 3, px, npx);
}

inline size_t sums_bytes(const int n) { return vt_round256((size_t)n * kSums * kSumBlocks * sizeof(unsigned long long)); }
}  // namespace

extern "C" size_t vt_colorjitter_workspace_bytes(int n) {
  if (n < 1) { vt_fail(VT_ERR_ARG, "vt_colorjitter_workspace_bytes: n < 1"); return 0; }
  return sums_bytes(n);
}

extern "C" int vt_colorjitter(const vt_colorjitter_frame* frames_host, const void* frames_dev, int n, int flags, void* out, void* ws,
                              size_t ws_bytes, vt_stream_t stream) {
  CK(vt_frames_call_check("vt_colorjitter", frames_host, n, flags, VT_COLORJITTER_LIFT));
  bool need_sums = flags & VT_COLORJITTER_LIFT;
  long max_items = 1;
  for (int i = 0; i < n; ++i) {
    const vt_colorjitter_frame& f = frames_host[i];
    CK(vt_frame_check("vt_colorjitter", f, i));
    const long items = (long)f.h * ((f.w + 3) / 4);
    if (items > INT_MAX - kSumBlocks * kNT) return vt_fail(VT_ERR_ARG, "vt_colorjitter: frame %d of %d x %d is too large", i, f.h, f.w);
    unsigned seen = 0;
    for (int k = 0; k < 4; ++k) {
      const int op = f.order[k];
      if (op < 0 || op > VT_COLORJITTER_NONE) return vt_fail(VT_ERR_ARG, "vt_colorjitter: frame %d: unknown operation id %d in slot %d", i, op, k);
      if (op == VT_COLORJITTER_NONE) continue;
      if (seen & (1u << op)) return vt_fail(VT_ERR_ARG, "vt_colorjitter: frame %d: operation %d appears twice", i, op);
      seen |= 1u << op;
    }
    if (seen & (1u << VT_COLORJITTER_CONTRAST)) need_sums = true;
    max_items = items > max_items ? items : max_items;
  }
  CK(vt_frames_buffers_check("vt_colorjitter", frames_dev, out, ws, ws_bytes, sums_bytes(n), true));
  hipStream_t st = (hipStream_t)stream;
  const vt_colorjitter_frame* fd = (const vt_colorjitter_frame*)frames_dev;
  unsigned long long* sums = (unsigned long long*)ws;
  if (need_sums) hipLaunchKernelGGL(colorjitter_sum_kernel, dim3(kSumBlocks, n), dim3(kNT), 0, st, fd, flags, sums);
  hipLaunchKernelGGL(colorjitter_apply_kernel, dim3((unsigned)((max_items + kNT - 1) / kNT), n), dim3(kNT), 0, st, fd, flags, (const unsigned long long*)sums, (uint8_t*)out);
  return vt_frames_launched("vt_colorjitter");
}
