// vt_imgprep.hip — camera frames (uint8 HWC RGB) -> SigLIP pixel_values on the device, bit-identical to the PIL path of
// scripts/franka_model_eef.py (RoboticDiffusionTransformerModel.preprocess_images; reference scripts/franka_model_eef.py:242-288):
// optional brightness lift, pad to square with the processor's mean colour (never materialised), antialiased resize with PIL's 8-bit
// resampler (horizontal pass, intermediate rounded to uint8, vertical pass; 22-bit fixed-point taps built by the host in double),
// then normalise + cast through a [3][256] table and a CHW store.
//
// Launches of one vt_imgprep call:
//   imgprep_sum_kernel    (brightness only) exact byte sums of every frame, one uint64 partial per block -> ws[n][64]; the consumers add them
//                         and take the decision themselves (no flag pass, nothing to zero, no read-back)
//   imgprep_fused_kernel  one workgroup = 16 output rows x 128 output columns of one frame: source rows -> LDS (wide loads), horizontal pass
//                         -> LDS bytes, vertical pass out of LDS, table lookup, 16-byte CHW stores
//   imgprep_h_kernel + imgprep_v_kernel   the same two passes through a uint8 scratch in the workspace: taken when a tile of some frame would
//                         need more than kFusedRows intermediate rows (vertical downscale beyond ~6x), for the uint8 HWC output mode
//                         (the `image_size` pre-resize), or on request (VT_IMGPREP_TWO_PASS)
// Integer VALU arithmetic only; every result is a pure function of the inputs (no atomics; the brightness sum is an integer sum).
#include <stdint.h>
#include "vt_common.h"
#include "vt_frames.h"
#include "vt_pixel.h"
#include "../../include/vlatouch.h"

namespace {
constexpr int kTR = 16;             // output rows of a tile
constexpr int kTC = 128;            // output columns of a tile
constexpr int kTCB = kTC * 3;       // bytes of one intermediate row of a tile
constexpr int kNT = 384;            // threads of a block: one per (column, channel) of the horizontal pass
constexpr int kStageBytes = 15360;  // LDS staging of source rows (wide global loads land here)
constexpr int kFusedRows = 128;     // most intermediate rows a fused tile keeps in LDS (48 KiB)
constexpr int kHR = 32;             // source rows of one block of imgprep_h_kernel
constexpr int kSumBlocks = 64;      // blocks per frame of imgprep_sum_kernel

struct Ctx {   // block-uniform view of one frame
  const uint8_t* src;
  long pitch;
  int h, w, in_h, in_w, pad_y, pad_x, out_h, out_w, ks_h, ks_v;
  const int* ch;   // horizontal table or null (pass skipped)
  const int* cv;
  bool lift;
  int fill;        // r | g << 8 | b << 16
};

__device__ __forceinline__ Ctx make_ctx(const vt_imgprep_frame& f, const int flags, const int fill, const unsigned long long* sums, const int i) {
  Ctx c;
  c.src = (const uint8_t*)f.src; c.pitch = f.pitch; c.h = f.h; c.w = f.w;
  c.out_h = f.out_h; c.out_w = f.out_w; c.ks_h = f.ksize_h; c.ks_v = f.ksize_v;
  c.ch = (const int*)f.coef_h; c.cv = (const int*)f.coef_v;
  c.in_h = f.h; c.in_w = f.w; c.pad_y = 0; c.pad_x = 0;
  if (flags & VT_IMGPREP_PAD) {
    const int side = f.h > f.w ? f.h : f.w;
    c.in_h = c.in_w = side;
    c.pad_y = (side - f.h) / 2; c.pad_x = (side - f.w) / 2;
  }
  c.fill = fill;
  c.lift = false;
  if ((flags & VT_IMGPREP_BRIGHT) && c.src) {
    unsigned long long tot = 0;
    for (int j = 0; j < kSumBlocks; ++j) tot += __hip_atomic_load(&sums[(long)i * kSumBlocks + j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    c.lift = lift_decision(tot, f.h, f.w);
  }
  return c;
}

__device__ __forceinline__ int clampi(const int v, const int lo, const int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// Horizontal pass of virtual rows [r0, r1) x output columns [xx0, xx1) of one frame: dst[(r - r0) * dst_stride + (xx - xx0) * 3 + c].
// Thread tid owns element tid = (xx - xx0) * 3 + c of every row.  The real source rows of a chunk are first copied to `stage` with
// aligned 4-byte loads (bytes outside the frame's row are never read); a segment wider than the staging area is read in place.
__device__ void hpass(const Ctx& c, const int r0, const int r1, const int xx0, const int xx1, uint8_t* dst, const long dst_stride, uint8_t* stage) {
  const int tid = threadIdx.x;
  int xs0 = xx0, xs1 = xx1;
  if (c.ch) { xs0 = c.ch[2 * xx0]; xs1 = c.ch[2 * (xx1 - 1)] + c.ch[2 * (xx1 - 1) + 1]; }
  const int c0 = clampi(xs0 - c.pad_x, 0, c.w), c1 = clampi(xs1 - c.pad_x, 0, c.w);
  const int nb = 3 * (c1 - c0);                       // source bytes of one row that this tile touches
  const int sstride = (nb + 6) & ~3;                  // room for the alignment head (<= 3 bytes), multiple of 4
  const bool staged = c.src && nb > 0 && sstride <= kStageBytes;
  const int RB = staged ? kStageBytes / sstride : (r1 - r0);
  const int nel = (xx1 - xx0) * 3;
  const int xx = xx0 + tid / 3, chn = tid - (tid / 3) * 3;
  const bool active = tid < nel;
  const int fillc = (c.fill >> (8 * chn)) & 255;
  int xmin = xx, cnt = 1;
  const int* kk = nullptr;
  if (active && c.ch) { xmin = c.ch[2 * xx]; cnt = c.ch[2 * xx + 1]; kk = c.ch + 2 * c.out_w + (long)xx * c.ks_h; }
  for (int rb = r0; rb < r1; rb += RB) {
    const int re = rb + RB < r1 ? rb + RB : r1;
    const int q0 = clampi(rb - c.pad_y, 0, c.h), q1 = clampi(re - c.pad_y, 0, c.h);   // real rows of this chunk
    if (staged) {
      __syncthreads();                                 // the previous chunk's readers are done
      const int wave = tid >> 6, lane = tid & 63;
      for (int row = q0 + wave; row < q1; row += kNT / 64) {
        const uintptr_t A = (uintptr_t)(c.src + (long)row * c.pitch + 3 * c0);
        const int head = (int)(A & 3);
        const uint8_t* base = (const uint8_t*)(A - head);
        uint32_t* srow = (uint32_t*)(stage + (long)(row - q0) * sstride);
        const int ndw = (head + nb + 3) >> 2;
        for (int j = lane; j < ndw; j += 64) {
          uint32_t v = 0;
          if (4 * j >= head && 4 * j + 4 <= head + nb) v = *(const uint32_t*)(base + 4 * j);
          else {
            for (int b = 0; b < 4; ++b) {
              const int off = 4 * j + b;
              if (off >= head && off < head + nb) v |= (uint32_t)base[off] << (8 * b);
            }
          }
          srow[j] = v;
        }
      }
      __syncthreads();
    }
    if (!active) continue;
    for (int r = rb; r < re; ++r) {
      const int rr = r - c.pad_y;
      const bool real_row = c.src && rr >= 0 && rr < c.h;
      // channel chn of real column x: grow[3 * x] in place, stage[soff + 3 * x] when staged (soff alone may be negative: it stays an
      // integer until 3 * x is added, an LDS pointer must not wrap below its base)
      const uint8_t* grow = c.src + (long)rr * c.pitch + chn;
      int soff = 0;
      if (real_row && staged) soff = (rr - q0) * sstride + (int)((uintptr_t)(c.src + (long)rr * c.pitch + 3 * c0) & 3) - 3 * c0 + chn;
      int val;
      if (kk) {
        int acc = 1 << 21;
        for (int t = 0; t < cnt; ++t) {
          const int x = xmin + t - c.pad_x;
          int v = fillc;
          if (real_row && x >= 0 && x < c.w) { v = staged ? stage[soff + 3 * x] : grow[3 * x]; if (c.lift) v = lift8(v); }
          acc += kk[t] * v;
        }
        val = clip8(acc >> 22);
      } else {
        const int x = xx - c.pad_x;
        val = fillc;
        if (real_row && x >= 0 && x < c.w) { val = staged ? stage[soff + 3 * x] : grow[3 * x]; if (c.lift) val = lift8(val); }
      }
      dst[(long)(r - r0) * dst_stride + tid] = (uint8_t)val;
    }
  }
}

template <typename T> struct Vec4;
template <> struct Vec4<float> { typedef float4 type; };
template <> struct Vec4<uint16_t> { typedef ushort4 type; };

// Vertical pass + store of output rows [y0, y1) x columns [xx0, xx1): inter[(row - ybase) * istride + (xx - xbase) * 3 + c] holds the
// horizontal pass.  T = float / uint16_t (bf16 bits): table lookup and CHW store, 4 pixels of a row per item; uint8_t: HWC bytes.
template <typename T>
__device__ void vpass(const Ctx& c, const int y0, const int y1, const int xx0, const int xx1, const uint8_t* inter, const long istride,
                      const int ybase, const int xbase, T* out, const T* lut) {
  const int ngrp = (xx1 - xx0 + 3) >> 2;
  const int items = (y1 - y0) * 3 * ngrp;
  for (int it = threadIdx.x; it < items; it += kNT) {
    const int g = it % ngrp, rest = it / ngrp;
    const int chn = rest % 3, y = y0 + rest / 3;
    const int x = xx0 + 4 * g;
    const uint8_t* col = inter + (long)(x - xbase) * 3 + chn;
    int v[4];
    if (c.cv) {
      const int ymin = c.cv[2 * y], cnt = c.cv[2 * y + 1];
      const int* kk = c.cv + 2 * c.out_h + (long)y * c.ks_v;
      int acc[4] = {1 << 21, 1 << 21, 1 << 21, 1 << 21};
      for (int t = 0; t < cnt; ++t) {
        const int k = kk[t];
        const uint8_t* p = col + (long)(ymin + t - ybase) * istride;
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (x + j < xx1) acc[j] += k * p[3 * j];
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = clip8(acc[j] >> 22);
    } else {
      const uint8_t* p = col + (long)(y - ybase) * istride;
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = x + j < xx1 ? p[3 * j] : 0;
    }
    if constexpr (sizeof(T) == 1) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (x + j < xx1) out[((long)y * c.out_w + x + j) * 3 + chn] = (T)v[j];
    } else {
      T* o = out + ((long)chn * c.out_h + y) * c.out_w + x;
      const T* l = lut + chn * 256;
      if ((c.out_w & 3) == 0) {                          // x % 4 == 0 and x + 3 < out_w: one aligned 16- / 8-byte store
        typename Vec4<T>::type q;
        q.x = l[v[0]]; q.y = l[v[1]]; q.z = l[v[2]]; q.w = l[v[3]];
        *reinterpret_cast<typename Vec4<T>::type*>(o) = q;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (x + j < xx1) o[j] = l[v[j]];
      }
    }
  }
}

// a missing frame: the S x S image of the fill colour, which the host path does not resample at all
template <typename T>
__device__ void fill_tile(const int S, const int y0, const int y1, const int xx0, const int xx1, const int fill, T* out, const T* lut) {
  const int wdt = xx1 - xx0, items = (y1 - y0) * 3 * wdt;
  for (int it = threadIdx.x; it < items; it += kNT) {
    const int x = xx0 + it % wdt, rest = it / wdt;
    const int chn = rest % 3, y = y0 + rest / 3;
    out[((long)chn * S + y) * S + x] = lut[chn * 256 + ((fill >> (8 * chn)) & 255)];
  }
}

__global__ void __launch_bounds__(256) imgprep_sum_kernel(const vt_imgprep_frame* __restrict__ frames, unsigned long long* __restrict__ sums) {
  const vt_imgprep_frame f = frames[blockIdx.y];
  if (!f.src) return;        // a missing frame's partials are never read
  const uint8_t* src = (const uint8_t*)f.src;
  const int nb = 3 * f.w;
  unsigned long long tot[1] = {0};
  for (int row = blockIdx.x; row < f.h; row += gridDim.x) {
    const uintptr_t A = (uintptr_t)(src + (long)row * f.pitch);
    const int head = (int)(A & 3);
    const uint8_t* base = (const uint8_t*)(A - head);
    const int ndw = (head + nb + 3) >> 2;
    uint32_t s = 0;
    for (int j = threadIdx.x; j < ndw; j += 256) {
      if (4 * j >= head && 4 * j + 4 <= head + nb) {
        const uint32_t v = *(const uint32_t*)(base + 4 * j);
        s += (v & 255u) + ((v >> 8) & 255u) + ((v >> 16) & 255u) + (v >> 24);
      } else {
        for (int b = 0; b < 4; ++b) {
          const int off = 4 * j + b;
          if (off >= head && off < head + nb) s += base[off];
        }
      }
    }
    tot[0] += s;
  }
  block_sums_store(tot, sums + (long)blockIdx.y * kSumBlocks + blockIdx.x, 0);
}

template <typename T>
__global__ void __launch_bounds__(kNT) imgprep_fused_kernel(const vt_imgprep_frame* __restrict__ frames, const unsigned long long* __restrict__ sums,
                                                            const int S, const T* __restrict__ lut, const int fill, const int flags, const int rows_cap, T* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  uint8_t* stage = smem;
  uint8_t* inter = smem + kStageBytes;
  const int i = blockIdx.z;
  const Ctx c = make_ctx(frames[i], flags, fill, sums, i);
  const int xx0 = blockIdx.x * kTC, y0 = blockIdx.y * kTR;
  const int xx1 = xx0 + kTC < S ? xx0 + kTC : S, y1 = y0 + kTR < S ? y0 + kTR : S;
  T* o = out + (long)i * 3 * S * S;
  if (!c.src) { fill_tile<T>(S, y0, y1, xx0, xx1, fill, o, lut); return; }
  int r0 = y0, r1 = y1;
  if (c.cv) { r0 = c.cv[2 * y0]; r1 = c.cv[2 * (y1 - 1)] + c.cv[2 * (y1 - 1) + 1]; }
  if (r1 - r0 > rows_cap) return;          // more rows than the LDS of this launch holds: rows_max of the frame table was wrong
  hpass(c, r0, r1, xx0, xx1, inter, kTCB, stage);
  __syncthreads();
  vpass<T>(c, y0, y1, xx0, xx1, inter, kTCB, r0, xx0, o, lut);
}

__global__ void __launch_bounds__(kNT) imgprep_h_kernel(const vt_imgprep_frame* __restrict__ frames, const unsigned long long* __restrict__ sums,
                                                        const int fill, const int flags, uint8_t* __restrict__ ws) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int i = blockIdx.z;
  const vt_imgprep_frame f = frames[i];
  if (!f.src) return;
  const Ctx c = make_ctx(f, flags, fill, sums, i);
  const int xx0 = blockIdx.x * kTC, r0 = blockIdx.y * kHR;
  if (xx0 >= c.out_w || r0 >= c.in_h) return;
  const int xx1 = xx0 + kTC < c.out_w ? xx0 + kTC : c.out_w, r1 = r0 + kHR < c.in_h ? r0 + kHR : c.in_h;
  const long stride = (long)c.out_w * 3;
  hpass(c, r0, r1, xx0, xx1, ws + f.ws_off + (long)r0 * stride + (long)xx0 * 3, stride, smem);
}

template <typename T>
__global__ void __launch_bounds__(kNT) imgprep_v_kernel(const vt_imgprep_frame* __restrict__ frames, const int S, const T* __restrict__ lut, const int fill,
                                                        const int flags, const uint8_t* __restrict__ ws, T* __restrict__ out) {
  const int i = blockIdx.z;
  const vt_imgprep_frame f = frames[i];
  const int xx0 = blockIdx.x * kTC, y0 = blockIdx.y * kTR;
  const int ow = sizeof(T) == 1 ? f.out_w : S, oh = sizeof(T) == 1 ? f.out_h : S;     // a missing frame's record carries no sizes
  if (xx0 >= ow || y0 >= oh) return;
  const int xx1 = xx0 + kTC < ow ? xx0 + kTC : ow, y1 = y0 + kTR < oh ? y0 + kTR : oh;
  if constexpr (sizeof(T) == 1) {
    const Ctx c = make_ctx(f, 0, fill, nullptr, i);
    vpass<T>(c, y0, y1, xx0, xx1, ws + f.ws_off, (long)f.out_w * 3, 0, 0, out + f.out_off, lut);
  } else {
    T* o = out + (long)i * 3 * S * S;
    if (!f.src) { fill_tile<T>(S, y0, y1, xx0, xx1, fill, o, lut); return; }
    const Ctx c = make_ctx(f, flags & VT_IMGPREP_PAD, fill, nullptr, i);
    vpass<T>(c, y0, y1, xx0, xx1, ws + f.ws_off, (long)f.out_w * 3, 0, 0, o, lut);
  }
}

inline void virt_size(const vt_imgprep_frame& f, const int flags, int& in_h, int& in_w) {
  in_h = f.h; in_w = f.w;
  if (flags & VT_IMGPREP_PAD) in_h = in_w = f.h > f.w ? f.h : f.w;
}
// argument check of one call; returns 0 or a vt_fail code.  `fused` receives whether every frame fits the fused kernel
int check_frames(const vt_imgprep_frame* fr, const int n, const int S, const int flags, bool& fused) {
  CK(vt_frames_table_check("vt_imgprep", fr, n));
  const bool u8 = flags & VT_IMGPREP_OUT_U8;
  if (u8 && (flags & (VT_IMGPREP_OUT_BF16 | VT_IMGPREP_BRIGHT | VT_IMGPREP_PAD)))
    return vt_fail(VT_ERR_ARG, "vt_imgprep: the uint8 HWC output mode takes no pad / brightness / bf16 flag");
  if (!u8 && S < 1) return vt_fail(VT_ERR_ARG, "vt_imgprep: output size S < 1");
  fused = !u8 && !(flags & VT_IMGPREP_TWO_PASS);
  for (int i = 0; i < n; ++i) {
    const vt_imgprep_frame& f = fr[i];
    if (!f.src) {
      if (u8) return vt_fail(VT_ERR_ARG, "vt_imgprep: frame %d is missing (null), which the uint8 HWC output mode does not take", i);
      continue;
    }
    if (f.h < 1 || f.w < 1 || f.out_h < 1 || f.out_w < 1) return vt_fail(VT_ERR_ARG, "vt_imgprep: frame %d has a zero size (%d x %d -> %d x %d)", i, f.h, f.w, f.out_h, f.out_w);
    CK(vt_frame_pitch_check("vt_imgprep", f, i));
    if (!u8 && (f.out_h != S || f.out_w != S)) return vt_fail(VT_ERR_ARG, "vt_imgprep: frame %d: output %d x %d is not S = %d", i, f.out_h, f.out_w, S);
    int in_h, in_w;
    virt_size(f, flags, in_h, in_w);
    if (!f.coef_h && in_w != f.out_w) return vt_fail(VT_ERR_ARG, "vt_imgprep: frame %d: null horizontal table but width %d != %d", i, in_w, f.out_w);
    if (!f.coef_v && in_h != f.out_h) return vt_fail(VT_ERR_ARG, "vt_imgprep: frame %d: null vertical table but height %d != %d", i, in_h, f.out_h);
    if ((f.coef_h && f.ksize_h < 1) || (f.coef_v && f.ksize_v < 1)) return vt_fail(VT_ERR_ARG, "vt_imgprep: frame %d: tap count < 1", i);
    if (f.rows_max < 1) return vt_fail(VT_ERR_ARG, "vt_imgprep: frame %d: rows_max < 1", i);
    if (f.rows_max > kFusedRows) fused = false;
  }
  return VT_OK;
}
}  // namespace

extern "C" size_t vt_imgprep_workspace_bytes(vt_imgprep_frame* frames, int n, int S, int flags) {
  bool fused = false;
  if (check_frames(frames, n, S, flags, fused)) return 0;
  size_t off = vt_round256((size_t)n * kSumBlocks * sizeof(unsigned long long));
  for (int i = 0; i < n; ++i) {
    frames[i].ws_off = (long)off;
    if (fused || !frames[i].src) continue;
    int in_h, in_w;
    virt_size(frames[i], flags, in_h, in_w);
    off += vt_round16((size_t)in_h * frames[i].out_w * 3);
  }
  return off;
}

extern "C" int vt_imgprep(const vt_imgprep_frame* frames_host, const void* frames_dev, int n, int S, const void* lut, unsigned fill_rgb,
                          int flags, void* out, void* ws, size_t ws_bytes, vt_stream_t stream) {
  bool fused = false;
  CK(check_frames(frames_host, n, S, flags, fused));
  const bool u8 = flags & VT_IMGPREP_OUT_U8;
  if (!u8 && !lut) return vt_fail(VT_ERR_ARG, "vt_imgprep: null normalise table");
  if (!u8 && ((uintptr_t)out & 15)) return vt_fail(VT_ERR_ARG, "vt_imgprep: the output must be 16-byte aligned");
  // the workspace layout vt_imgprep_workspace_bytes gave (ws_off of every frame) must be the one in the table
  size_t need = vt_round256((size_t)n * kSumBlocks * sizeof(unsigned long long));
  int max_in_h = 1, max_out_h = u8 ? 1 : S, max_out_w = u8 ? 1 : S, rows_cap = 1;
  for (int i = 0; i < n; ++i) {
    const vt_imgprep_frame& f = frames_host[i];
    if (!f.src) continue;
    int in_h, in_w;
    virt_size(f, flags, in_h, in_w);
    if (!fused) {
      if (f.ws_off != (long)need) return vt_fail(VT_ERR_ARG, "vt_imgprep: frame %d: ws_off %ld is not the planned %zu (call vt_imgprep_workspace_bytes on the table first)", i, f.ws_off, need);
      need += vt_round16((size_t)in_h * f.out_w * 3);
    }
    if (u8 && f.out_off < 0) return vt_fail(VT_ERR_ARG, "vt_imgprep: frame %d: negative out_off", i);
    max_in_h = in_h > max_in_h ? in_h : max_in_h;
    max_out_h = f.out_h > max_out_h ? f.out_h : max_out_h;
    max_out_w = f.out_w > max_out_w ? f.out_w : max_out_w;
    rows_cap = f.rows_max > rows_cap ? f.rows_max : rows_cap;
  }
  CK(vt_frames_buffers_check("vt_imgprep", frames_dev, out, ws, ws_bytes, need, false));      // (this entry point never asked for an aligned workspace)
  hipStream_t st = (hipStream_t)stream;
  const vt_imgprep_frame* fd = (const vt_imgprep_frame*)frames_dev;
  unsigned long long* sums = (unsigned long long*)ws;
  const int fill = (int)(fill_rgb & 0xffffffu);
  if (flags & VT_IMGPREP_BRIGHT)
    hipLaunchKernelGGL(imgprep_sum_kernel, dim3(kSumBlocks, n), dim3(256), 0, st, fd, sums);
  const dim3 tiles((max_out_w + kTC - 1) / kTC, (max_out_h + kTR - 1) / kTR, n);
  const bool bf = flags & VT_IMGPREP_OUT_BF16;
  if (fused) {
    const size_t lds = kStageBytes + (size_t)rows_cap * kTCB;
    if (bf) hipLaunchKernelGGL((imgprep_fused_kernel<uint16_t>), tiles, dim3(kNT), lds, st, fd, sums, S, (const uint16_t*)lut, fill, flags, rows_cap, (uint16_t*)out);
    else hipLaunchKernelGGL((imgprep_fused_kernel<float>), tiles, dim3(kNT), lds, st, fd, sums, S, (const float*)lut, fill, flags, rows_cap, (float*)out);
  } else {
    hipLaunchKernelGGL(imgprep_h_kernel, dim3(tiles.x, (max_in_h + kHR - 1) / kHR, n), dim3(kNT), kStageBytes, st, fd, sums, fill, flags, (uint8_t*)ws);
    if (u8) hipLaunchKernelGGL((imgprep_v_kernel<uint8_t>), tiles, dim3(kNT), 0, st, fd, S, (const uint8_t*)nullptr, fill, flags, (const uint8_t*)ws, (uint8_t*)out);
    else if (bf) hipLaunchKernelGGL((imgprep_v_kernel<uint16_t>), tiles, dim3(kNT), 0, st, fd, S, (const uint16_t*)lut, fill, flags, (const uint8_t*)ws, (uint16_t*)out);
    else hipLaunchKernelGGL((imgprep_v_kernel<float>), tiles, dim3(kNT), 0, st, fd, S, (const float*)lut, fill, flags, (const uint8_t*)ws, (float*)out);
  }
  return vt_frames_launched("vt_imgprep");
}
