// vt_corrupt.hip — the training-time corruption of camera frames (train/image_corrupt.py: imgaug's additive noise and blur, restated in
// integers) on the device.  uint8 HWC in (pitched views allowed), uint8 HWC out (tight), so the stage sits between
// vt_colorjitter and vt_imgprep.  The host does everything transcendental, once per frame: the noise arrives as a table of 510 cumulative
// thresholds, a Gaussian, box or motion blur as a list of integer taps; the device compares, multiplies and divides integers.
//
// One launch over all frames: a workgroup of 256 threads owns a 32 x 32 output tile of one frame (blockIdx.y = frame, blockIdx.x = tile) and
//   1. stages the tile plus a halo of the frame's blur radius (k / 2 <= 18) into LDS as HWC bytes, resolving the border there (the periodic
//      reflect-101 for the tap blurs, replicate for the median) and, when the noise comes first, adding it there: the noise is a pure
//      function of (key, source position), so a halo pixel gets the value its own tile gives it;
//   2. runs the frame's blur out of LDS, a thread on 4 pixels of a row = 12 bytes, read as four aligned words and shifted into place:
//      the tap correlation (S = sum of W * p in uint32, divided by D = sum of W, remainder rounded half to even) or the median (per byte a
//      bisection over the value: eight counting passes over the window, exact for every k);
//   3. adds the noise in the epilogue when the blur comes first, and writes 12 bytes as three words (vt_pixel.h).
// Frames of one call differ in every parameter: the dispatch is per workgroup, on block-uniform fields of the record.  No atomics, no
// workspace, no host read: a pure function of the inputs.
#include <stdint.h>
#include <limits.h>
#include "vt_common.h"
#include "vt_frames.h"
#include "vt_philox.h"
#include "vt_pixel.h"
#include "../../include/vlatouch.h"

namespace {
constexpr int kNT = 256;
constexpr int kTile = 32;                         // output tile side; a thread owns 4 pixels of a row: 8 threads per row, 32 rows
constexpr int kRmax = VT_CORRUPT_MAX_RADIUS;      // 18: motion blur at k = 37
constexpr int kSide = kTile + 2 * kRmax;          // 68 staged rows and columns at most
// LDS row pitch in bytes: >= 3 * 68 + 4 (the fourth word of a shifted read), and 72 words = 8 mod 32: a 32-lane half of a wave is four
// rows of eight lanes three words apart, whose word reads (banks (a / 4) % 32) then start at 8 row + 3 lane: 32 different banks
constexpr int kPitch = 288;
constexpr int kThresh = VT_CORRUPT_THRESHOLDS;    // 510: C[n], n = -255 .. 254

__device__ __forceinline__ int mirror_index(const int i, const int n) {      // reflect-101, periodic: period 2 (n - 1); n = 1 -> 0
  if ((unsigned)i < (unsigned)n) return i;
  if (n == 1) return 0;
  const int P = 2 * (n - 1);
  int m = i % P;
  if (m < 0) m += P;
  return m < n ? m : P - m;
}
__device__ __forceinline__ int clamp_index(const int i, const int n) { return i < 0 ? 0 : (i >= n ? n - 1 : i); }

__device__ __forceinline__ uint32_t word_of(const uint32_t (&c)[4], const int i) {
  return i == 0 ? c[0] : (i == 1 ? c[1] : (i == 2 ? c[2] : c[3]));
}
__device__ __forceinline__ void philox_at(const unsigned long long key, const unsigned long long ctr, uint32_t (&c)[4]) {
  c[0] = (uint32_t)ctr; c[1] = (uint32_t)(ctr >> 32); c[2] = 0u; c[3] = 0u;
  philox4x32_10(c, (uint32_t)key, (uint32_t)(key >> 32));
}
// -255 + #{n : u >= C[n]} over the non-decreasing thresholds
__device__ __forceinline__ int noise_of(const uint32_t* C, const uint32_t u) {
  int lo = 0, hi = kThresh;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (C[mid] <= u) lo = mid + 1; else hi = mid;
  }
  return lo - 255;
}
// the noise of the three bytes of pixel `pix` (= y * w + x): word idx & 3 of the counter idx >> 2, idx = pix (shared) or 3 * pix + c
__device__ __forceinline__ void noise_px(const vt_corrupt_frame& f, const uint32_t* C, const unsigned long long pix, int (&nz)[3]) {
  uint32_t c[4];
  if (!f.per_channel) {
    philox_at(f.key, pix >> 2, c);
    nz[0] = nz[1] = nz[2] = noise_of(C, word_of(c, (int)(pix & 3)));
    return;
  }
  const unsigned long long i0 = 3ull * pix, q0 = i0 >> 2, q1 = (i0 + 2) >> 2;
  uint32_t d[4];
  philox_at(f.key, q0, c);
  if (q1 != q0) philox_at(f.key, q1, d);
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const unsigned long long i = i0 + ch;
    nz[ch] = noise_of(C, (i >> 2) == q0 ? word_of(c, (int)(i & 3)) : word_of(d, (int)(i & 3)));
  }
}

// the 12 bytes at byte offset `o` of the staged tile -> three words (a[0] = bytes 0..3, ...)
__device__ __forceinline__ void lds_run(const uint32_t* px, const int o, uint32_t (&a)[3]) {
  const uint32_t* p = px + (o >> 2);
  const int sh = (o & 3) * 8;
  const uint32_t w0 = p[0], w1 = p[1], w2 = p[2], w3 = p[3];
  a[0] = (uint32_t)((((uint64_t)w1 << 32) | w0) >> sh);
  a[1] = (uint32_t)((((uint64_t)w2 << 32) | w1) >> sh);
  a[2] = (uint32_t)((((uint64_t)w3 << 32) | w2) >> sh);
}
__device__ __forceinline__ uint32_t byte_of(const uint32_t (&a)[3], const int j) { return (a[j >> 2] >> ((j & 3) * 8)) & 255u; }

__global__ void __launch_bounds__(kNT) corrupt_kernel(const vt_corrupt_frame* __restrict__ frames, const uint32_t* __restrict__ tables,
                                                      uint8_t* __restrict__ out) {
  __shared__ uint32_t px[kSide * kPitch / 4];
  __shared__ uint32_t C[kThresh + 2];
  const vt_corrupt_frame f = frames[blockIdx.y];
  const int tiles_x = (f.w + kTile - 1) / kTile, tiles_y = (f.h + kTile - 1) / kTile;
  if ((long)blockIdx.x >= (long)tiles_x * tiles_y) return;
  const int tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
  const int y0 = tile_y * kTile, x0 = tile_x * kTile;
  const bool noise = f.noise != VT_CORRUPT_NOISE_NONE, noise_first = f.order == VT_CORRUPT_NOISE_FIRST;
  const bool median = f.blur == VT_CORRUPT_BLUR_MEDIAN;
  const int r = f.blur == VT_CORRUPT_BLUR_NONE ? 0 : f.k >> 1;
  const int side = kTile + 2 * r;

  if (noise) {
    for (int i = threadIdx.x; i < kThresh; i += kNT) C[i] = tables[f.noise_off + i];
    __syncthreads();
  }
  // 1. stage
  uint8_t* pb = (uint8_t*)px;
  for (int p = threadIdx.x; p < side * side; p += kNT) {
    const int ly = p / side, lx = p - ly * side;
    const int gy = median ? clamp_index(y0 - r + ly, f.h) : mirror_index(y0 - r + ly, f.h);
    const int gx = median ? clamp_index(x0 - r + lx, f.w) : mirror_index(x0 - r + lx, f.w);
    const uint8_t* sp = (const uint8_t*)f.src + (long)gy * f.pitch + 3L * gx;
    int v0 = sp[0], v1 = sp[1], v2 = sp[2];
    if (noise && noise_first) {
      int nz[3];
      noise_px(f, C, (unsigned long long)gy * (unsigned)f.w + (unsigned)gx, nz);
      v0 = clip8(v0 + nz[0]); v1 = clip8(v1 + nz[1]); v2 = clip8(v2 + nz[2]);
    }
    uint8_t* dp = pb + ly * kPitch + lx * 3;
    dp[0] = (uint8_t)v0; dp[1] = (uint8_t)v1; dp[2] = (uint8_t)v2;
  }
  __syncthreads();

  // 2. blur: this thread's 12 bytes = pixels [tx, tx + 4) of row ty of the tile
  const int ty = threadIdx.x >> 3, tx = (threadIdx.x & 7) << 2;
  const int base = (ty + r) * kPitch + (tx + r) * 3;          // the thread's own run in the staged tile
  uint32_t val[12];
  if (f.blur == VT_CORRUPT_BLUR_NONE) {
    uint32_t a[3];
    lds_run(px, base, a);
#pragma unroll
    for (int j = 0; j < 12; ++j) val[j] = byte_of(a, j);
  } else if (median) {
    const int need = (f.k * f.k + 1) >> 1;                      // the median is the smallest v with #{p <= v} >= need
    uint32_t lo[12], hi[12];
#pragma unroll
    for (int j = 0; j < 12; ++j) { lo[j] = 0; hi[j] = 255; }
    for (int pass = 0; pass < 8; ++pass) {
      uint32_t mid[12], cnt[12];
#pragma unroll
      for (int j = 0; j < 12; ++j) { mid[j] = (lo[j] + hi[j]) >> 1; cnt[j] = 0; }
      for (int dy = -r; dy <= r; ++dy) {
        for (int dx = -r; dx <= r; ++dx) {
          uint32_t a[3];
          lds_run(px, base + dy * kPitch + dx * 3, a);
#pragma unroll
          for (int j = 0; j < 12; ++j) cnt[j] += byte_of(a, j) <= mid[j] ? 1u : 0u;
        }
      }
#pragma unroll
      for (int j = 0; j < 12; ++j) {
        if ((int)cnt[j] >= need) hi[j] = mid[j]; else lo[j] = mid[j] + 1;
      }
    }
#pragma unroll
    for (int j = 0; j < 12; ++j) val[j] = lo[j];
  } else {
    const int* taps = (const int*)tables + f.taps_off;
    uint32_t acc[12];
#pragma unroll
    for (int j = 0; j < 12; ++j) acc[j] = 0;
    for (int t = 0; t < f.ntaps; ++t) {
      const int dy = taps[3 * t], dx = taps[3 * t + 1];
      const uint32_t W = (uint32_t)taps[3 * t + 2];
      uint32_t a[3];
      lds_run(px, base + dy * kPitch + dx * 3, a);
#pragma unroll
      for (int j = 0; j < 12; ++j) acc[j] += W * byte_of(a, j);
    }
    const uint32_t D = f.tap_sum;
#pragma unroll
    for (int j = 0; j < 12; ++j) {                              // half to even on the exact remainder
      const uint32_t q = acc[j] / D, rem = acc[j] - q * D;
      val[j] = q + ((2ull * rem > D || (2ull * rem == D && (q & 1u))) ? 1u : 0u);
    }
  }

  // 3. epilogue
  const int y = y0 + ty, x = x0 + tx;
  if (y >= f.h || x >= f.w) return;
  const int npx = f.w - x < 4 ? f.w - x : 4;
  uint32_t o4[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    int v0 = (int)val[3 * j], v1 = (int)val[3 * j + 1], v2 = (int)val[3 * j + 2];
    if (noise && !noise_first && j < npx) {
      int nz[3];
      noise_px(f, C, (unsigned long long)y * (unsigned)f.w + (unsigned)(x + j), nz);
      v0 = clip8(v0 + nz[0]); v1 = clip8(v1 + nz[1]); v2 = clip8(v2 + nz[2]);
    }
    o4[j] = (uint32_t)v0 | ((uint32_t)v1 << 8) | ((uint32_t)v2 << 16);
  }
  store_px4(out + f.out_off + ((long)y * f.w + x) * 3, o4, npx);
}
}  // namespace

extern "C" int vt_corrupt(const vt_corrupt_frame* frames_host, const void* frames_dev, int n, const unsigned* tables_host, const void* tables_dev,
                          long table_words, void* out, vt_stream_t stream) {
  const char* fn = "vt_corrupt";
  CK(vt_frames_call_check(fn, frames_host, n, 0, 0));
  if (!frames_dev || !out) return vt_fail(VT_ERR_ARG, "%s: null device frame table or output", fn);
  if (table_words < 0 || table_words > INT_MAX || (table_words > 0 && (!tables_host || !tables_dev)))
    return vt_fail(VT_ERR_ARG, "%s: %ld table words with a null table", fn, table_words);
  long max_tiles = 1;
  for (int i = 0; i < n; ++i) {
    const vt_corrupt_frame& f = frames_host[i];
    CK(vt_frame_check(fn, f, i));
    const long tiles = (long)((f.h + kTile - 1) / kTile) * ((f.w + kTile - 1) / kTile);
    if (tiles > INT_MAX) return vt_fail(VT_ERR_ARG, "%s: frame %d of %d x %d is too large", fn, i, f.h, f.w);
    max_tiles = tiles > max_tiles ? tiles : max_tiles;
    if (f.order != VT_CORRUPT_NOISE_FIRST && f.order != VT_CORRUPT_BLUR_FIRST) return vt_fail(VT_ERR_ARG, "%s: frame %d: unknown order %d", fn, i, f.order);
    if (f.noise < VT_CORRUPT_NOISE_NONE || f.noise > VT_CORRUPT_NOISE_POISSON) return vt_fail(VT_ERR_ARG, "%s: frame %d: unknown noise kind %d", fn, i, f.noise);
    if (f.noise != VT_CORRUPT_NOISE_NONE) {
      if (f.noise_off < 0 || (long)f.noise_off + kThresh > table_words)
        return vt_fail(VT_ERR_ARG, "%s: frame %d: threshold table at %d lies outside the %ld table words", fn, i, f.noise_off, table_words);
      const unsigned* C = tables_host + f.noise_off;
      for (int k = 1; k < kThresh; ++k)
        if (C[k] < C[k - 1]) return vt_fail(VT_ERR_ARG, "%s: frame %d: threshold %d decreases", fn, i, k);
    }
    switch (f.blur) {
      case VT_CORRUPT_BLUR_NONE: break;
      case VT_CORRUPT_BLUR_MEDIAN:
        if (f.k < 3 || f.k > 11 || !(f.k & 1)) return vt_fail(VT_ERR_ARG, "%s: frame %d: median k = %d is not odd in 3..11", fn, i, f.k);
        break;
      case VT_CORRUPT_BLUR_GAUSSIAN: case VT_CORRUPT_BLUR_AVERAGE: case VT_CORRUPT_BLUR_MOTION: {
        const int kmax = 2 * kRmax + 1, r = f.k >> 1;
        if (f.blur == VT_CORRUPT_BLUR_AVERAGE ? (f.k < 2 || f.k > 7) : (f.k < 3 || f.k > kmax || !(f.k & 1)))
          return vt_fail(VT_ERR_ARG, "%s: frame %d: k = %d is even or out of range for blur kind %d", fn, i, f.k, f.blur);
        if (f.ntaps < 1) return vt_fail(VT_ERR_ARG, "%s: frame %d: empty tap list", fn, i);
        if (f.taps_off < 0 || f.ntaps > kmax * kmax || (long)f.taps_off + 3L * f.ntaps > table_words)
          return vt_fail(VT_ERR_ARG, "%s: frame %d: %d taps at %d lie outside the %ld table words", fn, i, f.ntaps, f.taps_off, table_words);
        const int* t = (const int*)tables_host + f.taps_off;
        unsigned long long D = 0;
        for (int k = 0; k < f.ntaps; ++k) {
          const int dy = t[3 * k], dx = t[3 * k + 1], W = t[3 * k + 2];
          if (dy < -r || dy > r || dx < -r || dx > r)
            return vt_fail(VT_ERR_ARG, "%s: frame %d: tap %d at (%d, %d) reaches beyond radius %d", fn, i, k, dy, dx, r);
          if (W < 1) return vt_fail(VT_ERR_ARG, "%s: frame %d: tap %d has weight %d", fn, i, k, W);
          D += (unsigned)W;
        }
        if (D == 0 || D > VT_CORRUPT_MAX_TAP_SUM || D != f.tap_sum)     // 255 * D fits uint32
          return vt_fail(VT_ERR_ARG, "%s: frame %d: taps sum to %llu, the record says %u (1 .. 2^24)", fn, i, D, f.tap_sum);
        break;
      }
      default: return vt_fail(VT_ERR_ARG, "%s: frame %d: unknown blur kind %d", fn, i, f.blur);
    }
  }
  hipLaunchKernelGGL(corrupt_kernel, dim3((unsigned)max_tiles, n), dim3(kNT), 0, (hipStream_t)stream, (const vt_corrupt_frame*)frames_dev,
                     (const uint32_t*)tables_dev, (uint8_t*)out);
  return vt_frames_launched(fn);
}
