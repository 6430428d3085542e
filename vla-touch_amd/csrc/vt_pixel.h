// vt_pixel.h — the pixel idioms of the camera-frame kernels (vt_imgprep.hip, vt_colorjitter.hip, vt_jpegmap.hip, vt_jpegdec.hip), stated once: the byte clip,
// the brightness lift and its decision, the luma weights, four RGB pixels as three aligned words, and the per-block tail of an exact sum.
// Integer arithmetic throughout, but for the lift decision: one quotient of products in double, no sum in it, so there is nothing a
// floating-point contraction could fuse (vt_colorjitter.hip turns contraction off for its own expressions, behind its includes).
#pragma once
#include <stdint.h>

__device__ __forceinline__ int clip8(const int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }
// ImageEnhance.Brightness(1.75) against black: min(255, (int)(1.75f * v)); 1.75f * v is exact, so the truncation is (7 v) >> 2
__device__ __forceinline__ int lift8(const int v) { const int t = (v * 7) >> 2; return t > 255 ? 255 : t; }
// whether a frame of byte sum `sum` takes the lift: the host's test, in double: sum / (h * w * 255.0 * 3) <= 0.15
__device__ __forceinline__ bool lift_decision(const unsigned long long sum, const int h, const int w) {
  return (double)sum / ((double)((long)h * w) * 255.0 * 3.0) <= 0.15;
}
// ITU-R 601 luma in 16-bit fixed point, rounded: PIL's convert("L"), and libjpeg's Y (jccolor.c)
__device__ __forceinline__ int luma8(const int r, const int g, const int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }

// four pixels = 12 bytes at a 4-byte aligned `sp` -> px[j] = r | g << 8 | b << 16, through three word loads
__device__ __forceinline__ void load_px4(const uint8_t* sp, uint32_t px[4]) {
  const uint32_t a = ((const uint32_t*)sp)[0], b = ((const uint32_t*)sp)[1], c = ((const uint32_t*)sp)[2];
  px[0] = a & 0xffffffu;
  px[1] = (a >> 24) | ((b & 0xffffu) << 8);
  px[2] = (b >> 16) | ((c & 0xffu) << 16);
  px[3] = c >> 8;
}
// the inverse: px[0 .. npx) to `dp`, three word stores where all four are there and dp is 4-byte aligned, bytes otherwise
__device__ __forceinline__ void store_px4(uint8_t* dp, const uint32_t px[4], const int npx) {
  if (npx == 4 && ((uintptr_t)dp & 3) == 0) {
    ((uint32_t*)dp)[0] = px[0] | (px[1] << 24);
    ((uint32_t*)dp)[1] = (px[1] >> 8) | (px[2] << 16);
    ((uint32_t*)dp)[2] = (px[2] >> 16) | (px[3] << 8);
  } else {
    for (int j = 0; j < npx; ++j) {
      dp[3 * j] = (uint8_t)px[j]; dp[3 * j + 1] = (uint8_t)(px[j] >> 8); dp[3 * j + 2] = (uint8_t)(px[j] >> 16);
    }
  }
}

// The tail of a sum kernel of 256 threads: K per-thread totals -> one uint64 partial per block and sum, slot[k * stride].  Every slot is
// rewritten by every call: nothing to zero beforehand, no atomics.
template <int K>
__device__ __forceinline__ void block_sums_store(const unsigned long long (&tot)[K], unsigned long long* slot, const long stride) {
  __shared__ unsigned long long part[K][4];
  for (int k = 0; k < K; ++k) {
    unsigned long long v = tot[k];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if ((threadIdx.x & 63) == 0) part[k][threadIdx.x >> 6] = v;
  }
  __syncthreads();
  if (threadIdx.x < K) slot[threadIdx.x * stride] = part[threadIdx.x][0] + part[threadIdx.x][1] + part[threadIdx.x][2] + part[threadIdx.x][3];
}
