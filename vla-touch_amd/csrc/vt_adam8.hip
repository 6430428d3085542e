// vt_adam8.hip — AdamW with block-wise 8-bit moments for the RDT fine-tuning step (stands where the reference passes --use_8bit_adam:
// finetune.sh:55, train/train.py:216-237, bnb.optim.AdamW8bit).  The dynamic block-wise quantisation of Dettmers et al., "8-bit Optimizers via
// Block-wise Quantization": a moment is a uint8 code into a 256-entry table times one fp32 scale per block of 256 consecutive elements.  The
// arithmetic is the statement of DESIGN.md §8 (tests/adam8_ref.py is its numpy form); it is UNPINNED against bitsandbytes.
//   tables (device, 1024 fp32, vlatouch/adam8.py): T_s[256] | T_u[256] | B_s[256] | B_u[256], B[j] = fp32(((double)T[j] + T[j+1]) / 2), B[255] = +inf
//   code(x) = the number of B[j] strictly below x = the index of the nearest table value, ties to the lower index
// The element update is adamw_elem / ema_elem of vt_optim.h, so a tensor kept in fp32 (aux pair null) gets the bits of
// vt_adamw_ema_multi, and so does every tensor on the first step, where the dequantised state is exactly zero.
// HBM-bound by design: 24 B per parameter (p 8, g 4, codes 2 + 2, shadow 8) against vt_adamw_ema_multi's 36 B; no MFMA.
#include <math.h>
#include "vt_common.h"
#include "vt_host.h"
#include "vt_optim.h"
#include "../../include/vlatouch.h"

namespace {

// the table of vt_adamw_ema_multi (vt_optim.h); a row's m / v point at `unsigned char` codes where aux[k] is not null, at fp32 moments where it is
static_assert(4 * 4 * 256 == MT_CHUNK, "4 passes of 4 waves, one 256-element quantisation block each, walk one chunk");
struct AuxEntry { float* am; float* av; };

// The code search.  The tables are decade-structured: decade d = 0 .. 6 holds the midpoints of n_d equal sub-intervals of [0.1, 1] x 10^(d-6),
// n_d = 2^d (signed, per sign) or 2^(d+1) (unsigned), so the sub-interval edges are the decision boundaries inside a decade and the index
// of a = |x| follows from the decade and one multiply-add.  Two small look-up tables in LDS replace a compare per power of ten:
//   le[s][b], b = the binade of a (2^(b-24) <= a < 2^(b-23), everything smaller in b = 0): {thr, j0}.  The thresholds are the first positive
//             boundary and the six boundaries between decades (just above 1e-6 .. 1e-1); at most one falls into a binade (thr, +inf if none), j0 of them lie below it, so row j = j0 + (a >= thr)
//   ld[s][j]: {A, C, base, kmax}: j = 0 is "below the first boundary" (index `base`), j = d + 1 is decade d: index = base + clamp((int)(a A - C), 0, kmax)
// (s = 0 signed, counted from index 127; s = 1 unsigned).  The guess can be off by one by rounding next to a sub-interval edge and between the last decade and 1, so `code_fix` reads the two boundaries around it, both at once, and
// moves one step if one of them says so; only then does it go on comparing.  Whatever the guess, the result is exactly the count of
// boundaries below x; an 8-step binary search would be 8 dependent LDS reads per code instead.
struct Luts { float2 le[2][32]; float4 ld[2][8]; };
__device__ __forceinline__ void build_luts(Luts& L, const float* __restrict__ tables, int t) {   // t = threadIdx.x of a block of >= 80 threads; a barrier follows
  if (t < 64) {
    const int s = t >> 5, b = t & 31;
    if (b < 25) {
      float p10[7];                                          // the boundary below each row's first index: the first positive one, then the six between decades
#pragma unroll
      for (int i = 0; i < 7; ++i) p10[i] = tables[s ? 768 + (i ? (2 << i) - 2 : 0) : 512 + (i ? 126 + (1 << i) : 127)];
      const float lo = b ? ldexpf(1.0f, b - 24) : 0.0f, hi = ldexpf(1.0f, b - 23);
      float thr = INFINITY;
      int j0 = 0;
#pragma unroll
      for (int i = 0; i < 7; ++i) {
        if (p10[i] < lo) ++j0;
        else if (p10[i] < hi) thr = p10[i];
      }
      L.le[s][b] = make_float2(thr, __int_as_float(j0));
    }
  } else if (t < 80) {
    const int s = (t >> 3) & 1, j = t & 7;
    const float sc[7] = {1e6f, 1e5f, 1e4f, 1e3f, 1e2f, 1e1f, 1.0f};
    float A = 0.0f, C = 0.0f;
    int base = s ? 0 : 127, n = 0;
    if (j) {
      n = 1 << (j - 1 + s);
      float scd = 1.0f;
#pragma unroll
      for (int i = 0; i < 7; ++i) scd = i == j - 1 ? sc[i] : scd;
      A = scd * ((float)n * 1.1111112f);
      C = 0.1f * ((float)n * 1.1111112f);
      base = s ? n - 1 : 127 + n;
    }
    L.ld[s][j] = make_float4(A, C, __int_as_float(base), __int_as_float(j == 7 ? n : n ? n - 1 : 0));   // only the last decade steps up, to the entry 1
  }
}
__device__ __forceinline__ int guess_pos(const Luts& L, int s, float a) {         // a >= 0; always inside 0 .. 255 (s = 1) or 127 .. 255 (s = 0), NaN included
  int b = (int)(__float_as_uint(a) >> 23) - 103;
  b = b < 0 ? 0 : (b > 24 ? 24 : b);
  const float2 t = L.le[s][b];
  const float4 c = L.ld[s][__float_as_int(t.y) + (a >= t.x ? 1 : 0)];
  const int kmax = __float_as_int(c.w);
  int k = (int)fmaf(a, c.x, -c.y);
  k = k < 0 ? 0 : (k > kmax ? kmax : k);
  return __float_as_int(c.z) + k;
}
__device__ __forceinline__ int code_fix(const float* __restrict__ B, float x, int idx) {
  const float below = B[idx > 0 ? idx - 1 : 0], at = B[idx];
  if (at < x) {
    ++idx;
    while (B[idx] < x) ++idx;                                 // B[255] = +inf ends it
  } else if (idx > 0 && below >= x) {
    --idx;
    while (idx > 0 && B[idx - 1] >= x) --idx;
  }
  return idx;                                                 // a NaN x keeps the guess
}
__device__ __forceinline__ int code_u(const Luts& L, const float* __restrict__ B, float x) { return code_fix(B, x, guess_pos(L, 1, x)); }   // x in [0, 1]
__device__ __forceinline__ int code_s(const Luts& L, const float* __restrict__ B, float x) {                                                // x in [-1, 1]
  const int pos = guess_pos(L, 0, fabsf(x));                  // 127 .. 255
  const int neg = 254 - pos;                                  // the table has no -1: the mirror of index 255 is clamped to 0
  return code_fix(B, x, x < 0.0f ? (neg < 0 ? 0 : neg) : pos);
}

// x / d of the statement for a whole block with one reciprocal: given r = 1.0f / d, correctly rounded, two residual corrections give the
// correctly rounded quotient (Markstein: a faithful q corrected by (x - q d) r rounds to the nearest, and the first correction makes q
// faithful).  The residuals must be exact: with |x| <= d, d >= 2^-60 and a quotient of at least 2^-23 (every decision boundary is above
// 1.6e-7 > 2^-23, so a smaller quotient has code 127 / 0 whatever its last bit) they stay far above the subnormals.
#define VT_ADAM8_MIN_SCALE 8.6736174e-19f                    /* 2^-60; a smaller (or zero) scale takes the plain division */
__device__ __forceinline__ float div_by(float x, float d, float r) {
  float q = x * r;
  q = fmaf(fmaf(-q, d, x), r, q);
  return fmaf(fmaf(-q, d, x), r, q);
}

// A 256-thread block takes one MT_CHUNK-element chunk of one tensor (mt_find, as vt_adamw_ema_multi does): 16
// quantisation blocks of 256 elements, none of which straddles a chunk.  A wave takes one block per iteration, 4 consecutive elements per
// lane: one 32-bit word of each code array and 128-bit words of p / g / shadow where every base is aligned for them (a block starts 1 KiB
// into p, 256 B into the codes, so the tensor's alignment is the block's); an unaligned tensor and the last partial block go element by
// element.  The two block maxima are wave-local DPP / permlane reductions (no LDS, no barrier; a maximum does not depend on the order, so
// the scales are reproducible).  LDS holds the 4 KiB of tables, loaded once per chunk (4 % on top of the chunk's 96 KiB of traffic, from L2), and the 768 B of the guess's look-up tables.
__global__ __launch_bounds__(256) void adamw8_ema_mt_kernel(const MtEntry* __restrict__ tab, const AuxEntry* __restrict__ aux, const float* __restrict__ tables,
                                                            int ntensors, const float* __restrict__ hyper, float b1, float b2, float eps, float wd) {
  __shared__ __attribute__((aligned(16))) float tb[1024];
  __shared__ Luts lut;
  const long chunk = blockIdx.x;
  const int row = mt_find(tab, ntensors, chunk);
  const MtEntry e = tab[row];
  const AuxEntry ax = aux[row];
  const long base = (chunk - e.first_chunk) * MT_CHUNK;
  const float lr = hyper[0], bc1 = hyper[1], bc2_sqrt = hyper[2], omd = hyper[3];
  if (!ax.am) {                                               // fp32 moments: the chunk body of vt_train.hip's adamw_ema_mt_kernel
    adamw_ema_chunk_f32(e.p, e.g, e.m, e.v, e.shadow, base, e.n, lr, b1, b2, eps, wd, bc1, bc2_sqrt, omd);
    return;
  }
  reinterpret_cast<float4*>(tb)[threadIdx.x] = reinterpret_cast<const float4*>(tables)[threadIdx.x];
  build_luts(lut, tables, threadIdx.x);
  __syncthreads();
  const float* Ts = tb;
  const float* Tu = tb + 256;
  const float* Bs = tb + 512;
  const float* Bu = tb + 768;
  unsigned char* __restrict__ m8 = (unsigned char*)e.m;
  unsigned char* __restrict__ v8 = (unsigned char*)e.v;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const bool vec = ((((size_t)e.p | (size_t)e.g | (size_t)e.shadow) & 15) == 0) && ((((size_t)m8 | (size_t)v8) & 3) == 0);
  const int j0 = lane * 4;
#pragma unroll 1
  for (int it = 0; it < 4; ++it) {
    const long off = base + (long)(it * 4 + wv) * 256;        // this wave's block; everything up to the stores is wave-uniform control flow
    if (off >= e.n) break;
    const long left = e.n - off;
    const int cnt = left < 256 ? (int)left : 256;
    const bool full = vec && cnt == 256;
    const long bi = off >> 8;
    float pv[4], gv[4], sv[4], mn[4], vn[4];
    int cm[4], cv[4];
    if (full) {
      const float4 P = *reinterpret_cast<const float4*>(e.p + off + j0);
      const float4 G = *reinterpret_cast<const float4*>(e.g + off + j0);
      const unsigned wm = *reinterpret_cast<const unsigned*>(m8 + off + j0), wq = *reinterpret_cast<const unsigned*>(v8 + off + j0);
      pv[0] = P.x; pv[1] = P.y; pv[2] = P.z; pv[3] = P.w;
      gv[0] = G.x; gv[1] = G.y; gv[2] = G.z; gv[3] = G.w;
#pragma unroll
      for (int j = 0; j < 4; ++j) { cm[j] = (int)((wm >> (8 * j)) & 255u); cv[j] = (int)((wq >> (8 * j)) & 255u); sv[j] = 0.0f; }
      if (e.shadow) {
        const float4 S = *reinterpret_cast<const float4*>(e.shadow + off + j0);
        sv[0] = S.x; sv[1] = S.y; sv[2] = S.z; sv[3] = S.w;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool act = j0 + j < cnt;
        const long i = off + j0 + j;
        pv[j] = act ? e.p[i] : 0.0f;
        gv[j] = act ? e.g[i] : 0.0f;
        sv[j] = act && e.shadow ? e.shadow[i] : 0.0f;
        cm[j] = act ? (int)m8[i] : 127;
        cv[j] = act ? (int)v8[i] : 0;
      }
    }
    const float am = ax.am[bi], av = ax.av[bi];
    float mx = 0.0f, vx = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float mo = Ts[cm[j]] * am, vo = Tu[cv[j]] * av;
      pv[j] = adamw_elem(pv[j], gv[j], mo, vo, lr, b1, b2, eps, wd, bc1, bc2_sqrt);
      sv[j] = ema_elem(sv[j], pv[j], omd);
      mn[j] = mo; vn[j] = vo;
      if (j0 + j < cnt) { mx = fmaxf(mx, fabsf(mo)); vx = fmaxf(vx, vo); }
    }
    mx = wave_max(mx);
    vx = wave_max(vx);
    unsigned wm = 0, wq = 0;
    if (mx >= VT_ADAM8_MIN_SCALE && vx >= VT_ADAM8_MIN_SCALE) {                  // wave-uniform: every lane holds the block's maxima
      const float rm = 1.0f / mx, rv = 1.0f / vx;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        wm |= (unsigned)code_s(lut, Bs, div_by(mn[j], mx, rm)) << (8 * j);
        wq |= (unsigned)code_u(lut, Bu, div_by(vn[j], vx, rv)) << (8 * j);
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        wm |= (unsigned)(mx == 0.0f ? 127 : code_s(lut, Bs, mn[j] / mx)) << (8 * j);
        wq |= (unsigned)(vx == 0.0f ? 0 : code_u(lut, Bu, vn[j] / vx)) << (8 * j);
      }
    }
    if (full) {
      *reinterpret_cast<float4*>(e.p + off + j0) = make_float4(pv[0], pv[1], pv[2], pv[3]);
      if (e.shadow) *reinterpret_cast<float4*>(e.shadow + off + j0) = make_float4(sv[0], sv[1], sv[2], sv[3]);
      *reinterpret_cast<unsigned*>(m8 + off + j0) = wm;
      *reinterpret_cast<unsigned*>(v8 + off + j0) = wq;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j0 + j < cnt) {
          const long i = off + j0 + j;
          e.p[i] = pv[j];
          if (e.shadow) e.shadow[i] = sv[j];
          m8[i] = (unsigned char)(wm >> (8 * j));
          v8[i] = (unsigned char)(wq >> (8 * j));
        }
      }
    }
    if (lane == 0) { ax.am[bi] = mx; ax.av[bi] = vx; }
  }
}

// the block rule alone: a wave per 256-element block, the table's boundaries in LDS
__global__ __launch_bounds__(256) void adam8_quantize_kernel(const float* __restrict__ x, unsigned char* __restrict__ codes, float* __restrict__ absmax,
                                                             const float* __restrict__ tables, int sgn, long n) {
  __shared__ float B[256];
  __shared__ Luts lut;
  B[threadIdx.x] = tables[(sgn ? 512 : 768) + threadIdx.x];
  build_luts(lut, tables, threadIdx.x);
  __syncthreads();
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long blk = (long)blockIdx.x * 4 + wv, off = blk * 256;
  if (off >= n) return;                                       // wave-uniform, behind the barrier
  float xv[4], mx = 0.0f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const long i = off + lane * 4 + j;
    xv[j] = i < n ? x[i] : 0.0f;
    mx = fmaxf(mx, sgn ? fabsf(xv[j]) : xv[j]);
  }
  mx = wave_max(mx);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const long i = off + lane * 4 + j;
    if (i < n) codes[i] = (unsigned char)(sgn ? (mx == 0.0f ? 127 : code_s(lut, B, xv[j] / mx)) : (mx == 0.0f ? 0 : code_u(lut, B, xv[j] / mx)));
  }
  if (lane == 0) absmax[blk] = mx;
}
__global__ void adam8_dequantize_kernel(const unsigned char* __restrict__ codes, const float* __restrict__ absmax, const float* __restrict__ tables, int sgn,
                                        float* __restrict__ out, long n) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = tables[(sgn ? 0 : 256) + codes[i]] * absmax[i >> 8];
}

}  // namespace

int vt_adamw8_ema_multi(const void* table, const void* aux, const float* tables, int ntensors, long total_chunks, const float* hyper, float beta1, float beta2,
                        float eps, float weight_decay, vt_stream_t s) {
  if (!table || !aux || !tables || !hyper || ntensors < 1 || total_chunks < 1) return vt_fail(VT_ERR_ARG, "vt_adamw8_ema_multi: bad argument");
  if ((size_t)tables & 15) return vt_fail(VT_ERR_ARG, "vt_adamw8_ema_multi: tables must be 16-byte aligned");
  hipLaunchKernelGGL(adamw8_ema_mt_kernel, dim3((unsigned)total_chunks), dim3(256), 0, (hipStream_t)s, (const MtEntry*)table, (const AuxEntry*)aux, tables,
                     ntensors, hyper, beta1, beta2, eps, weight_decay);
  return vt_check_launch();
}
int vt_adam8_quantize(const float* x, unsigned char* codes, float* absmax, const float* tables, int signed_table, long n, vt_stream_t s) {
  if (!x || !codes || !absmax || !tables || n < 1) return vt_fail(VT_ERR_ARG, "vt_adam8_quantize: bad argument");
  hipLaunchKernelGGL(adam8_quantize_kernel, dim3((unsigned)((n + 1023) / 1024)), dim3(256), 0, (hipStream_t)s, x, codes, absmax, tables, signed_table ? 1 : 0, n);
  return vt_check_launch();
}
int vt_adam8_dequantize(const unsigned char* codes, const float* absmax, const float* tables, int signed_table, float* out, long n, vt_stream_t s) {
  if (!codes || !absmax || !tables || !out || n < 1) return vt_fail(VT_ERR_ARG, "vt_adam8_dequantize: bad argument");
  hipLaunchKernelGGL(adam8_dequantize_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)s, codes, absmax, tables, signed_table ? 1 : 0, out, n);
  return vt_check_launch();
}
