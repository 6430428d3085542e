// vt_train_rdt.hip — backward arithmetic of the RDT fine-tuning step (VLA/train/train.py:404-448, RDTRunner.compute_loss
// models/rdt_runner.py:168-222): what the forward primitives and csrc/vt_train.hip do not already provide to differentiate an RDT block
// and to clip its gradients.  Every Linear of the step (forward, data gradient, weight gradient) stays a vt_gemm call; the kernels here are
//   * attention backward with recomputed probabilities (no stored P, no floating-point atomics: bit-reproducible),
//   * RMSNorm / per-head RMSNorm backward in both timm forms (vt_rownorm modes 1 and 2),
//   * tanh-GELU / SiLU and their derivatives on libm functions (gradients are not the place for the ~1 ulp shortcuts of the epilogues),
//   * the DDPM forward process written into the state ‖ noisy-action ‖ mask token layout, the sinusoidal timestep embedding,
//   * global-norm gradient clipping over the multi-tensor table vt_adamw_ema_multi reads, gradient accumulation into that table and the bf16
//     pack / unpack of the data-parallel gradient exchange,
//   * a zero-padding transpose (the weight-gradient products reduce over the token count, which vt_gemm wants as a multiple of 4 / 8),
//   * dtype-typed column sum / add / column copy for the bf16 mode (the helpers of vt_train.hip are fp32 only).
// A wave owns one query row (dQ) or one key row (dK, dV) with lane = head-dim element (head_dim 64 = the wave width), so every sum has a
// fixed order.  These are fp32 VALU kernels with one wave reduction per (query, key) pair: correct and reproducible, not fast — at RDT-1B size
// the two attention-backward kernels are 40 % of the fp32 step's kernel time and 65 % of the bf16 step's (profiles/rdt_train_kernels*.txt), almost all of it the 4 374-key image
// cross-attention.  The MFMA tile for that case exists beside them: vt_attention_bwd_mfma (csrc/vt_attn_bwd.hip; bf16 only, at most 128 query rows,
// P and dS rounded to bf16), which the trainer takes with attention_backward="mfma".  These kernels stay the default, the fp32-P statement and the
// only fp32 path.
#include <math.h>
#include "vt_common.h"
#include "vt_host.h"
#include "vt_optim.h"
#include "../../include/vlatouch.h"

namespace {

inline dim3 g1(long n) { return dim3((unsigned)((n + 255) / 256)); }

// ------------------------------------------------------------------------------------------------ attention backward
// Pass 1 + dQ: one wave per (b, h, query row i).  Online softmax statistics over the keys give m_i (row max), 1 / l_i and
// delta_i = sum_j P_ij dP_ij (dP_ij = dO_i . v_j); they are written to ws[(b, h, i)][3] for the dK / dV kernel, then a second walk over
// the keys accumulates dQ_i = scale * sum_j P_ij (dP_ij - delta_i) k_j.  A row whose keys are all masked gets m = 0, 1 / l = 0: P = 0.
template <typename T>
__global__ __launch_bounds__(256) void attn_bwd_dq_kernel(VtAttnBwdParams p) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long row = (long)blockIdx.x * 4 + wv;                 // (b * H + h) * Nq + i
  const long rows = (long)p.B * p.H * p.Nq;
  if (row >= rows) return;                                     // whole wave leaves together
  const int i = (int)(row % p.Nq);
  const long bh = row / p.Nq;
  const int h = (int)(bh % p.H), b = (int)(bh / p.H);
  const T* q = (const T*)p.Q + (long)b * p.q_bs + (long)i * p.q_rs + (long)h * p.q_hs;
  const T* go = (const T*)p.dO + (long)b * p.do_bs + (long)i * p.do_rs + (long)h * p.do_hs;
  const T* kb = (const T*)p.K + (long)b * p.k_bs + (long)h * p.k_hs;
  const T* vb = (const T*)p.V + (long)b * p.v_bs + (long)h * p.v_hs;
  const unsigned char* km = p.kmask ? p.kmask + (long)b * p.km_bs : nullptr;
  const float qd = ldf<T>(q, lane) * p.scale, gd = ldf<T>(go, lane);
  float m = -INFINITY, l = 0.f, acc = 0.f;
  for (int j = 0; j < p.Nk; ++j) {
    if (km && !km[j]) continue;                                // uniform over the wave
    const float s = wave_sum(qd * ldf<T>(kb + (long)j * p.k_rs, lane));
    const float dp = wave_sum(gd * ldf<T>(vb + (long)j * p.v_rs, lane));
    const float mn = fmaxf(m, s);
    const float c = expf(m - mn), e = expf(s - mn);            // first key: m = -inf -> c = 0
    l = l * c + e;
    acc = acc * c + e * dp;
    m = mn;
  }
  const float inv_l = l > 0.f ? 1.0f / l : 0.f;
  if (!(l > 0.f)) m = 0.f;
  const float delta = acc * inv_l;
  if (lane == 0) { float* w = p.ws + row * 3; w[0] = m; w[1] = inv_l; w[2] = delta; }
  float dq = 0.f;
  for (int j = 0; j < p.Nk; ++j) {
    if (km && !km[j]) continue;
    const float kd = ldf<T>(kb + (long)j * p.k_rs, lane);
    const float s = wave_sum(qd * kd);
    const float dp = wave_sum(gd * ldf<T>(vb + (long)j * p.v_rs, lane));
    const float pr = expf(s - m) * inv_l;
    dq += pr * (dp - delta) * kd;
  }
  stf<T>((T*)p.dQ + (long)b * p.dq_bs + (long)i * p.dq_rs + (long)h * p.dq_hs, lane, dq * p.scale);
}

// dK, dV: one wave per (b, h, key j), walking the query rows with the statistics of the kernel above:
//   dV_j = sum_i P_ij dO_i,  dK_j = scale * sum_i P_ij (dP_ij - delta_i) q_i.   A masked key gets zeros.
template <typename T>
__global__ __launch_bounds__(256) void attn_bwd_dkv_kernel(VtAttnBwdParams p) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int j = blockIdx.x * 4 + wv;
  if (j >= p.Nk) return;
  const int h = blockIdx.y % p.H, b = blockIdx.y / p.H;
  const bool live = !(p.kmask && !p.kmask[(long)b * p.km_bs + j]);
  const float kd = ldf<T>((const T*)p.K + (long)b * p.k_bs + (long)j * p.k_rs + (long)h * p.k_hs, lane);
  const float vd = ldf<T>((const T*)p.V + (long)b * p.v_bs + (long)j * p.v_rs + (long)h * p.v_hs, lane);
  const T* qb = (const T*)p.Q + (long)b * p.q_bs + (long)h * p.q_hs;
  const T* gb = (const T*)p.dO + (long)b * p.do_bs + (long)h * p.do_hs;
  const float* ws = p.ws + ((long)b * p.H + h) * p.Nq * 3;
  float dk = 0.f, dv = 0.f;
  if (live) {
    for (int i = 0; i < p.Nq; ++i) {
      const float qd = ldf<T>(qb + (long)i * p.q_rs, lane), gd = ldf<T>(gb + (long)i * p.do_rs, lane);
      const float s = wave_sum(qd * kd) * p.scale;
      const float dp = wave_sum(gd * vd);
      const float pr = expf(s - ws[i * 3]) * ws[i * 3 + 1];
      dv += pr * gd;
      dk += pr * (dp - ws[i * 3 + 2]) * qd;
    }
  }
  stf<T>((T*)p.dK + (long)b * p.dk_bs + (long)j * p.dk_rs + (long)h * p.dk_hs, lane, dk * p.scale);
  stf<T>((T*)p.dV + (long)b * p.dv_bs + (long)j * p.dv_rs + (long)h * p.dv_hs, lane, dv);
}

// ------------------------------------------------------------------------------------------------ RMSNorm backward
// y = x r w with r = rsqrt(v + eps); mode 1: v = mean(x^2); mode 2: v = sum (x - mean)^2 / (D - 1)  (timm <= 1.0.8).  With g = dy w:
//   mode 1: dx = r g - r^3 <g, x> x / D          mode 2: dx = r g - r^3 <g, x> (x - mean) / (D - 1)
// One block per row.  dyxr (fp32) = dy x r, whose column sums are d w (vt_colsum finishes, as after vt_ln_bwd).
// Every element-wise kernel below is typed on the activation type T (fp32, or bf16 / fp16 storage with fp32 arithmetic and one rounding at the store).
__device__ __forceinline__ float block_sum4(float t, float* red) {
  t = wave_sum(t);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = t;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}
template <typename T>
__global__ __launch_bounds__(256) void rmsnorm_bwd_kernel(const T* __restrict__ x, const float* __restrict__ w, const T* __restrict__ dy,
                                                          T* __restrict__ dx, float* __restrict__ dyxr, int D, float eps, int mode) {
  __shared__ float red[4];
  const long base = (long)blockIdx.x * D;
  float s1 = 0.f, s2 = 0.f;
  for (int c = threadIdx.x; c < D; c += 256) { const float v = ldf<T>(x, base + c); s1 += v; s2 += v * v; }
  float mean = 0.f, var;
  if (mode == 2) {
    mean = block_sum4(s1, red) / (float)D;
    float q = 0.f;
    for (int c = threadIdx.x; c < D; c += 256) { const float d = ldf<T>(x, base + c) - mean; q += d * d; }
    var = block_sum4(q, red) / (float)(D - 1);
  } else {
    var = block_sum4(s2, red) / (float)D;
  }
  const float r = rsqrtf(var + eps);
  float gx = 0.f;
  for (int c = threadIdx.x; c < D; c += 256) gx += ldf<T>(dy, base + c) * w[c] * ldf<T>(x, base + c);
  const float k = block_sum4(gx, red) * r * r * r / (float)(mode == 2 ? D - 1 : D);
  for (int c = threadIdx.x; c < D; c += 256) {
    const float xv = ldf<T>(x, base + c), dv = ldf<T>(dy, base + c);
    stf<T>(dx, base + c, r * dv * w[c] - k * (xv - mean));
    dyxr[base + c] = dv * xv * r;
  }
}

// The same over 64-wide head slices: x (pre-norm) and dy (overwritten by dx) live at [token * stride + head * 64 + lane].  A block takes 64
// consecutive (token, head) pairs, 16 per wave; lane d keeps d w[d] of its pairs, the four waves are added in a fixed order into
// part[block][64] (vt_colsum finishes).
template <typename T>
__global__ __launch_bounds__(256) void headnorm_bwd_kernel(const T* __restrict__ x, long x_stride, T* __restrict__ dy, long dy_stride, int heads,
                                                           long pairs, const float* __restrict__ w, float* __restrict__ part, float eps, int mode) {
  __shared__ float red[4][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const float wd = w[lane];
  float dw = 0.f;
  for (int it = 0; it < 16; ++it) {
    const long pr = (long)blockIdx.x * 64 + wv * 16 + it;
    if (pr >= pairs) break;
    const long tok = pr / heads;
    const int hh = (int)(pr - tok * heads);
    const float xv = ldf<T>(x, tok * x_stride + hh * 64 + lane);
    const long di = tok * dy_stride + hh * 64 + lane;
    const float dv = ldf<T>(dy, di);
    float mean = 0.f, var;
    if (mode == 2) {
      mean = wave_sum(xv) * (1.0f / 64.0f);
      const float d = xv - mean;
      var = wave_sum(d * d) * (1.0f / 63.0f);
    } else {
      var = wave_sum(xv * xv) * (1.0f / 64.0f);
    }
    const float r = rsqrtf(var + eps);
    const float k = wave_sum(dv * wd * xv) * r * r * r * (mode == 2 ? 1.0f / 63.0f : 1.0f / 64.0f);
    stf<T>(dy, di, r * dv * wd - k * (xv - mean));
    dw += dv * xv * r;
  }
  red[wv][lane] = dw;
  __syncthreads();
  if (wv == 0) part[(long)blockIdx.x * 64 + lane] = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
}

// ------------------------------------------------------------------------------------------------ activations
__device__ __forceinline__ void gelu_tanh_fd(float x, float& y, float& d) {     // timm Mlp / adaptor GELU(approximate="tanh")
  const float c = 0.7978845608028654f, a = 0.044715f;
  const float t = tanhf(c * (x + a * x * x * x));
  y = 0.5f * x * (1.0f + t);
  d = 0.5f * (1.0f + t) + 0.5f * x * (1.0f - t * t) * c * (1.0f + 3.0f * a * x * x);
}
__device__ __forceinline__ void silu_fd(float x, float& y, float& d) {          // TimestepEmbedder nn.SiLU
  const float s = 1.0f / (1.0f + expf(-x));
  y = x * s;
  d = s * (1.0f + x * (1.0f - s));
}
template <typename T>
__global__ void act_kernel(const T* __restrict__ x, const T* __restrict__ dy, T* __restrict__ out, long n, int act) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float y, d;
  if (act == VT_ACT_SILU) silu_fd(ldf<T>(x, i), y, d); else gelu_tanh_fd(ldf<T>(x, i), y, d);
  stf<T>(out, i, dy ? ldf<T>(dy, i) * d : y);
}

// ------------------------------------------------------------------------------------------------ DDPM forward process + token layout
// out [B][horizon + 1][2A]: row 0 = state ‖ mask, row 1 + r = (sqrt(ab_t) a_r + sqrt(1 - ab_t) eps_r) ‖ mask   (rdt_runner.py:197-204,
// DDPMScheduler.add_noise); ab = alphas_cumprod [T] fp32, t [B] int64 (clamped into the table).
template <typename T>
__global__ void ddpm_qsample_kernel(const float* __restrict__ state, const float* __restrict__ action, const float* __restrict__ noise,
                                    const float* __restrict__ mask, const long* __restrict__ t, const float* __restrict__ ab, int Tn,
                                    T* __restrict__ out, int B, int horizon, int A) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const long per = (long)(horizon + 1) * 2 * A;
  if (i >= (long)B * per) return;
  const int b = (int)(i / per);
  const long e = i - (long)b * per;
  const int r = (int)(e / (2 * A)), c = (int)(e - (long)r * 2 * A);
  float v;
  if (c >= A) v = mask[(long)b * A + c - A];
  else if (r == 0) v = state[(long)b * A + c];
  else {
    long tt = t[b];
    tt = tt < 0 ? 0 : (tt >= Tn ? Tn - 1 : tt);
    const float a = ab[tt];
    const long k = ((long)b * horizon + r - 1) * A + c;
    v = sqrtf(a) * action[k] + sqrtf(1.0f - a) * noise[k];
  }
  stf<T>(out, i, v);
}

// TimestepEmbedder.timestep_embedding (blocks.py:41-61): out[b] = [cos(t_b f_j) | sin(t_b f_j)], f_j = exp(-ln(max_period) j / half) from the
// host's table (an angle of up to 1000 rad turns one ulp of f_j into 6e-5 of the embedding, so the table is the one torch computes)
template <typename T>
__global__ void timestep_embed_kernel(const float* __restrict__ t, const float* __restrict__ freqs, T* __restrict__ out, int B, int dim) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= B * dim) return;
  const int b = i / dim, j = i - b * dim, half = dim / 2;
  const int jj = j < half ? j : j - half;
  const float a = t[b] * freqs[jj];
  stf<T>(out, i, j < half ? cosf(a) : sinf(a));
}

// a[r][c] += v[c]: a position embedding (fp32 parameter) added to every sample
template <typename T>
__global__ void add_rowvec_kernel(T* __restrict__ a, const float* __restrict__ v, long rows, long cols) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < rows * cols) stf<T>(a, i, ldf<T>(a, i) + v[i % cols]);
}

// [M][N] -> [N][Mp], columns M .. Mp-1 zero
template <typename T>
__global__ void transpose_pad_kernel(const T* __restrict__ in, T* __restrict__ out, int M, int N, int Mp) {
  __shared__ float tile[32][33];
  const int n0 = blockIdx.x * 32, m0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int r = ty; r < 32; r += 8) { const int m = m0 + r, n = n0 + tx; tile[r][tx] = (m < M && n < N) ? ldf<T>(in, (long)m * N + n) : 0.f; }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) { const int n = n0 + r, m = m0 + tx; if (n < N && m < Mp) stf<T>(out, (long)n * Mp + m, tile[tx][r]); }
}

// 16-bit-capable forms of vt_colsum / vt_add_ / vt_copy_cols (csrc/vt_train.hip, fp32 only): same orders of summation, typed loads
template <typename T>
__global__ __launch_bounds__(1024) void colsum_t_kernel(const T* __restrict__ x, long ld, float* __restrict__ out, int M, int N) {
  __shared__ float part[32][33];
  const int c = threadIdx.x & 31, r = threadIdx.x >> 5;
  const int n = blockIdx.x * 32 + c;
  float s0 = 0.f, s1 = 0.f;
  if (n < N) {
    int m = r;
    for (; m + 32 < M; m += 64) { s0 += ldf<T>(x, (long)m * ld + n); s1 += ldf<T>(x, (long)(m + 32) * ld + n); }
    if (m < M) s0 += ldf<T>(x, (long)m * ld + n);
  }
  part[r][c] = s0 + s1;
  __syncthreads();
  for (int h = 16; h > 0; h >>= 1) {
    if (r < h) part[r][c] += part[r + h][c];
    __syncthreads();
  }
  if (r == 0 && n < N) out[n] = part[0][c];
}
template <typename T>
__global__ void add_t_kernel(T* __restrict__ a, const T* __restrict__ b, long n) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) stf<T>(a, i, ldf<T>(a, i) + ldf<T>(b, i));
}
template <typename T>
__global__ void copy_cols_t_kernel(const T* __restrict__ src, long lds_, long off, T* __restrict__ dst, long ldd, long doff, long rows, long cols) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * cols) return;
  const long c = i % cols, m = i / cols;
  dst[m * ldd + doff + c] = src[m * lds_ + off + c];
}

// ------------------------------------------------------------------------------------------------ global-norm clipping
// The table is vt_adamw_ema_multi's (vt_optim.h: MtEntry, MT_CHUNK); a block takes one chunk of one gradient (mt_chunk).  The kernels of this
// and the next three sections that take 128-bit words where their tensors are 16-byte aligned share the walk over a chunk too (mt_walk).
static_assert(16 * 256 == MT_CHUNK, "the 16 scalar passes of 256 threads of sumsq_mt_kernel and scale_mt_kernel walk one chunk");
__global__ __launch_bounds__(256) void sumsq_mt_kernel(const MtEntry* __restrict__ tab, int ntensors, float* __restrict__ part) {
  __shared__ float red[4];
  const MtChunk c = mt_chunk(tab, ntensors);
  float s = 0.f;
  for (int it = 0; it < 16; ++it) {
    const long i = c.base + it * 256 + threadIdx.x;
    if (i < c.e.n) { const float v = c.e.g[i]; s += v * v; }
  }
  s = block_sum4(s, red);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}
// one block: norm = sqrt(sum of the chunk partials, fixed order), coef = min(1, max_norm / (norm + 1e-6))  (torch clip_grad_norm_)
__global__ __launch_bounds__(256) void clip_coef_kernel(const float* __restrict__ part, long nchunks, float max_norm, float* __restrict__ out2) {
  __shared__ float red[4];
  float s = 0.f;
  for (long i = threadIdx.x; i < nchunks; i += 256) s += part[i];
  s = block_sum4(s, red);
  if (threadIdx.x == 0) {
    const float norm = sqrtf(s);
    out2[0] = norm;
    out2[1] = fminf(1.0f, max_norm / (norm + 1e-6f));
  }
}
__global__ __launch_bounds__(256) void scale_mt_kernel(const MtEntry* __restrict__ tab, int ntensors, const float* __restrict__ norm_coef) {
  const MtChunk c = mt_chunk(tab, ntensors);
  const float k = norm_coef[1];
  if (k >= 1.0f) return;                                       // torch multiplies by a coefficient clamped to 1: the same values
  for (int it = 0; it < 16; ++it) {
    const long i = c.base + it * 256 + threadIdx.x;
    if (i < c.e.n) c.e.g[i] *= k;
  }
}

// fp16 training (dynamic loss scaling): the table's gradients are S times too large.  Pass 1 looks at every RAW element (found_inf |= !isfinite(g),
// what torch's _amp_foreach_non_finite_check_and_unscale_ checks) and forms the chunk's sum of squares of u = g * inv_S; the flag is an integer OR (order
// independent), the float partials have a fixed order of their own: a thread adds its 4 words of 4, not sumsq_mt_kernel's 16 scalars.  A word's
// squares are rounded before they are added and the tail's are fused, which is what the compiler made of `s += u * u` when the norms of fp16
// training were first recorded: written out (contract(off), fmaf) so that their last bits do not hang on where it chooses to contract.
__global__ __launch_bounds__(256) void unscale_sumsq_mt_kernel(const MtEntry* __restrict__ tab, int ntensors, float inv_scale, float* __restrict__ part,
                                                               int* __restrict__ found_inf) {
  __shared__ float red[4];
  const MtChunk c = mt_chunk(tab, ntensors);
  const float* __restrict__ g = c.e.g + c.base;
  float s = 0.f;
  bool bad = false;
  mt_walk(c.cnt, (((size_t)g) & 15) == 0,
          [&](int j) {
#pragma clang fp contract(off)
            const float4 v = reinterpret_cast<const float4*>(g)[j];
            bad |= !(isfinite(v.x) && isfinite(v.y) && isfinite(v.z) && isfinite(v.w));
            const float ux = v.x * inv_scale, uy = v.y * inv_scale, uz = v.z * inv_scale, uw = v.w * inv_scale;
            s += ux * ux; s += uy * uy; s += uz * uz; s += uw * uw;
          },
          [&](int i) {
            const float v = g[i], u = v * inv_scale;
            bad |= !isfinite(v);
            s = fmaf(u, u, s);
          });
  s = block_sum4(s, red);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
  if (bad) atomicOr(found_inf, 1);
}
// pass 2: g = (g * inv_S) * coef as TWO multiplications (the bits of torch's unscale followed by its clip, for any S); nothing is written when the
// flag is set.  No coef >= 1 exit: the unscale is always due.
__global__ __launch_bounds__(256) void unscale_scale_mt_kernel(const MtEntry* __restrict__ tab, int ntensors, float inv_scale,
                                                               const float* __restrict__ norm_coef, const int* __restrict__ found_inf) {
  if (*found_inf) return;
  const MtChunk c = mt_chunk(tab, ntensors);
  float* __restrict__ g = c.e.g + c.base;
  const float k = norm_coef[1];
  mt_walk(c.cnt, (((size_t)g) & 15) == 0,
          [&](int j) {
            float4 v = reinterpret_cast<const float4*>(g)[j];
            v.x = (v.x * inv_scale) * k; v.y = (v.y * inv_scale) * k; v.z = (v.z * inv_scale) * k; v.w = (v.w * inv_scale) * k;
            reinterpret_cast<float4*>(g)[j] = v;
          },
          [&](int i) { g[i] = (g[i] * inv_scale) * k; });
}

// ------------------------------------------------------------------------------------------------ gradient accumulation
// Folds one micro-batch's fresh gradients (fresh[k], a second device array of pointers: they are new allocations every micro-batch) into the
// persistent fp32 accumulators, which are the table's g column, so that the clip and AdamW kernels read the accumulated gradient from the
// table as it stands.  accumulate = 0 stores g * scale (first micro-batch of a window: no zero pass, the accumulator is not read), otherwise
// acc = fma(g, scale, acc): one rounding per element and micro-batch in a fixed order, no atomics (vt_optim.h's grad_fold_elem).  A chunk is
// read and written as 128-bit words where both tensors are 16-byte aligned.
// The folded element i / word j of a chunk, for this kernel and for the bf16 pack below:
__device__ __forceinline__ float fold_at(const float* g, const float* acc, int i, float scale, int accumulate) {
  return accumulate ? grad_fold_elem(g[i], scale, acc[i], 1) : grad_fold_elem(g[i], scale, 0.f, 0);      // store mode does not read the accumulator
}
__device__ __forceinline__ float4 fold_quad_at(const float* g, const float* acc, int j, float scale, int accumulate) {
  const float4 gv = reinterpret_cast<const float4*>(g)[j];
  if (!accumulate)                                             // store mode does not read the accumulator (nor ask for its alignment)
    return make_float4(grad_fold_elem(gv.x, scale, 0.f, 0), grad_fold_elem(gv.y, scale, 0.f, 0), grad_fold_elem(gv.z, scale, 0.f, 0),
                       grad_fold_elem(gv.w, scale, 0.f, 0));
  const float4 a = reinterpret_cast<const float4*>(acc)[j];
  return make_float4(grad_fold_elem(gv.x, scale, a.x, 1), grad_fold_elem(gv.y, scale, a.y, 1), grad_fold_elem(gv.z, scale, a.z, 1),
                     grad_fold_elem(gv.w, scale, a.w, 1));
}
__global__ __launch_bounds__(256) void grad_accum_mt_kernel(const MtEntry* __restrict__ tab, const float* const* __restrict__ fresh, int ntensors,
                                                            float scale, int accumulate) {
  const MtChunk c = mt_chunk(tab, ntensors);
  float* __restrict__ acc = c.e.g + c.base;
  const float* __restrict__ g = fresh[c.row] + c.base;
  mt_walk(c.cnt, ((((size_t)acc) | ((size_t)g)) & 15) == 0,
          [&](int j) { reinterpret_cast<float4*>(acc)[j] = fold_quad_at(g, acc, j, scale, accumulate); },
          [&](int i) { acc[i] = fold_at(g, acc, i, scale, accumulate); });
}
// ------------------------------------------------------------------------------------------------ bf16 gradient exchange
// Data-parallel fine-tuning with comm_dtype="bf16": the window's last fold and the rounding for the exchange in one pass, and the way back.
// comm is one bf16 buffer of total_chunks * MT_CHUNK elements laid out as the table implies: tensor i starts at first_chunk_i * MT_CHUNK, so
// a block's chunk of comm starts 8 KiB-aligned whatever the tensors' own alignment.
// bf16 bits of v, round-to-nearest-even, every NaN as the one quiet NaN 0x7FC0 (what torch's .to(bfloat16) gives)
__device__ __forceinline__ uint32_t bf16_rne_bits(float v) { return v != v ? 0x7FC0u : (uint32_t)f2bf(v); }
__device__ __forceinline__ uint2 bf16_rne_quad(float4 a) {
  return make_uint2(bf16_rne_bits(a.x) | (bf16_rne_bits(a.y) << 16), bf16_rne_bits(a.z) | (bf16_rne_bits(a.w) << 16));
}
// comm[first_chunk * MT_CHUNK + e] = bf16_rne of the value grad_accum_mt_kernel would have stored (fold_at / fold_quad_at above, shared with
// it); the accumulator is read in add mode and never written.  The rest of a tensor's last chunk is written as zeros, so the
// whole buffer is defined and a sum over it is too.  Aligned tensors: one float4 (two in add mode) in, one 8-byte store out per thread and pass.
__global__ __launch_bounds__(256) void grad_fold_pack_mt_kernel(const MtEntry* __restrict__ tab, const float* const* __restrict__ fresh, int ntensors,
                                                                float scale, int accumulate, bf16_t* __restrict__ comm) {
  const MtChunk c = mt_chunk(tab, ntensors);
  const int cnt = c.cnt;
  const float* __restrict__ acc = c.e.g + c.base;
  const float* __restrict__ g = fresh[c.row] + c.base;
  bf16_t* __restrict__ out = comm + (long)blockIdx.x * MT_CHUNK;
  mt_walk(cnt, ((((size_t)g) | (accumulate ? (size_t)acc : 0)) & 15) == 0,
          [&](int j) { reinterpret_cast<uint2*>(out)[j] = bf16_rne_quad(fold_quad_at(g, acc, j, scale, accumulate)); },
          [&](int i) { out[i] = (bf16_t)bf16_rne_bits(fold_at(g, acc, i, scale, accumulate)); });
  if (cnt < MT_CHUNK) {                                          // the padding behind the tensor's last element
    const int z0 = (cnt + 3) & ~3;
    for (int i = cnt + threadIdx.x; i < z0; i += 256) out[i] = 0;
    for (int j = (z0 >> 2) + threadIdx.x; j < MT_CHUNK / 4; j += 256) reinterpret_cast<uint2*>(out)[j] = make_uint2(0u, 0u);
  }
}
// acc[e] = float(comm[first_chunk * MT_CHUNK + e]) for the n real elements of every tensor; nothing else is written.
__global__ __launch_bounds__(256) void grad_unpack_mt_kernel(const MtEntry* __restrict__ tab, int ntensors, const bf16_t* __restrict__ comm) {
  const MtChunk c = mt_chunk(tab, ntensors);
  float* __restrict__ acc = c.e.g + c.base;
  const bf16_t* __restrict__ in = comm + (long)blockIdx.x * MT_CHUNK;
  mt_walk(c.cnt, (((size_t)acc) & 15) == 0,
          [&](int j) {
            const uint2 w = reinterpret_cast<const uint2*>(in)[j];
            reinterpret_cast<float4*>(acc)[j] = make_float4(__uint_as_float(w.x << 16), __uint_as_float(w.x & 0xFFFF0000u), __uint_as_float(w.y << 16),
                                                            __uint_as_float(w.y & 0xFFFF0000u));
          },
          [&](int i) { acc[i] = bf2f(in[i]); });
}

// EMAModel.step alone over the table (the micro-batches that take no optimizer step): shadow -= (1 - decay) (shadow - p) by vt_optim.h's
// ema_elem, so it gives the bits of vt_ema_update_dev per tensor.  hyper[3] = 1 - decay.
__global__ __launch_bounds__(256) void ema_mt_kernel(const MtEntry* __restrict__ tab, int ntensors, const float* __restrict__ hyper) {
  const MtChunk c = mt_chunk(tab, ntensors);
  if (!c.e.shadow) return;
  const float omd = hyper[3];
  float* __restrict__ sh = c.e.shadow + c.base;
  const float* __restrict__ p = c.e.p + c.base;
  mt_walk(c.cnt, ((((size_t)sh) | ((size_t)p)) & 15) == 0,
          [&](int j) {
            const float4 pv = reinterpret_cast<const float4*>(p)[j];
            float4 s = reinterpret_cast<const float4*>(sh)[j];
            s.x = ema_elem(s.x, pv.x, omd); s.y = ema_elem(s.y, pv.y, omd); s.z = ema_elem(s.z, pv.z, omd); s.w = ema_elem(s.w, pv.w, omd);
            reinterpret_cast<float4*>(sh)[j] = s;
          },
          [&](int i) { sh[i] = ema_elem(sh[i], p[i], omd); });
}

// mean squared error of pred against target (fp32) and its gradient: loss = mean((pred - target)^2), dpred = grad_scale * 2 (pred - target) / n,
// the factor formed once in fp32, one rounding at the store; the loss is not scaled.  grad_scale is the loss scale of fp16 training and 1
// otherwise (1 * x is exact: the unscaled gradient's bits).  One block.
template <typename T>
__global__ __launch_bounds__(256) void mse_kernel(const T* __restrict__ pred, const float* __restrict__ tgt, T* __restrict__ dpred,
                                                  float* __restrict__ loss, long n, float grad_scale) {
  __shared__ float red[4];
  float s = 0.f;
  const float k = grad_scale * (2.0f / (float)n);
  for (long i = threadIdx.x; i < n; i += 256) {
    const float d = ldf<T>(pred, i) - tgt[i];
    s += d * d;
    stf<T>(dpred, i, k * d);
  }
  s = block_sum4(s, red);
  if (threadIdx.x == 0) loss[0] = s / (float)n;
}

}  // namespace

#define LAUNCH_OK() (vt_check_launch())
// The dtype-typed entry points: arguments first, then the activation dtype code `dt` (BAD_DT), then KERNEL<float>, <bf16_t> or <half_t> by
// vt_common.h's DISPATCH_T.
#define BAD_DT(name) vt_fail(VT_ERR_UNSUPPORTED, name ": activation dtype must be fp32 (0), bf16 (1) or fp16 (3)")

int vt_attention_bwd(const VtAttnBwdParams* p, vt_stream_t s) {
  if (!p) return vt_fail(VT_ERR_ARG, "vt_attention_bwd: null params");
  if (!p->Q || !p->K || !p->V || !p->dO || !p->dQ || !p->dK || !p->dV || !p->ws) return vt_fail(VT_ERR_ARG, "vt_attention_bwd: null pointer");
  if (p->B < 1 || p->H < 1 || p->Nq < 1 || p->Nk < 1 || p->hd != 64) return vt_fail(VT_ERR_ARG, "vt_attention_bwd: bad shape (head_dim must be 64)");
  if ((long)p->B * p->H > 65535) return vt_fail(VT_ERR_ARG, "vt_attention_bwd: B * H > 65535");
  if (p->kmask && p->km_bs < p->Nk) return vt_fail(VT_ERR_ARG, "vt_attention_bwd: key mask row shorter than Nk");
  if (!vt_is_act_dtype(p->dtype)) return vt_fail(VT_ERR_UNSUPPORTED, "vt_attention_bwd: fp32, bf16 or fp16 operands");
  const long rows = (long)p->B * p->H * p->Nq;
  const dim3 gq((unsigned)((rows + 3) / 4)), gk((unsigned)((p->Nk + 3) / 4), (unsigned)(p->B * p->H));
  DISPATCH_T(p->dtype, T, {
    hipLaunchKernelGGL(attn_bwd_dq_kernel<T>, gq, dim3(256), 0, (hipStream_t)s, *p);
    hipLaunchKernelGGL(attn_bwd_dkv_kernel<T>, gk, dim3(256), 0, (hipStream_t)s, *p);
  })
  return LAUNCH_OK();
}
int vt_rmsnorm_bwd(const void* x, const float* w, const void* dy, void* dx, float* dyxr, int rows, int D, float eps, int mode, int dt, vt_stream_t s) {
  if (!x || !w || !dy || !dx || !dyxr || rows < 1 || D < 2 || (mode != 1 && mode != 2)) return vt_fail(VT_ERR_ARG, "vt_rmsnorm_bwd: bad argument");
  if (!vt_is_act_dtype(dt)) return BAD_DT("vt_rmsnorm_bwd");
  DISPATCH_T(dt, T, hipLaunchKernelGGL(rmsnorm_bwd_kernel<T>, dim3(rows), dim3(256), 0, (hipStream_t)s, (const T*)x, w, (const T*)dy, (T*)dx, dyxr, D, eps, mode))
  return LAUNCH_OK();
}
int vt_headnorm_bwd(const void* x, long x_stride, void* dy, long dy_stride, int heads, long tokens, const float* w, float* part, float eps, int mode,
                    int dt, vt_stream_t s) {
  if (!x || !dy || !w || !part || heads < 1 || tokens < 1 || x_stride < (long)heads * 64 || dy_stride < (long)heads * 64 || (mode != 1 && mode != 2))
    return vt_fail(VT_ERR_ARG, "vt_headnorm_bwd: bad argument");
  if (!vt_is_act_dtype(dt)) return BAD_DT("vt_headnorm_bwd");
  const long pairs = tokens * heads;
  const dim3 g((unsigned)((pairs + 63) / 64));
  DISPATCH_T(dt, T, hipLaunchKernelGGL(headnorm_bwd_kernel<T>, g, dim3(256), 0, (hipStream_t)s, (const T*)x, x_stride, (T*)dy, dy_stride, heads, pairs, w, part, eps, mode))
  return LAUNCH_OK();
}
int vt_act_bwd(const void* x, const void* dy, void* out, long n, int act, int dt, vt_stream_t s) {
  if (!x || !out || n < 1 || (act != VT_ACT_GELU_TANH && act != VT_ACT_SILU)) return vt_fail(VT_ERR_ARG, "vt_act_bwd: bad argument (act 2 = tanh-GELU, 3 = SiLU)");
  if (!vt_is_act_dtype(dt)) return BAD_DT("vt_act_bwd");
  DISPATCH_T(dt, T, hipLaunchKernelGGL(act_kernel<T>, g1(n), dim3(256), 0, (hipStream_t)s, (const T*)x, (const T*)dy, (T*)out, n, act))
  return LAUNCH_OK();
}
int vt_ddpm_qsample(const float* state, const float* action, const float* noise, const float* mask, const long* timesteps, const float* alphas_cumprod,
                    int num_train_timesteps, void* out, int odt, int B, int horizon, int action_dim, vt_stream_t s) {
  if (!state || !action || !noise || !mask || !timesteps || !alphas_cumprod || !out || num_train_timesteps < 1 || B < 1 || horizon < 1 || action_dim < 1)
    return vt_fail(VT_ERR_ARG, "vt_ddpm_qsample: bad argument");
  if (!vt_is_act_dtype(odt)) return BAD_DT("vt_ddpm_qsample");
  const dim3 g = g1((long)B * (horizon + 1) * 2 * action_dim);
  DISPATCH_T(odt, T, hipLaunchKernelGGL(ddpm_qsample_kernel<T>, g, dim3(256), 0, (hipStream_t)s, state, action, noise, mask, timesteps, alphas_cumprod,
                                        num_train_timesteps, (T*)out, B, horizon, action_dim))
  return LAUNCH_OK();
}
int vt_timestep_embed(const float* t, const float* freqs, void* out, int odt, int B, int dim, vt_stream_t s) {
  if (!t || !freqs || !out || B < 1 || dim < 2 || dim % 2) return vt_fail(VT_ERR_ARG, "vt_timestep_embed: bad argument");
  if (!vt_is_act_dtype(odt)) return BAD_DT("vt_timestep_embed");
  DISPATCH_T(odt, T, hipLaunchKernelGGL(timestep_embed_kernel<T>, g1((long)B * dim), dim3(256), 0, (hipStream_t)s, t, freqs, (T*)out, B, dim))
  return LAUNCH_OK();
}
int vt_add_rowvec_(void* a, int dt, const float* v, long rows, long cols, vt_stream_t s) {
  if (!a || !v || rows < 1 || cols < 1) return vt_fail(VT_ERR_ARG, "vt_add_rowvec_: bad argument");
  if (!vt_is_act_dtype(dt)) return BAD_DT("vt_add_rowvec_");
  DISPATCH_T(dt, T, hipLaunchKernelGGL(add_rowvec_kernel<T>, g1(rows * cols), dim3(256), 0, (hipStream_t)s, (T*)a, v, rows, cols))
  return LAUNCH_OK();
}
int vt_transpose_pad(const void* in, void* out, int dt, int M, int N, int Mp, vt_stream_t s) {
  if (!in || !out || M < 1 || N < 1 || Mp < M) return vt_fail(VT_ERR_ARG, "vt_transpose_pad: bad argument");
  if (!vt_is_act_dtype(dt)) return BAD_DT("vt_transpose_pad");
  const dim3 g((N + 31) / 32, (Mp + 31) / 32);
  DISPATCH_T(dt, T, hipLaunchKernelGGL(transpose_pad_kernel<T>, g, dim3(256), 0, (hipStream_t)s, (const T*)in, (T*)out, M, N, Mp))
  return LAUNCH_OK();
}
int vt_colsum_dt(const void* x, int dt, long ld, float* out, int M, int N, vt_stream_t s) {
  if (!x || !out || M < 1 || N < 1) return vt_fail(VT_ERR_ARG, "vt_colsum_dt: bad argument");
  if (!vt_is_act_dtype(dt)) return BAD_DT("vt_colsum_dt");
  DISPATCH_T(dt, T, hipLaunchKernelGGL(colsum_t_kernel<T>, dim3((N + 31) / 32), dim3(1024), 0, (hipStream_t)s, (const T*)x, ld, out, M, N))
  return LAUNCH_OK();
}
int vt_add_dt(void* a, const void* b, long n, int dt, vt_stream_t s) {
  if (!a || !b || n < 1) return vt_fail(VT_ERR_ARG, "vt_add_dt: bad argument");
  if (!vt_is_act_dtype(dt)) return BAD_DT("vt_add_dt");
  DISPATCH_T(dt, T, hipLaunchKernelGGL(add_t_kernel<T>, g1(n), dim3(256), 0, (hipStream_t)s, (T*)a, (const T*)b, n))
  return LAUNCH_OK();
}
int vt_copy_cols_dt(const void* src, long lds_, long off, void* dst, long ldd, long doff, long rows, long cols, int dt, vt_stream_t s) {
  if (!src || !dst || rows < 1 || cols < 1) return vt_fail(VT_ERR_ARG, "vt_copy_cols_dt: bad argument");
  if (!vt_is_act_dtype(dt)) return BAD_DT("vt_copy_cols_dt");
  DISPATCH_T(dt, T, hipLaunchKernelGGL(copy_cols_t_kernel<T>, g1(rows * cols), dim3(256), 0, (hipStream_t)s, (const T*)src, lds_, off, (T*)dst, ldd, doff, rows, cols))
  return LAUNCH_OK();
}
// vt_grad_clip_multi and vt_grad_unscale_clip_multi below stay two launch groups on purpose: their first passes add a chunk's squares in
// different orders (16 scalar passes per thread against 4 float4 passes), so one in place of the other would move the last bits of the norm
// that fp32 / bf16 training, or fp16 training, reports and clips by.
int vt_grad_clip_multi(const void* table, int ntensors, long total_chunks, float max_norm, float* chunk_part, float* norm_coef, vt_stream_t s) {
  if (!table || !chunk_part || !norm_coef || ntensors < 1 || total_chunks < 1 || !(max_norm > 0.f)) return vt_fail(VT_ERR_ARG, "vt_grad_clip_multi: bad argument");
  hipLaunchKernelGGL(sumsq_mt_kernel, dim3((unsigned)total_chunks), dim3(256), 0, (hipStream_t)s, (const MtEntry*)table, ntensors, chunk_part);
  hipLaunchKernelGGL(clip_coef_kernel, dim3(1), dim3(256), 0, (hipStream_t)s, chunk_part, total_chunks, max_norm, norm_coef);
  hipLaunchKernelGGL(scale_mt_kernel, dim3((unsigned)total_chunks), dim3(256), 0, (hipStream_t)s, (const MtEntry*)table, ntensors, norm_coef);
  return LAUNCH_OK();
}
int vt_grad_unscale_clip_multi(const void* table, int ntensors, long total_chunks, float max_norm, float inv_scale, float* chunk_part, float* norm_coef,
                               int* found_inf, vt_stream_t s) {
  if (!table || !chunk_part || !norm_coef || !found_inf || ntensors < 1 || total_chunks < 1 || !(max_norm > 0.f) || !(inv_scale > 0.f) || isinf(inv_scale))
    return vt_fail(VT_ERR_ARG, "vt_grad_unscale_clip_multi: bad argument");
  if (hipMemsetAsync(found_inf, 0, sizeof(int), (hipStream_t)s) != hipSuccess) return vt_fail(VT_ERR_LAUNCH, "vt_grad_unscale_clip_multi: clearing the flag failed");
  hipLaunchKernelGGL(unscale_sumsq_mt_kernel, dim3((unsigned)total_chunks), dim3(256), 0, (hipStream_t)s, (const MtEntry*)table, ntensors, inv_scale, chunk_part, found_inf);
  hipLaunchKernelGGL(clip_coef_kernel, dim3(1), dim3(256), 0, (hipStream_t)s, chunk_part, total_chunks, max_norm, norm_coef);
  hipLaunchKernelGGL(unscale_scale_mt_kernel, dim3((unsigned)total_chunks), dim3(256), 0, (hipStream_t)s, (const MtEntry*)table, ntensors, inv_scale, norm_coef,
                     found_inf);
  return LAUNCH_OK();
}
int vt_grad_accum_multi(const void* table, const void* fresh, int ntensors, long total_chunks, float scale, int accumulate, vt_stream_t s) {
  if (!table || !fresh || ntensors < 1 || total_chunks < 1 || !(scale > 0.f)) return vt_fail(VT_ERR_ARG, "vt_grad_accum_multi: bad argument");
  hipLaunchKernelGGL(grad_accum_mt_kernel, dim3((unsigned)total_chunks), dim3(256), 0, (hipStream_t)s, (const MtEntry*)table, (const float* const*)fresh, ntensors,
                     scale, accumulate);
  return LAUNCH_OK();
}
int vt_grad_fold_pack_multi(const void* table, const void* fresh, int ntensors, long total_chunks, float scale, int accumulate, void* comm_bf16,
                            vt_stream_t s) {
  if (!table || !fresh || !comm_bf16 || ntensors < 1 || total_chunks < 1 || !(scale > 0.f)) return vt_fail(VT_ERR_ARG, "vt_grad_fold_pack_multi: bad argument");
  if (((size_t)comm_bf16) & 15) return vt_fail(VT_ERR_ARG, "vt_grad_fold_pack_multi: comm_bf16 must be 16-byte aligned");
  hipLaunchKernelGGL(grad_fold_pack_mt_kernel, dim3((unsigned)total_chunks), dim3(256), 0, (hipStream_t)s, (const MtEntry*)table, (const float* const*)fresh,
                     ntensors, scale, accumulate, (bf16_t*)comm_bf16);
  return LAUNCH_OK();
}
int vt_grad_unpack_multi(const void* table, const void* comm_bf16, int ntensors, long total_chunks, vt_stream_t s) {
  if (!table || !comm_bf16 || ntensors < 1 || total_chunks < 1) return vt_fail(VT_ERR_ARG, "vt_grad_unpack_multi: bad argument");
  if (((size_t)comm_bf16) & 15) return vt_fail(VT_ERR_ARG, "vt_grad_unpack_multi: comm_bf16 must be 16-byte aligned");
  hipLaunchKernelGGL(grad_unpack_mt_kernel, dim3((unsigned)total_chunks), dim3(256), 0, (hipStream_t)s, (const MtEntry*)table, ntensors, (const bf16_t*)comm_bf16);
  return LAUNCH_OK();
}
int vt_ema_multi(const void* table, int ntensors, long total_chunks, const float* hyper, vt_stream_t s) {
  if (!table || !hyper || ntensors < 1 || total_chunks < 1) return vt_fail(VT_ERR_ARG, "vt_ema_multi: bad argument");
  hipLaunchKernelGGL(ema_mt_kernel, dim3((unsigned)total_chunks), dim3(256), 0, (hipStream_t)s, (const MtEntry*)table, ntensors, hyper);
  return LAUNCH_OK();
}
static int mse_launch(const void* pred, const float* target, void* dpred, float* loss, long n, int dt, float grad_scale, vt_stream_t s) {
  DISPATCH_T(dt, T, hipLaunchKernelGGL(mse_kernel<T>, dim3(1), dim3(256), 0, (hipStream_t)s, (const T*)pred, target, (T*)dpred, loss, n, grad_scale))
  return LAUNCH_OK();
}
int vt_mse_loss(const void* pred, const float* target, void* dpred, float* loss, long n, int dt, vt_stream_t s) {
  if (!pred || !target || !dpred || !loss || n < 1) return vt_fail(VT_ERR_ARG, "vt_mse_loss: bad argument");
  if (!vt_is_act_dtype(dt)) return BAD_DT("vt_mse_loss");
  return mse_launch(pred, target, dpred, loss, n, dt, 1.0f, s);
}
int vt_mse_loss_scaled(const void* pred, const float* target, void* dpred, float* loss, long n, int dt, float grad_scale, vt_stream_t s) {
  if (!pred || !target || !dpred || !loss || n < 1 || !(grad_scale > 0.f) || isinf(grad_scale)) return vt_fail(VT_ERR_ARG, "vt_mse_loss_scaled: bad argument");
  if (!vt_is_act_dtype(dt)) return BAD_DT("vt_mse_loss_scaled");
  return mse_launch(pred, target, dpred, loss, n, dt, grad_scale, s);
}
