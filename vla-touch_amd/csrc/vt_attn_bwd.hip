// vt_attn_bwd.hip — attention backward on 16-bit MFMA (bf16, or IEEE fp16 for fp16 fine-tuning) for head_dim 64 and at most 128 query rows (gfx950): the image cross-attention of RDT
// fine-tuning (67 queries x 4 374 keys), where the one-wave-per-row kernels of vt_train_rdt.hip spend 65 % of the bf16 step.
//
// Arithmetic (tests/attn_bwd_mfma_ref.py is the statement): S = scale Q K^T and dP = dO V^T are exact bf16 products summed in fp32; per query row
// m = max S, l = sum exp(S - m), delta = sum P dP over the live keys; P = exp(S - m) / l and dS = P (dP - delta) are rounded ONCE to bf16 (they
// are MFMA operands); dV = P^T dO, dK = scale dS^T Q, dQ = scale dS K accumulate in fp32 (the scale is applied to the fp32 sums, after the
// rounding of dS) and are rounded once at the store.  No atomics: every sum has a fixed order, two calls give the same bits.
//
// Keys are cut into tiles of 64 and runs of RUN_TILES tiles; grid = (run, batch * head), 4 waves.
//   stats kernel    per run: S^T and dP^T tiles (key on the accumulator row, query on the lane), online (m, l, sum e dP) per query, one partial
//                   per (run, query row)
//   combine kernel  merges the partials in run order into p->ws = (m, 1 / l, delta), as vt_attention_bwd writes them
//   main kernel     per run, with Q and dO of the (batch, head) in LDS:
//                   part 1, wave w = keys 16 w .. 16 w + 15 of the tile: S and dP with the KEY ON THE LANE (A = Q / dO rows, B = K / V rows);
//                           their accumulators, packed to bf16, are the B operands of dV^T += dO^T P and dK^T += Q^T dS, whose A operands are
//                           transposed reads (ds_read_b64_tr_b16) of the row-major Q / dO images.  All queries are here: dK, dV are complete.
//                   part 2, wave w = query tiles w, w + 4: S^T and dP^T again with the QUERY ON THE LANE (as vt_attn.hip's forward), packed dS is
//                           the B operand of dQ^T += K^T dS (A = transposed read of the K tile).  One fp32 dQ partial per run goes to ws2.
//                   Recomputing S and dP in the second orientation costs 16 MFMAs per (query tile, key tile) and saves the LDS round trip of dS.
//   dq kernel       sums the dQ partials in run order, scales, rounds, stores.
// Fragment conventions are those of vt_common.h (16x16x32, 8 consecutive k per lane); the k -> row assignment inside a 32-row block of a packed
// accumulator is (j >> 2) * 16 + g * 4 + (j & 3), which the transposed reads reproduce (vt_attn.hip, attn16u_kernel).
// Padded query rows (Nq up to the 32-row block), masked keys and the padding keys of a ragged tile have P = dS = 0 by predicate, never by
// multiplication, so they add nothing and NaNs behind a mask stay there.
// Every kernel is a template on the 16-bit type T: bf16_t (v_mfma_f32_16x16x32_bf16) or half_t (v_mfma_f32_16x16x32_f16; tests/attn_bwd_mfma16_ref.py is
// that statement).  The two forms share tiling, workspaces and summation orders; P, dS and the results are rounded once to T with the hardware's
// round-to-nearest-even conversion.  fp16 does not clamp: a dS or a result beyond 65504 becomes inf, which the loss scaler's flag catches.
#include <math.h>
#include "vt_common.h"
#include "vt_host.h"
#include "../../include/vlatouch.h"

namespace {

constexpr int KT = 64;            // keys per tile
constexpr int RUN_TILES = 4;      // key tiles per workgroup
constexpr int MAXQ = 128;         // query rows held in LDS

// stage `rows` rows of 64 bf16 (128 B) from a strided global view into the swizzled LDS image of vt_common.h (lds_frag); rows >= live are zeros
template <typename T>
__device__ __forceinline__ void stage_rows(char* dst, const T* src, long rs, int rows, int live) {
  for (int ci = threadIdx.x; ci < rows * 8; ci += 256) {
    const int r = ci >> 3, c = ci & 7;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (r < live) v = *reinterpret_cast<const uint4*>(src + (long)r * rs + c * 8);
    *reinterpret_cast<uint4*>(dst + r * 128 + swz(r, c) * 16) = v;
  }
}

// per-lane byte offset of the transposed fragment read: the 16 lanes of group g address rows g * 4 + (l15 >> 2), columns dt * 16 + (l15 & 3) * 4 .. + 3
// of a 16-row slab and receive rows g * 4 .. + 3 of column dt * 16 + l15.  Add (first row of the slab) * 128; the slab starts at a multiple of 16 rows.
__device__ __forceinline__ unsigned tr_off(int l15, int g, int dt) {
  const int row = g * 4 + (l15 >> 2);
  const int sw = ((row >> 1) & 7) ^ ((l15 & 3) >> 1);
  return (unsigned)(row * 128 + (((dt * 2) ^ sw) * 16) + (l15 & 1) * 8);
}
// A fragment X^T[column dt * 16 + l15][rows r0 + (j >> 2) * 16 + g * 4 + (j & 3)] of a row-major image
template <typename T>
__device__ __forceinline__ void tr_frag(Frag<T>& f, const char* img, int r0, unsigned off) {
#pragma unroll
  for (int hh = 0; hh < 2; ++hh) tr_frag_half(f, hh, img + (r0 + hh * 16) * 128 + off);
}
template <typename T>
__device__ __forceinline__ void pack8(Frag<T>& f, const float4_t lo, const float4_t hi) {
  const uint4 w = make_uint4(pk16<T>(lo[0], lo[1]), pk16<T>(lo[2], lo[3]), pk16<T>(hi[0], hi[1]), pk16<T>(hi[2], hi[3]));
  f.v = __builtin_bit_cast(short8_t, w);
}

// the tile's K, V images and key validity bytes (0: masked or past Nk)
template <typename T>
__device__ __forceinline__ void stage_tile(char* Ks, char* Vs, unsigned char* kval, const T* K, const T* V, long k_rs, long v_rs,
                                           const unsigned char* km, int key0, int Nk) {
  const int live = min(KT, Nk - key0);
  stage_rows(Ks, K + (long)key0 * k_rs, k_rs, KT, live);
  stage_rows(Vs, V + (long)key0 * v_rs, v_rs, KT, live);
  if (threadIdx.x < KT) {
    const int key = key0 + threadIdx.x;
    kval[threadIdx.x] = key < Nk && (!km || km[key]) ? 1 : 0;
  }
}

// S^T and dP^T of one key tile for the 16 queries of (qf, gf): lane holds [key = kt * 16 + g * 4 + r][query = l15]
template <typename T>
__device__ __forceinline__ void sdp_qlane(float4_t s[4], float4_t dp[4], const char* Ks, const char* Vs, const Frag<T> qf[2],
                                          const Frag<T> gf[2], int l15, int g) {
#pragma unroll
  for (int kt = 0; kt < 4; ++kt) {
    s[kt] = (float4_t){0.f, 0.f, 0.f, 0.f};
    dp[kt] = (float4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      Frag<T> kf, vf;
      lds_frag(kf, Ks, kt * 16 + l15, ks * 4 + g);
      lds_frag(vf, Vs, kt * 16 + l15, ks * 4 + g);
      mma16(s[kt], kf, qf[ks]);
      mma16(dp[kt], vf, gf[ks]);
    }
  }
}

// ---- statistics: one partial (max, sum exp, sum exp dP) per (batch * head, run, query row)
template <typename T>
__global__ __launch_bounds__(256) void attn_bwd_mfma_stats_kernel(VtAttnBwdParams p, float* part, int nruns) {
  __shared__ __attribute__((aligned(16))) char Ks[KT * 128];
  __shared__ __attribute__((aligned(16))) char Vs[KT * 128];
  __shared__ __attribute__((aligned(4))) unsigned char kval[KT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, g = lane >> 4;
  const int run = blockIdx.x, bh = blockIdx.y, h = bh % p.H, b = bh / p.H;
  const T* Q = (const T*)p.Q + (long)b * p.q_bs + (long)h * p.q_hs;
  const T* G = (const T*)p.dO + (long)b * p.do_bs + (long)h * p.do_hs;
  const T* K = (const T*)p.K + (long)b * p.k_bs + (long)h * p.k_hs;
  const T* V = (const T*)p.V + (long)b * p.v_bs + (long)h * p.v_hs;
  const unsigned char* km = p.kmask ? p.kmask + (long)b * p.km_bs : nullptr;
  const int nqt = (p.Nq + 15) >> 4;
  const int ntiles = (p.Nk + KT - 1) / KT;
  const int t0 = run * RUN_TILES, t1 = min(t0 + RUN_TILES, ntiles);

  Frag<T> qf[2][2], gf[2][2];
  float m[2], l[2], acc[2];
#pragma unroll
  for (int qi = 0; qi < 2; ++qi) {
    const int q = (wave + qi * 4) * 16 + l15;
    const bool ok = q < p.Nq;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      qf[qi][ks].v = ok ? *reinterpret_cast<const short8_t*>(Q + (long)q * p.q_rs + ks * 32 + g * 8) : (short8_t){0, 0, 0, 0, 0, 0, 0, 0};
      gf[qi][ks].v = ok ? *reinterpret_cast<const short8_t*>(G + (long)q * p.do_rs + ks * 32 + g * 8) : (short8_t){0, 0, 0, 0, 0, 0, 0, 0};
    }
    m[qi] = -INFINITY; l[qi] = 0.f; acc[qi] = 0.f;
  }
  for (int tile = t0; tile < t1; ++tile) {
    __syncthreads();
    stage_tile(Ks, Vs, kval, K, V, p.k_rs, p.v_rs, km, tile * KT, p.Nk);
    __syncthreads();
#pragma unroll
    for (int qi = 0; qi < 2; ++qi) {
      if (wave + qi * 4 >= nqt) continue;                       // wave-uniform
      float4_t s[4], dp[4];
      sdp_qlane(s, dp, Ks, Vs, qf[qi], gf[qi], l15, g);
      bool ok[16];
      float mx = -INFINITY;
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) {
        const unsigned kv = *reinterpret_cast<const unsigned*>(kval + kt * 16 + g * 4);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          ok[kt * 4 + r] = (kv >> (8 * r)) & 0xff;
          s[kt][r] *= p.scale;
          if (ok[kt * 4 + r]) mx = fmaxf(mx, s[kt][r]);
        }
      }
      const float mn = fmaxf(m[qi], mx);
      if (mn > -INFINITY) {                                     // this lane has seen a live key
        const float c = expf(m[qi] - mn);                       // first live key: exp(-inf) = 0
        float ls = 0.f, as = 0.f;
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (ok[kt * 4 + r]) { const float e = expf(s[kt][r] - mn); ls += e; as += e * dp[kt][r]; }
        l[qi] = l[qi] * c + ls;
        acc[qi] = acc[qi] * c + as;
        m[qi] = mn;
      }
    }
  }
  // the four lanes of a query (g = 0..3) hold disjoint keys: merge, a lane that saw no live key contributes nothing
#pragma unroll
  for (int qi = 0; qi < 2; ++qi) {
    const int q = (wave + qi * 4) * 16 + l15;
    const float M = rows4_max(m[qi]);
    const float f = m[qi] > -INFINITY ? expf(m[qi] - M) : 0.f;
    const float L = rows4_sum(l[qi] * f), A = rows4_sum(acc[qi] * f);
    if (g == 0 && q < p.Nq) {
      float* w = part + (((long)bh * nruns + run) * p.Nq + q) * 3;
      w[0] = M; w[1] = L; w[2] = A;
    }
  }
}

// merge the partials of a row in run order -> ws = (m, 1 / l, delta); no live key at all: (0, 0, 0)
__global__ __launch_bounds__(256) void attn_bwd_mfma_combine_kernel(const float* __restrict__ part, float* __restrict__ ws, long rows, int Nq, int nruns) {
  const long row = (long)blockIdx.x * 256 + threadIdx.x;        // bh * Nq + i
  if (row >= rows) return;
  const long bh = row / Nq;
  const int i = (int)(row - bh * Nq);
  float m = -INFINITY, l = 0.f, a = 0.f;
  for (int r = 0; r < nruns; ++r) {
    const float* w = part + ((bh * nruns + r) * Nq + i) * 3;
    const float mr = w[0];
    if (!(mr > -INFINITY)) continue;                            // a run whose keys are all masked: exp(-inf - (-inf)) would be NaN
    const float mn = fmaxf(m, mr);
    const float c = expf(m - mn), cr = expf(mr - mn);
    l = l * c + w[1] * cr;
    a = a * c + w[2] * cr;
    m = mn;
  }
  const float inv = l > 0.f ? 1.0f / l : 0.f;
  if (!(l > 0.f)) m = 0.f;
  ws[row * 3] = m; ws[row * 3 + 1] = inv; ws[row * 3 + 2] = a * inv;
}

// ---- dK, dV of the run's keys and the run's dQ partial
template <typename T>
__global__ __launch_bounds__(256) void attn_bwd_mfma_main_kernel(VtAttnBwdParams p, float* dqpart, int nruns) {
  __shared__ __attribute__((aligned(16))) char Qs[MAXQ * 128];
  __shared__ __attribute__((aligned(16))) char Gs[MAXQ * 128];
  __shared__ __attribute__((aligned(16))) char Ks[KT * 128];
  __shared__ __attribute__((aligned(16))) char Vs[KT * 128];
  __shared__ float st[MAXQ * 3];                                // (m, 1 / l, delta); padded rows (0, 0, 0)
  __shared__ __attribute__((aligned(4))) unsigned char kval[KT];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, g = lane >> 4;
  const int run = blockIdx.x, bh = blockIdx.y, h = bh % p.H, b = bh / p.H;
  const T* K = (const T*)p.K + (long)b * p.k_bs + (long)h * p.k_hs;
  const T* V = (const T*)p.V + (long)b * p.v_bs + (long)h * p.v_hs;
  const unsigned char* km = p.kmask ? p.kmask + (long)b * p.km_bs : nullptr;
  const int nqt = (p.Nq + 15) >> 4, nqb = (nqt + 1) >> 1;
  const int ntiles = (p.Nk + KT - 1) / KT;
  const int t0 = run * RUN_TILES, t1 = min(t0 + RUN_TILES, ntiles);

  stage_rows(Qs, (const T*)p.Q + (long)b * p.q_bs + (long)h * p.q_hs, p.q_rs, nqb * 32, p.Nq);
  stage_rows(Gs, (const T*)p.dO + (long)b * p.do_bs + (long)h * p.do_hs, p.do_rs, nqb * 32, p.Nq);
  for (int i = tid; i < nqb * 32 * 3; i += 256) st[i] = i < p.Nq * 3 ? p.ws[(long)bh * p.Nq * 3 + i] : 0.f;

  unsigned troff[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) troff[dt] = tr_off(l15, g, dt);
  float4_t dq[2][4];
#pragma unroll
  for (int qi = 0; qi < 2; ++qi)
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) dq[qi][dt] = (float4_t){0.f, 0.f, 0.f, 0.f};

  for (int tile = t0; tile < t1; ++tile) {
    const int key0 = tile * KT;
    __syncthreads();
    stage_tile(Ks, Vs, kval, K, V, p.k_rs, p.v_rs, km, key0, p.Nk);
    __syncthreads();

    // ---- part 1: this wave's 16 keys against every query block -> dK^T, dV^T [d = dt * 16 + g * 4 + r][key = wave * 16 + l15]
    {
      Frag<T> kf[2], vf[2];
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        lds_frag(kf[ks], Ks, wave * 16 + l15, ks * 4 + g);
        lds_frag(vf[ks], Vs, wave * 16 + l15, ks * 4 + g);
      }
      const bool kok = kval[wave * 16 + l15] != 0;
      float4_t dk[4], dv[4];
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) { dk[dt] = (float4_t){0.f, 0.f, 0.f, 0.f}; dv[dt] = (float4_t){0.f, 0.f, 0.f, 0.f}; }
      for (int qb = 0; qb < nqb; ++qb) {
        float4_t pr[2], ds[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {                           // the two 16-query tiles of the block: [query = g * 4 + r][key = l15]
          const int q0 = qb * 32 + t * 16;
          float4_t s = (float4_t){0.f, 0.f, 0.f, 0.f}, dp = (float4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int ks = 0; ks < 2; ++ks) {
            Frag<T> qf, gf;
            lds_frag(qf, Qs, q0 + l15, ks * 4 + g);
            lds_frag(gf, Gs, q0 + l15, ks * 4 + g);
            mma16(s, qf, kf[ks]);
            mma16(dp, gf, vf[ks]);
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float* w = st + (q0 + g * 4 + r) * 3;
            const float inv = w[1];
            const bool live = kok && inv > 0.f;
            const float pv = live ? expf(s[r] * p.scale - w[0]) * inv : 0.f;
            pr[t][r] = pv;
            ds[t][r] = live ? pv * (dp[r] - w[2]) : 0.f;
          }
        }
        Frag<T> pf, sf;
        pack8(pf, pr[0], pr[1]);
        pack8(sf, ds[0], ds[1]);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          Frag<T> gt, qt;
          tr_frag(gt, Gs, qb * 32, troff[dt]);
          tr_frag(qt, Qs, qb * 32, troff[dt]);
          mma16(dv[dt], gt, pf);
          mma16(dk[dt], qt, sf);
        }
      }
      const int key = key0 + wave * 16 + l15;
      if (key < p.Nk) {                                         // masked keys store their zeros, padding keys nothing
        T* dK = (T*)p.dK + (long)b * p.dk_bs + (long)key * p.dk_rs + (long)h * p.dk_hs;
        T* dV = (T*)p.dV + (long)b * p.dv_bs + (long)key * p.dv_rs + (long)h * p.dv_hs;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          *reinterpret_cast<uint2*>(dK + dt * 16 + g * 4) = make_uint2(pk16<T>(dk[dt][0] * p.scale, dk[dt][1] * p.scale), pk16<T>(dk[dt][2] * p.scale, dk[dt][3] * p.scale));
          *reinterpret_cast<uint2*>(dV + dt * 16 + g * 4) = make_uint2(pk16<T>(dv[dt][0], dv[dt][1]), pk16<T>(dv[dt][2], dv[dt][3]));
        }
      }
    }

    // ---- part 2: this wave's query tiles against the tile's 64 keys -> dQ^T [d = dt * 16 + g * 4 + r][query = l15]
#pragma unroll
    for (int qi = 0; qi < 2; ++qi) {
      const int qt = wave + qi * 4;
      if (qt >= nqt) continue;                                  // wave-uniform
      Frag<T> qf[2], gf[2];
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        lds_frag(qf[ks], Qs, qt * 16 + l15, ks * 4 + g);
        lds_frag(gf[ks], Gs, qt * 16 + l15, ks * 4 + g);
      }
      float4_t s[4], dp[4];
      sdp_qlane(s, dp, Ks, Vs, qf, gf, l15, g);
      const float* w = st + (qt * 16 + l15) * 3;
      const float mrow = w[0], inv = w[1], delta = w[2];
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) {
        const unsigned kv = *reinterpret_cast<const unsigned*>(kval + kt * 16 + g * 4);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const bool live = ((kv >> (8 * r)) & 0xff) && inv > 0.f;
          const float pv = live ? expf(s[kt][r] * p.scale - mrow) * inv : 0.f;
          s[kt][r] = live ? pv * (dp[kt][r] - delta) : 0.f;     // dS
        }
      }
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) {
        Frag<T> sf;
        pack8(sf, s[kb * 2], s[kb * 2 + 1]);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          Frag<T> ktf;
          tr_frag(ktf, Ks, kb * 32, troff[dt]);
          mma16(dq[qi][dt], ktf, sf);
        }
      }
    }
  }
#pragma unroll
  for (int qi = 0; qi < 2; ++qi) {
    const int q = (wave + qi * 4) * 16 + l15;
    if (q < p.Nq) {
      float* o = dqpart + (((long)bh * nruns + run) * p.Nq + q) * 64;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) *reinterpret_cast<float4_t*>(o + dt * 16 + g * 4) = dq[qi][dt];
    }
  }
}

// dQ = scale * (sum of the run partials, in run order); one wave per (batch * head, query row), lane = head-dim element
template <typename T>
__global__ __launch_bounds__(256) void attn_bwd_mfma_dq_kernel(VtAttnBwdParams p, const float* __restrict__ dqpart, int nruns) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= (long)p.B * p.H * p.Nq) return;
  const long bh = row / p.Nq;
  const int i = (int)(row - bh * p.Nq), h = (int)(bh % p.H), b = (int)(bh / p.H);
  float s = 0.f;
  for (int r = 0; r < nruns; ++r) s += dqpart[((bh * nruns + r) * p.Nq + i) * 64 + lane];
  stf<T>((T*)p.dQ, (long)b * p.dq_bs + (long)i * p.dq_rs + (long)h * p.dq_hs + lane, s * p.scale);
}

inline int nruns_of(int Nk) { return ((Nk + KT - 1) / KT + RUN_TILES - 1) / RUN_TILES; }

}  // namespace

long vt_attention_bwd_mfma_ws_bytes(int B, int H, int Nq, int Nk) {
  if (B < 1 || H < 1 || Nq < 1 || Nq > MAXQ || Nk < 1 || (long)B * H > 65535) return -1;
  return (long)B * H * nruns_of(Nk) * Nq * (3 + 64) * (long)sizeof(float);
}

int vt_attention_bwd_mfma(const VtAttnBwdParams* p, void* ws2, long ws2_bytes, vt_stream_t s) {
  if (!p) return vt_fail(VT_ERR_ARG, "vt_attention_bwd_mfma: null params");
  if (!p->Q || !p->K || !p->V || !p->dO || !p->dQ || !p->dK || !p->dV || !p->ws || !ws2) return vt_fail(VT_ERR_ARG, "vt_attention_bwd_mfma: null pointer");
  if (p->B < 1 || p->H < 1 || p->Nq < 1 || p->Nk < 1 || p->hd != 64) return vt_fail(VT_ERR_ARG, "vt_attention_bwd_mfma: bad shape (head_dim must be 64)");
  if (p->dtype != VT_BF16 && p->dtype != VT_F16) return vt_fail(VT_ERR_UNSUPPORTED, "vt_attention_bwd_mfma: bf16 or fp16 operands only (vt_attention_bwd takes fp32)");
  if (p->Nq > MAXQ) return vt_fail(VT_ERR_UNSUPPORTED, "vt_attention_bwd_mfma: Nq = %d > %d query rows", p->Nq, MAXQ);
  if ((long)p->B * p->H > 65535) return vt_fail(VT_ERR_ARG, "vt_attention_bwd_mfma: B * H > 65535");
  if (p->kmask && p->km_bs < p->Nk) return vt_fail(VT_ERR_ARG, "vt_attention_bwd_mfma: key mask row shorter than Nk");
  const long strides[] = {p->q_bs, p->q_rs, p->q_hs, p->k_bs, p->k_rs, p->k_hs, p->v_bs, p->v_rs, p->v_hs, p->do_bs, p->do_rs, p->do_hs,
                          p->dq_bs, p->dq_rs, p->dq_hs, p->dk_bs, p->dk_rs, p->dk_hs, p->dv_bs, p->dv_rs, p->dv_hs};
  for (long v : strides)
    if (v % 8) return vt_fail(VT_ERR_ARG, "vt_attention_bwd_mfma: stride %ld is not a multiple of 8 elements", v);
  const void* bases[] = {p->Q, p->K, p->V, p->dO, p->dQ, p->dK, p->dV, ws2};
  for (const void* a : bases)
    if ((uintptr_t)a & 15) return vt_fail(VT_ERR_ARG, "vt_attention_bwd_mfma: base pointer not 16-byte aligned");
  const long need = vt_attention_bwd_mfma_ws_bytes(p->B, p->H, p->Nq, p->Nk);
  if (need < 0 || ws2_bytes < need) return vt_fail(VT_ERR_ARG, "vt_attention_bwd_mfma: ws2 has %ld bytes, %ld needed", ws2_bytes, need);
  const int nruns = nruns_of(p->Nk);
  const long rows = (long)p->B * p->H * p->Nq;
  float* dqpart = (float*)ws2;                                  // [B * H][nruns][Nq][64], first: its rows are stored 16 bytes at a time
  float* part = dqpart + rows * nruns * 64;                     // [B * H][nruns][Nq][3]
  const dim3 grid((unsigned)nruns, (unsigned)(p->B * p->H));
  const dim3 gc((unsigned)((rows + 255) / 256)), gq((unsigned)((rows + 3) / 4));
  DISPATCH_T16(p->dtype, T, {                                   // bf16 or fp16: checked above
    hipLaunchKernelGGL(attn_bwd_mfma_stats_kernel<T>, grid, dim3(256), 0, (hipStream_t)s, *p, part, nruns);
    hipLaunchKernelGGL(attn_bwd_mfma_combine_kernel, gc, dim3(256), 0, (hipStream_t)s, part, p->ws, rows, p->Nq, nruns);
    hipLaunchKernelGGL(attn_bwd_mfma_main_kernel<T>, grid, dim3(256), 0, (hipStream_t)s, *p, dqpart, nruns);
    hipLaunchKernelGGL(attn_bwd_mfma_dq_kernel<T>, gq, dim3(256), 0, (hipStream_t)s, *p, dqpart, nruns);
  })
  return vt_check_launch();
}
