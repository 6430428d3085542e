// vt_t5.hip — T5 v1.1 text encoder (HF T5EncoderModel, feed_forward_proj = "gated-gelu"): the instruction -> lang_tokens stage of RDT.
//
//   x = shared[ids]                                  (no embedding scale, no absolute positions; fp32 residual stream)
//   per layer:  x += o(Attn(rms1(x)))                Attn = softmax(q k^T + pos_bias[h, i, j] + mask) v,  d_kv = 64, NO 1/sqrt(d) scale
//               x += wo(gelu_tanh(wi_0 h) * wi_1 h)  h = rms2(x)
//   out = final_layer_norm(x)                        T5LayerNorm: mean-square RMSNorm, no bias
// pos_bias[h, i, j] = rel_bias[bucket(j - i)][h]: rel_bias [num_buckets][heads] comes from layer 0 and is shared by every layer; the bucket of
// every relative position -1023 .. 1023 is an int8 table computed on the host with HF's own fp32 formula (vt_t5_forward, include/vlatouch.h).
//
// Weight order (vt_t5_create):
//   0 shared [vocab][D] cdt   1 rel_bias [num_buckets][heads] fp32
//   per layer (6 entries): ln1 [D] fp32  qkv_w [3 I][D] cdt (q | k | v rows)  o_w [D][I] cdt  ln2 [D] fp32  wi_w [2 F][D] cdt (wi_0 | wi_1 rows)  wo_w [D][F] cdt
//   then  final_ln [D] fp32                                                   (I = heads * 64, F = d_ff)
#include <math.h>
#include <string.h>
#include <new>
#include <vector>
#include "vt_common.h"
#include "vt_kernels.h"
#include "vt_host.h"
#include "../../include/vlatouch.h"

namespace {

constexpr int T5_MAX_L = 1024;
constexpr int T5_REL_TAB = 2 * T5_MAX_L - 1;   // bucket table entries: rel = -1023 .. 1023 at index rel + 1023

inline dim3 g1(long n) { return dim3((unsigned)((n + 255) / 256)); }

// ------------------------------------------------------------------ token gather: x[r][:] = (float) emb[ids[r]][:]
// ids were range-checked on the host; the clamp only keeps a stray id from reading outside the table
template <typename T>
__global__ void t5_gather_kernel(const int* __restrict__ ids, const T* __restrict__ emb, float* __restrict__ x, long rows, int D, int vocab) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int per_row = D / 4;
  if (i >= rows * per_row) return;
  const long r = i / per_row;
  const int c = (int)(i - r * per_row) * 4;
  int id = ids[r];
  id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
  const T* e = emb + (long)id * D + c;
  *reinterpret_cast<float4*>(x + r * D + c) = make_float4(Elem<T>::to_f(e[0]), Elem<T>::to_f(e[1]), Elem<T>::to_f(e[2]), Elem<T>::to_f(e[3]));
}

// ------------------------------------------------------------------ GeGLU gate (VT_ACT_GEGLU): h[r][c] = gelu_tanh(g[r][c]) * g[r][F + c], c < F (out of place)
template <typename T>
__global__ void t5_geglu_kernel(const T* __restrict__ g, long ldg, T* __restrict__ h, long ldh, long rows, int F) {
  constexpr int V = 16 / sizeof(T);
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int per_row = F / V;
  if (i >= rows * per_row) return;
  const long r = i / per_row;
  const int c = (int)(i - r * per_row) * V;
  const T* p = g + r * ldg + c;
  const uint4 a = *reinterpret_cast<const uint4*>(p), b = *reinterpret_cast<const uint4*>(p + F);
  const T* av = reinterpret_cast<const T*>(&a);
  const T* bv = reinterpret_cast<const T*>(&b);
  uint4 o;
  T* ov = reinterpret_cast<T*>(&o);
#pragma unroll
  for (int k = 0; k < V; ++k) ov[k] = Elem<T>::from_f(act_apply(Elem<T>::to_f(av[k]), VT_ACT_GELU_TANH) * Elem<T>::to_f(bv[k]));   // HF gelu_new (tanh form)
  *reinterpret_cast<uint4*>(h + r * ldh + c) = o;
}

// ------------------------------------------------------------------ relative-position-bias attention, head width 64
// qkv [B*L][3 I] (q | k | v, head h at column h*64 of its part), out [B*L][I].  Block = 4 waves = 64 query rows of one (batch, head); the keys are
// walked in tiles of 64 with an fp32 online softmax.  S = q k^T: A = q rows straight from global (8 consecutive d per lane, library fragment
// convention of vt_common.h), B = k rows straight from global (the four waves of a block read the same tile: L1 / L2 hits).  P V: P goes through LDS
// (accumulator layout -> A fragment), V is staged transposed in LDS (Vt[d][key]) so a B fragment is 8 consecutive keys.  The bias of every relative
// position of this head is expanded into LDS once per block: relb[rel + L - 1] = rel_bias[bucket[rel + 1023]][h].
struct T5AttnParams {
  const void* qkv; void* out;
  const int8_t* bucket;       // [T5_REL_TAB], device
  const float* rel_bias;      // [num_buckets][H]
  const uint8_t* kmask;       // [B][L] (1 = attend) or null
  int B, H, L, inner, num_buckets;
};

template <typename T> constexpr int t5_pitch() { return 64 + 16 / (int)sizeof(T); }   // LDS row pitch in elements (one 16-B chunk of padding)

// 8 consecutive elements (16-B aligned for bf16, 32-B for fp32) -> a fragment
__device__ __forceinline__ void ld_frag8(Frag<bf16_t>& f, const bf16_t* src) { f.v = *reinterpret_cast<const short8_t*>(src); }
__device__ __forceinline__ void ld_frag8(Frag<float>& f, const float* src) {
  const float4 lo = *reinterpret_cast<const float4*>(src), hi = *reinterpret_cast<const float4*>(src + 4);
  f.v[0] = lo.x; f.v[1] = lo.y; f.v[2] = lo.z; f.v[3] = lo.w;
  f.v[4] = hi.x; f.v[5] = hi.y; f.v[6] = hi.z; f.v[7] = hi.w;
}

template <typename T>
__global__ __launch_bounds__(256) void t5_attn_kernel(const T5AttnParams p) {
  constexpr int PT = t5_pitch<T>();
  __shared__ float relb[T5_REL_TAB];
  __shared__ __attribute__((aligned(16))) T vt[64 * PT];          // Vt[d][key]
  __shared__ __attribute__((aligned(16))) T pl[4][16 * PT];       // per wave P[q][key]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, g = lane >> 4, c16 = lane & 15;
  const int q0 = blockIdx.x * 64, h = blockIdx.y, b = blockIdx.z;
  const int L = p.L, ld = 3 * p.inner;
  const T* base = reinterpret_cast<const T*>(p.qkv) + (long)b * L * ld;
  const T* Q = base + h * 64;
  const T* K = base + p.inner + h * 64;
  const T* V = base + 2 * p.inner + h * 64;
  const uint8_t* km = p.kmask ? p.kmask + (long)b * L : nullptr;

  for (int i = tid; i < 2 * L - 1; i += 256) {
    int bk = p.bucket[i - (L - 1) + (T5_MAX_L - 1)];
    bk = bk < 0 ? 0 : (bk >= p.num_buckets ? p.num_buckets - 1 : bk);
    relb[i] = p.rel_bias[bk * p.H + h];
  }

  // q fragments of this wave's 16 rows (rows past L read row L-1; their output is not stored)
  const int qa = min(q0 + w * 16 + c16, L - 1);
  Frag<T> qf[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) ld_frag8(qf[ks], Q + (long)qa * ld + ks * 32 + g * 8);
  float4_t o[4];
#pragma unroll
  for (int n = 0; n < 4; ++n) o[n] = (float4_t){0.f, 0.f, 0.f, 0.f};
  float m[4], lsum[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) { m[r] = -INFINITY; lsum[r] = 0.f; }
  const int qrow0 = q0 + w * 16 + g * 4;     // query index of accumulator row r is qrow0 + r

  for (int k0 = 0; k0 < L; k0 += 64) {
    __syncthreads();                          // previous tile's Vt / P reads are done (and relb is complete on the first pass)
    {   // V tile -> Vt[d][key]; keys past L are zeros
      const int kk = tid & 63, d0 = (tid >> 6) * 16;
      const int key = k0 + kk;
      uint4 buf[16 * sizeof(T) / 16];
      const uint4* src = reinterpret_cast<const uint4*>(V + (long)min(key, L - 1) * ld + d0);
#pragma unroll
      for (int j = 0; j < (int)(16 * sizeof(T) / 16); ++j) buf[j] = key < L ? src[j] : make_uint4(0u, 0u, 0u, 0u);
      const T* e = reinterpret_cast<const T*>(buf);
#pragma unroll
      for (int j = 0; j < 16; ++j) vt[(d0 + j) * PT + kk] = e[j];
    }
    // S = q k^T over 4 key sub-tiles of 16
    float4_t s[4];
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      s[n] = (float4_t){0.f, 0.f, 0.f, 0.f};
      const int key = min(k0 + n * 16 + c16, L - 1);
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        Frag<T> kf;
        ld_frag8(kf, K + (long)key * ld + ks * 32 + g * 8);
        mma16(s[n], qf[ks], kf);
      }
    }
    // bias + mask, running max
    float tmax[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) tmax[r] = -INFINITY;
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const int key = k0 + n * 16 + c16, kc = min(key, L - 1);
      const bool valid = key < L && (!km || km[kc]);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int qi = min(qrow0 + r, L - 1);
        const float v = valid ? s[n][r] + relb[kc - qi + L - 1] : -INFINITY;
        s[n][r] = v;
        tmax[r] = fmaxf(tmax[r], v);
      }
    }
    float alpha[4], mu[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float mn = fmaxf(m[r], row16_max(tmax[r]));
      mu[r] = mn == -INFINITY ? 0.f : mn;     // a row with no valid key yet: exp(-inf - 0) = 0, never inf - inf
      alpha[r] = __expf(m[r] - mu[r]);
      m[r] = mn;
      lsum[r] *= alpha[r];
    }
#pragma unroll
    for (int n = 0; n < 4; ++n) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float e = __expf(s[n][r] - mu[r]);
        lsum[r] += e;
        pl[w][(g * 4 + r) * PT + n * 16 + c16] = Elem<T>::from_f(e);
        o[n][r] *= alpha[r];
      }
    }
    __syncthreads();                          // Vt and P complete
    // O += P Vt^T: A = P[q = c16][key = ks*32 + g*8 + j], B = Vt[d = n*16 + c16][key]
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      Frag<T> pf;
      ld_frag8(pf, &pl[w][c16 * PT + ks * 32 + g * 8]);
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        Frag<T> vf;
        ld_frag8(vf, &vt[(n * 16 + c16) * PT + ks * 32 + g * 8]);
        mma16(o[n], pf, vf);
      }
    }
  }
  T* O = reinterpret_cast<T*>(p.out) + (long)b * L * p.inner + h * 64;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int qi = qrow0 + r;
    const float l = row16_sum(lsum[r]);
    const float inv = l > 0.f ? 1.0f / l : 0.f;     // no valid key at all (rejected on the host): zeros, not NaN
    if (qi < L) {
#pragma unroll
      for (int n = 0; n < 4; ++n) O[(long)qi * p.inner + n * 16 + c16] = Elem<T>::from_f(o[n][r] * inv);
    }
  }
}

}  // namespace

// ======================================================================================= the two kernels as entries of their own (include/vlatouch.h)
// vt_t5_forward launches attention and the gate through these and nowhere else, so a test of either entry runs the engine's code.
int vt_t5_attention(const void* qkv, void* out, const int8_t* bucket_tab, const float* rel_bias, const uint8_t* kmask, int B, int H, int L,
                    int num_buckets, int dt, vt_stream_t stream) {
  if (!qkv || !out || !bucket_tab || !rel_bias) return vt_fail(VT_ERR_ARG, "vt_t5_attention: null qkv, out, bucket_tab or rel_bias");
  if (B < 1 || H < 1 || L < 1) return vt_fail(VT_ERR_ARG, "vt_t5_attention: bad sizes B=%d H=%d L=%d", B, H, L);
  if (B > 65535 || H > 65535) return vt_fail(VT_ERR_ARG, "vt_t5_attention: B=%d or H=%d exceeds the grid's 65535", B, H);
  if (L > T5_MAX_L) return vt_fail(VT_ERR_ARG, "vt_t5_attention: L = %d exceeds %d", L, T5_MAX_L);
  if (num_buckets < 1 || num_buckets > 127) return vt_fail(VT_ERR_ARG, "vt_t5_attention: num_buckets = %d is outside 1 .. 127", num_buckets);
  if (dt != VT_F32 && dt != VT_BF16) return vt_fail(VT_ERR_UNSUPPORTED, "vt_t5_attention: dt must be fp32 (0) or bf16 (1), got %d", dt);
  T5AttnParams p;
  p.qkv = qkv; p.out = out; p.bucket = bucket_tab; p.rel_bias = rel_bias; p.kmask = kmask;
  p.B = B; p.H = H; p.L = L; p.inner = H * 64; p.num_buckets = num_buckets;
  const dim3 grid((L + 63) / 64, H, B);
  // chosen by hand between the two types a T5 handle admits: DISPATCH_T (vt_common.h) would also instantiate the kernel for half_t
  if (dt == VT_BF16) hipLaunchKernelGGL((t5_attn_kernel<bf16_t>), grid, dim3(256), 0, (hipStream_t)stream, p);
  else hipLaunchKernelGGL((t5_attn_kernel<float>), grid, dim3(256), 0, (hipStream_t)stream, p);
  return vt_check_launch();
}

int vt_t5_geglu(const void* g, long ldg, void* h, long ldh, long rows, int F, int dt, vt_stream_t stream) {
  if (!g || !h) return vt_fail(VT_ERR_ARG, "vt_t5_geglu: null g or h");
  if (dt != VT_F32 && dt != VT_BF16) return vt_fail(VT_ERR_UNSUPPORTED, "vt_t5_geglu: dt must be fp32 (0) or bf16 (1), got %d", dt);
  const int V = 16 / vt_dt_bytes(dt);                       // elements of a lane's 16-byte vector
  if (rows < 1 || F < 1) return vt_fail(VT_ERR_ARG, "vt_t5_geglu: bad sizes rows=%ld F=%d", rows, F);
  if (F % V || ldg % V || ldh % V) return vt_fail(VT_ERR_ARG, "vt_t5_geglu: F=%d, ldg=%ld and ldh=%ld must be multiples of %d elements (16 bytes)", F, ldg, ldh, V);
  if (ldg < 2L * F || ldh < F) return vt_fail(VT_ERR_ARG, "vt_t5_geglu: ldg=%ld < 2 F or ldh=%ld < F (F=%d)", ldg, ldh, F);
  const long n = rows * (F / V);
  if (n > 0x7fffffffL * 256) return vt_fail(VT_ERR_ARG, "vt_t5_geglu: rows=%ld x F=%d is more than one launch covers", rows, F);
  if (dt == VT_BF16) hipLaunchKernelGGL((t5_geglu_kernel<bf16_t>), g1(n), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)g, ldg, (bf16_t*)h, ldh, rows, F);
  else hipLaunchKernelGGL((t5_geglu_kernel<float>), g1(n), dim3(256), 0, (hipStream_t)stream, (const float*)g, ldg, (float*)h, ldh, rows, F);
  return vt_check_launch();
}

// ======================================================================================= driver
struct T5Layer { const float *ln1, *ln2; const void *qkv_w, *o_w, *wi_w, *wo_w; };
struct vt_t5_s {
  vt_t5_desc d;
  const void* shared; const float* rel_bias; const float* final_ln;
  std::vector<T5Layer> L;
};

int vt_t5_num_weights(const vt_t5_desc* d) { return d ? 2 + 6 * d->layers + 1 : -1; }

int vt_t5_create(const vt_t5_desc* desc, const void* const* w, int n, vt_t5_t* out) {
  CK(vt_create_args("vt_t5_create", desc, w, out));
  const vt_t5_desc& d = *desc;
  if (d.d_kv != 64) return vt_fail(VT_ERR_UNSUPPORTED, "vt_t5_create: d_kv must be 64 (got %d)", d.d_kv);
  if (!((d.cdt == VT_F32 && d.adt == VT_F32) || (d.cdt == VT_BF16 && d.adt == VT_BF16)))
    return vt_fail(VT_ERR_UNSUPPORTED, "vt_t5_create: precisions are fp32 (cdt = adt = 0) and bf16 (cdt = adt = 1)");
  if (d.layers < 1 || d.heads < 1 || d.vocab < 1 || d.d_model < 64 || d.d_model % 64 || d.d_model > 4096 || d.d_ff < 64 || d.d_ff % 64 ||
      d.num_buckets < 1 || d.num_buckets > 127 || d.max_distance < 1 || !(d.eps > 0.f))
    return vt_fail(VT_ERR_ARG, "vt_t5_create: unsupported config (d_model, d_ff multiples of 64, d_model <= 4096, 1 <= num_buckets <= 127)");
  VtWeights W;
  CK(W.open("vt_t5_create", w, n, vt_t5_num_weights(desc)));
  vt_t5_s* h = new (std::nothrow) vt_t5_s();
  if (!h) return vt_fail(-12, "out of host memory");
  h->d = d;
  h->L.resize(d.layers);
  h->shared = W.next(); h->rel_bias = W.next_f32();
  for (auto& L : h->L) {
    L.ln1 = W.next_f32(); L.qkv_w = W.next(); L.o_w = W.next();
    L.ln2 = W.next_f32(); L.wi_w = W.next(); L.wo_w = W.next();
  }
  h->final_ln = W.next_f32();
  *out = h;
  return VT_OK;
}
void vt_t5_destroy(vt_t5_t h) { delete h; }

namespace {
struct TWs { size_t ids, mask, tok, xn, qkv, att, g, hf, total; };
TWs t5_carve(const vt_t5_s* h, int B, int L) {
  const vt_t5_desc& d = h->d;
  const size_t M = (size_t)B * L, a = vt_dt_bytes(d.adt), I = (size_t)d.heads * d.d_kv;
  TWs w; VtCarver cv;
  w.ids = cv.take(M * 4); w.mask = cv.take(M);
  w.tok = cv.take(M * d.d_model * 4);
  w.xn = cv.take(M * d.d_model * a);
  w.qkv = cv.take(M * 3 * I * a);
  w.att = cv.take(M * I * a);
  w.g = cv.take(M * 2 * d.d_ff * a);
  w.hf = cv.take(M * d.d_ff * a);
  w.total = cv.o;
  return w;
}
}  // namespace

size_t vt_t5_workspace_bytes(vt_t5_t h, int B, int L) { return h && B > 0 && L > 0 ? t5_carve(h, B, L).total : 0; }

int vt_t5_forward(vt_t5_t h, const int32_t* ids, const uint8_t* mask, int B, int L, const int8_t* bucket_tab, void* out, int out_dt, void* workspace,
                  vt_stream_t stream) {
  if (!h || !ids || !bucket_tab || !out || !workspace) return vt_fail(VT_ERR_ARG, "vt_t5_forward: null argument");
  if (B < 1 || L < 1) return vt_fail(VT_ERR_ARG, "vt_t5_forward: bad sizes B=%d L=%d", B, L);
  if (L > T5_MAX_L) return vt_fail(VT_ERR_ARG, "vt_t5_forward: L = %d exceeds %d", L, T5_MAX_L);
  if (out_dt != VT_F32 && out_dt != VT_BF16) return vt_fail(VT_ERR_ARG, "vt_t5_forward: out_dt must be fp32 (0) or bf16 (1)");
  const vt_t5_desc& d = h->d;
  // host-side validation of the token ids and the key mask (both host arrays)
  for (long r = 0; r < (long)B * L; ++r)
    if (ids[r] < 0 || ids[r] >= d.vocab) return vt_fail(VT_ERR_ARG, "vt_t5_forward: token id %d at position %ld is outside [0, %d)", ids[r], r, d.vocab);
  if (mask)
    for (int b = 0; b < B; ++b) {
      int any = 0;
      for (int l = 0; l < L; ++l) any |= mask[(long)b * L + l] != 0;
      if (!any) return vt_fail(VT_ERR_ARG, "vt_t5_forward: row %d of the attention mask has no valid token", b);
    }
  hipStream_t s = (hipStream_t)stream;
  const TWs w = t5_carve(h, B, L);
  char* ws = (char*)workspace;
  const int M = B * L, D = d.d_model, I = d.heads * d.d_kv, F = d.d_ff, cdt = d.cdt, adt = d.adt;
  if (hipMemcpyAsync(ws + w.ids, ids, (size_t)M * 4, hipMemcpyHostToDevice, s) != hipSuccess) return vt_fail(VT_ERR_LAUNCH, "vt_t5_forward: id upload");
  if (mask && hipMemcpyAsync(ws + w.mask, mask, (size_t)M, hipMemcpyHostToDevice, s) != hipSuccess) return vt_fail(VT_ERR_LAUNCH, "vt_t5_forward: mask upload");
  float* tok = (float*)(ws + w.tok);
  // the typed gather is chosen by hand between the two types `create` admits: DISPATCH_T (vt_common.h) would also instantiate it for half_t,
  // which no T5 handle can ask for
  if (cdt == VT_BF16) hipLaunchKernelGGL((t5_gather_kernel<bf16_t>), g1((long)M * D / 4), dim3(256), 0, s, (const int*)(ws + w.ids), (const bf16_t*)h->shared, tok, (long)M, D, d.vocab);
  else hipLaunchKernelGGL((t5_gather_kernel<float>), g1((long)M * D / 4), dim3(256), 0, s, (const int*)(ws + w.ids), (const float*)h->shared, tok, (long)M, D, d.vocab);
  CK(vt_wrap(vt_check_launch(), "t5 token gather"));
  const uint8_t* kmask = mask ? (const uint8_t*)(ws + w.mask) : nullptr;
  for (const T5Layer& Ly : h->L) {
    CK(vt_wrap(vt_k_rownorm(tok, VT_F32, D, ws + w.xn, adt, D, Ly.ln1, nullptr, M, D, d.eps, VT_NORM_RMS_MEANSQ, s), "t5 rms1"));
    { VtGemmParams p = vt_linear(ws + w.xn, adt, D, Ly.qkv_w, cdt, D, nullptr, ws + w.qkv, adt, 3 * I, M, 3 * I, D, VT_ACT_NONE);
      CK(vt_wrap(vt_gemm_launch(p, s), "t5 qkv")); }
    CK(vt_wrap(vt_t5_attention(ws + w.qkv, ws + w.att, bucket_tab, h->rel_bias, kmask, B, d.heads, L, d.num_buckets, adt, stream), "t5 attention"));
    { VtGemmParams p = vt_linear(ws + w.att, adt, I, Ly.o_w, cdt, I, nullptr, tok, VT_F32, D, M, D, I, VT_ACT_NONE);
      p.residual = tok; p.ldr = D;
      CK(vt_wrap(vt_gemm_launch(p, s), "t5 o")); }
    CK(vt_wrap(vt_k_rownorm(tok, VT_F32, D, ws + w.xn, adt, D, Ly.ln2, nullptr, M, D, d.eps, VT_NORM_RMS_MEANSQ, s), "t5 rms2"));
    { VtGemmParams p = vt_linear(ws + w.xn, adt, D, Ly.wi_w, cdt, D, nullptr, ws + w.g, adt, 2 * F, M, 2 * F, D, VT_ACT_NONE);
      CK(vt_wrap(vt_gemm_launch(p, s), "t5 wi")); }
    CK(vt_wrap(vt_t5_geglu(ws + w.g, (long)2 * F, ws + w.hf, (long)F, (long)M, F, adt, stream), "t5 geglu gate"));
    { VtGemmParams p = vt_linear(ws + w.hf, adt, F, Ly.wo_w, cdt, F, nullptr, tok, VT_F32, D, M, D, F, VT_ACT_NONE);
      p.residual = tok; p.ldr = D;
      CK(vt_wrap(vt_gemm_launch(p, s), "t5 wo")); }
  }
  CK(vt_wrap(vt_k_rownorm(tok, VT_F32, D, out, out_dt, D, h->final_ln, nullptr, M, D, d.eps, VT_NORM_RMS_MEANSQ, s), "t5 final norm"));
  return VT_OK;
}
