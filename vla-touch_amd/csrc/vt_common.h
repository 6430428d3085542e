// vt_common.h — shared device helpers for the gfx950 (CDNA4) kernels of libvlatouch_hip.so.
// Wave = 64 lanes.  MFMA fragment convention used everywhere in this library ("8-consecutive-k"):
//   a lane (row = lane & 15, g = lane >> 4) holds the 8 elements k = g*8 .. g*8+7 of a 32-wide k-step
//   for BOTH operands; C/D: lane holds D[(lane>>4)*4 + r][lane & 15], r = 0..3.
//   bf16 : one v_mfma_f32_16x16x32_bf16 per k-step.
//   f32  : eight v_mfma_f32_16x16x4_f32 (element j of every lane = one 4-deep slice); any consistent
//          k -> (slice, lane-group) assignment sums the same products, so both types share addressing.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

typedef uint16_t bf16_t;  // raw bits
typedef __attribute__((ext_vector_type(8))) short short8_t;
typedef __attribute__((ext_vector_type(4))) float float4_t;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8_t;
struct half_t { uint16_t b; };   // raw IEEE binary16 bits, a distinct type so templates can tell it from bf16_t
typedef __attribute__((ext_vector_type(4))) short short4_t;
typedef __attribute__((ext_vector_type(4))) int int4_t;
typedef __attribute__((ext_vector_type(16))) float float16_t;
// address spaces, as the LDS-DMA and transposing-read builtins want their pointers
typedef __attribute__((address_space(3))) void lds_void;
typedef const __attribute__((address_space(1))) void glb_void;
typedef __attribute__((address_space(3))) short4_t lds_short4_t;

#define VT_OK 0
#define VT_ERR_ARG (-22)
#define VT_ERR_LAUNCH (-5)
#define VT_ERR_UNSUPPORTED (-95)

// F32X3: fp32 storage, split-bf16 3-MFMA compute (GEMM weights only).  F16: IEEE half storage + v_mfma_f32_16x16x32_f16
// (same rate as bf16, 3 more mantissa bits; used where activations are range-bounded, i.e. the DINOv2 encoders).
enum { VT_F32 = 0, VT_BF16 = 1, VT_F32X3 = 2, VT_F16 = 3 };
enum { VT_ACT_NONE = 0, VT_ACT_GELU_ERF = 1, VT_ACT_GELU_TANH = 2, VT_ACT_SILU = 3, VT_ACT_MISH = 4,
       VT_ACT_SWIGLU = 5,      // not an element-wise epilogue: a ViT FFN form (vt_dino_desc.act): fc1 -> [x1 | x2], silu(x1) * x2, fc2 (HF Dinov2SwiGLUFFN)
       VT_ACT_GEGLU = 6,       // likewise, the T5 v1.1 gated-gelu FFN (vt_t5.hip): wi_0 | wi_1 -> gelu_tanh(a) * b, wo (HF T5DenseGatedActDense)
       VT_ACT_QUICK_GELU = 7 };   // element-wise: x * sigmoid(1.702 x) (HF "quick_gelu", the CLIP towers)

__device__ __forceinline__ float bf2f(bf16_t h) { return __uint_as_float(((uint32_t)h) << 16); }
typedef __attribute__((ext_vector_type(2))) float float2_t;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
// float -> bf16, round-to-nearest-even, NaN preserved: v_cvt_pk_bf16_f32 (one instruction per PAIR)
__device__ __forceinline__ uint32_t pk_bf16(float lo, float hi) {
  return __builtin_bit_cast(uint32_t, __builtin_convertvector((float2_t){lo, hi}, bf16x2_t));
}
typedef __attribute__((ext_vector_type(2))) _Float16 f16x2_t;
// two fp32 -> two T in one word, round-to-nearest-even (fp16: v_cvt_f16_f32 semantics, overflow gives inf)
template <typename T> __device__ __forceinline__ uint32_t pk16(float lo, float hi);
template <> __device__ __forceinline__ uint32_t pk16<bf16_t>(float lo, float hi) { return pk_bf16(lo, hi); }
template <> __device__ __forceinline__ uint32_t pk16<half_t>(float lo, float hi) {
  return __builtin_bit_cast(uint32_t, __builtin_convertvector((float2_t){lo, hi}, f16x2_t));
}
// 1.0 in the 16-bit type T (a fragment of ones sums its other operand on the matrix pipe)
template <typename T> __host__ __device__ constexpr short one16() { return std::is_same<T, half_t>::value ? (short)0x3C00 : (short)0x3F80; }
__device__ __forceinline__ bf16_t f2bf(float f) { return __builtin_bit_cast(bf16_t, (__bf16)f); }
__device__ __forceinline__ float h2f(half_t h) { return (float)__builtin_bit_cast(_Float16, h.b); }
__device__ __forceinline__ half_t f2h(float f) { half_t r; r.b = __builtin_bit_cast(uint16_t, (_Float16)f); return r; }   // v_cvt_f16_f32: RNE, saturates to inf

template <typename T> struct Elem;
template <> struct Elem<float> {
  static constexpr int EPC = 4;  // elements per 16-byte chunk
  __device__ static __forceinline__ float to_f(float v) { return v; }
  __device__ static __forceinline__ float from_f(float v) { return v; }
};
template <> struct Elem<bf16_t> {
  static constexpr int EPC = 8;
  __device__ static __forceinline__ float to_f(bf16_t v) { return bf2f(v); }
  __device__ static __forceinline__ bf16_t from_f(float v) { return f2bf(v); }
};
template <> struct Elem<half_t> {
  static constexpr int EPC = 8;
  __device__ static __forceinline__ float to_f(half_t v) { return h2f(v); }
  __device__ static __forceinline__ half_t from_f(float v) { return f2h(v); }
};

// 8-element fragment of compute type T
template <typename T> struct Frag;
template <> struct Frag<bf16_t> { short8_t v; };
template <> struct Frag<half_t> { short8_t v; };
template <> struct Frag<float> { float v[8]; };

__device__ __forceinline__ void mma16(float4_t& acc, const Frag<bf16_t>& a, const Frag<bf16_t>& b) {
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a.v), __builtin_bit_cast(bf16x8_t, b.v), acc, 0, 0, 0);
}
__device__ __forceinline__ void mma16(float4_t& acc, const Frag<half_t>& a, const Frag<half_t>& b) {
  acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, a.v), __builtin_bit_cast(f16x8_t, b.v), acc, 0, 0, 0);
}
__device__ __forceinline__ void mma16(float4_t& acc, const Frag<float>& a, const Frag<float>& b) {
#pragma unroll
  for (int j = 0; j < 8; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.v[j], b.v[j], acc, 0, 0, 0);
}

// v_mfma_f32_32x32x16: D[n][m] += W-fragment x A-fragment of the packed-weights GEMMs (vt_gemm_pw.hip, vt_gemm_pws.hip)
template <typename T16> __device__ __forceinline__ float16_t mma32(const int4_t w, const int4_t a, const float16_t c);
template <> __device__ __forceinline__ float16_t mma32<bf16_t>(const int4_t w, const int4_t a, const float16_t c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, w), __builtin_bit_cast(bf16x8_t, a), c, 0, 0, 0);
}
template <> __device__ __forceinline__ float16_t mma32<half_t>(const int4_t w, const int4_t a, const float16_t c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8_t, w), __builtin_bit_cast(f16x8_t, a), c, 0, 0, 0);
}

// compile-time loop: f(std::integral_constant<int, 0>{}) .. f(std::integral_constant<int, N - 1>{}).  Indices are constants by construction (a
// loop that the unroller gives up on would index register arrays dynamically and push them to scratch)
template <int N, typename F> __device__ __forceinline__ void static_for(F&& f) {
  if constexpr (N > 0) { static_for<N - 1>(f); f(std::integral_constant<int, N - 1>{}); }
}

// counted wait: at most N of this wave's vector-memory operations (loads, LDS-DMA and stores share the in-order counter on gfx950) stay in flight.
// The second form names the registers the wait retires (filled by loads hipcc does not see, wload) as "+v", which is what orders their uses behind
// it: ONE statement, so that no copy of them can be placed ahead of the wait.  A run-time count is an if-chain over compile-time counts.
// VLATOUCH_DRAIN_WAITS (debug build, tools/drain_waits_check.sh): every counted wait drains the whole queue — results must not change by a bit.
#ifdef VLATOUCH_DRAIN_WAITS
#define VT_VMCNT(N) 0
#else
#define VT_VMCNT(N) N
#endif
template <int N> __device__ __forceinline__ void vt_wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(VT_VMCNT(N)) : "memory"); }
template <int N> __device__ __forceinline__ void vt_wait_vm(int4_t (&w)[4]) {
  asm volatile("s_waitcnt vmcnt(%[n])" : "+v"(w[0]), "+v"(w[1]), "+v"(w[2]), "+v"(w[3]) : [n] "i"(VT_VMCNT(N)) : "memory");
}
template <int N> __device__ __forceinline__ void vt_wait_vm(int4_t (&w)[8]) {
  asm volatile("s_waitcnt vmcnt(%[n])" : "+v"(w[0]), "+v"(w[1]), "+v"(w[2]), "+v"(w[3]), "+v"(w[4]), "+v"(w[5]), "+v"(w[6]), "+v"(w[7]) : [n] "i"(VT_VMCNT(N)) : "memory");
}

// one KiB of fragment-packed weights -> 4 VGPRs per lane; saddr form: uniform 64-bit base + 32-bit lane offset + immediate.  The load is inline
// asm because hipcc drains the whole queue with vmcnt(0) at the first use of an ordinary VGPR load issued beside LDS-DMA; it does not see this
// one, whose completion is counted by hand (vt_wait_vm).  FIRST: the base SGPRs may come from a VALU readfirstlane -> 5 wait states.
template <int OFF, bool FIRST>
__device__ __forceinline__ void wload(int4_t& d, const unsigned voff, const char* sbase) {
  if constexpr (FIRST) asm volatile("s_nop 4\n\tglobal_load_dwordx4 %0, %1, %2 offset:%3" : "=v"(d) : "v"(voff), "s"(sbase), "i"(OFF) : "memory");
  else asm volatile("global_load_dwordx4 %0, %1, %2 offset:%3" : "=v"(d) : "v"(voff), "s"(sbase), "i"(OFF) : "memory");
}
// a wave-uniform `const char*` rebuilt in SGPRs for the saddr form (the builtin returns int: widen through unsigned, or a low half with bit 31
// set sign-extends into the high half).  A macro: as an inlined function it reorders hipcc's register definitions in gemm_pws_kernel.
#define VT_UNIFORM_PTR(p)                                                                                                             \
  reinterpret_cast<const char*>(((unsigned long)(unsigned)__builtin_amdgcn_readfirstlane((int)((unsigned long)(p) >> 32)) << 32) | \
                                (unsigned long)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned long)(p)))

// read an 8-element fragment from LDS rows of 8 16-byte chunks (128 B), chunk XOR-swizzled by row.
// `k8` = index of the 8-element group inside the row (0 .. 128/ (8*sizeof(T)) - 1).
__device__ __forceinline__ int swz(int row, int chunk) { return chunk ^ ((row >> 1) & 7); }

__device__ __forceinline__ void lds_frag(Frag<bf16_t>& f, const char* tile, int row, int k8) {
  f.v = *reinterpret_cast<const short8_t*>(tile + row * 128 + swz(row, k8) * 16);
}
__device__ __forceinline__ void lds_frag(Frag<half_t>& f, const char* tile, int row, int k8) {
  f.v = *reinterpret_cast<const short8_t*>(tile + row * 128 + swz(row, k8) * 16);
}
__device__ __forceinline__ void lds_frag(Frag<float>& f, const char* tile, int row, int k8) {
  const float4_t lo = *reinterpret_cast<const float4_t*>(tile + row * 128 + swz(row, 2 * k8) * 16);
  const float4_t hi = *reinterpret_cast<const float4_t*>(tile + row * 128 + swz(row, 2 * k8 + 1) * 16);
  f.v[0] = lo[0]; f.v[1] = lo[1]; f.v[2] = lo[2]; f.v[3] = lo[3];
  f.v[4] = hi[0]; f.v[5] = hi[1]; f.v[6] = hi[2]; f.v[7] = hi[3];
}

// transposing fragment read (ds_read_b64_tr_b16) from a row-major 16-bit image: the 16 lanes of a lane group address a [4 rows][16 columns] block
// (lane i: row i / 4, columns (i % 4) * 4 .. + 3) and the hardware hands lane i the 4 rows of column i = elements hh * 4 .. + 3 of the fragment.
// `a` = this lane's finished LDS address for half hh; row pitch, swizzle and slab arithmetic are the caller's.
template <typename T>
__device__ __forceinline__ void tr_frag_half(Frag<T>& f, const int hh, const char* a) {
  const short4_t t = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_short4_t*)a);
  f.v[hh * 4 + 0] = t[0]; f.v[hh * 4 + 1] = t[1]; f.v[hh * 4 + 2] = t[2]; f.v[hh * 4 + 3] = t[3];
}

// exp(x) on the hardware exp2 unit (v_exp_f32, ~1 ulp): the activations below are evaluated per output element of GEMM / GroupNorm
// epilogues, where libm's tanhf / log1pf / expf (30-60 instructions each) cost more than the GEMM's k-loop saves
__device__ __forceinline__ float fast_exp(float x) { return __builtin_amdgcn_exp2f(x * 1.4426950408889634f); }

// erf(x) by Abramowitz & Stegun 7.1.26 (|error| <= 1.5e-7 absolute, i.e. about one fp32 ulp of erf near 1; exact GELU differs from it by
// <= 0.5 |x| 1.5e-7) on the exp2 / rcp units: ~14 instructions where libm's erff is ~60 with branches.  The fc1 epilogue of a ViT applies
// it to M x 4D elements per layer: with erff the DINOv2-base fc1 launch (16448 x 3072 x 768) took 185 us against 99 us without activation.
__device__ __forceinline__ float fast_erf(float x) {
  const float ax = fabsf(x);
  const float t = __builtin_amdgcn_rcpf(1.0f + 0.3275911f * ax);
  const float p = t * (0.254829592f + t * (-0.284496736f + t * (1.421413741f + t * (-1.453152027f + t * 1.061405429f))));
  return copysignf(1.0f - p * fast_exp(-ax * ax), x);
}

__device__ __forceinline__ float act_apply(float x, int act) {
  switch (act) {
    case VT_ACT_GELU_ERF: return 0.5f * x * (1.0f + fast_erf(x * 0.70710678118654752440f));
    case VT_ACT_GELU_TANH: {
      // 0.5 x (1 + tanh(u)) == x * sigmoid(2u), u = sqrt(2/pi) (x + 0.044715 x^3)
      const float u2 = 1.5957691216057308f * (x + 0.044715f * x * x * x);
      return x * __builtin_amdgcn_rcpf(1.0f + fast_exp(-u2));
    }
    case VT_ACT_SILU: return x * __builtin_amdgcn_rcpf(1.0f + fast_exp(-x));
    case VT_ACT_QUICK_GELU: return x * __builtin_amdgcn_rcpf(1.0f + fast_exp(-1.702f * x));
    case VT_ACT_MISH: {
      // x tanh(log(1 + e^x)) == x w / (w + 2), w = e^x (e^x + 2)   (tanh(log s) = (s^2 - 1) / (s^2 + 1), s = 1 + e^x)
      if (x > 20.0f) return x;
      const float n = fast_exp(x), w = n * (n + 2.0f);
      return x * w * __builtin_amdgcn_rcpf(w + 2.0f);
    }
    default: return x;
  }
}

// sum / max over the 64 lanes, result in every lane.  Round 5: inside a row of 16 on DPP lane permutes, across the four rows on v_permlane16_swap /
// v_permlane32_swap — all VALU — instead of six __shfl_xor = ds_bpermute round trips through the LDS crossbar.
// rows_pair<W>: every lane's value combined with that of the lane W away (W = 16: rows (0,1) and (2,3); W = 32: the two halves of the wave).
template <int W, bool MAX> __device__ __forceinline__ float rows_pair(float v) {
  static_assert(W == 16 || W == 32, "a row is 16 lanes: pairs of rows, then pairs of pairs");
  const unsigned u = __builtin_bit_cast(unsigned, v);
  float a0, a1;
  if constexpr (W == 16) {
    const auto a = __builtin_amdgcn_permlane16_swap(u, u, false, false);
    a0 = __builtin_bit_cast(float, (unsigned)a[0]); a1 = __builtin_bit_cast(float, (unsigned)a[1]);
  } else {
    const auto a = __builtin_amdgcn_permlane32_swap(u, u, false, false);
    a0 = __builtin_bit_cast(float, (unsigned)a[0]); a1 = __builtin_bit_cast(float, (unsigned)a[1]);
  }
  return MAX ? fmaxf(a0, a1) : a0 + a1;
}
// over the four 16-lane rows of a wave (lanes that differ in bits 4 and 5)
__device__ __forceinline__ float rows4_sum(float v) { return rows_pair<32, false>(rows_pair<16, false>(v)); }
__device__ __forceinline__ float rows4_max(float v) { return rows_pair<32, true>(rows_pair<16, true>(v)); }
// sum over each aligned group of 16 lanes, result in every lane, on DPP lane permutes only (no LDS crossbar round trips as
// __shfl_xor would take): pairs inside quads, quads inside 8s (row_half_mirror pairs quad 0 <-> quad 1), 8s inside the row of 16
// (row_mirror); for a sum any pairing that covers the group works.
__device__ __forceinline__ float row16_sum(float v) {
  auto dpp = [](float x, auto ctrl) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), decltype(ctrl)::value, 0xf, 0xf, false));
  };
  v += dpp(v, std::integral_constant<int, 0xB1>{});    // quad_perm [1,0,3,2]
  v += dpp(v, std::integral_constant<int, 0x4E>{});    // quad_perm [2,3,0,1]
  v += dpp(v, std::integral_constant<int, 0x141>{});   // row_half_mirror
  v += dpp(v, std::integral_constant<int, 0x140>{});   // row_mirror
  return v;
}
__device__ __forceinline__ float row16_max(float v) {
  auto dpp = [](float x, auto ctrl) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), decltype(ctrl)::value, 0xf, 0xf, false));
  };
  v = fmaxf(v, dpp(v, std::integral_constant<int, 0xB1>{}));
  v = fmaxf(v, dpp(v, std::integral_constant<int, 0x4E>{}));
  v = fmaxf(v, dpp(v, std::integral_constant<int, 0x141>{}));
  v = fmaxf(v, dpp(v, std::integral_constant<int, 0x140>{}));
  return v;
}
__device__ __forceinline__ float wave_sum(float v) { return rows4_sum(row16_sum(v)); }
__device__ __forceinline__ float wave_max(float v) { return rows4_max(row16_max(v)); }

// generic typed load/store as float
template <typename T> __device__ __forceinline__ float ldf(const T* p, size_t i);
template <> __device__ __forceinline__ float ldf<float>(const float* p, size_t i) { return p[i]; }
template <> __device__ __forceinline__ float ldf<bf16_t>(const bf16_t* p, size_t i) { return bf2f(p[i]); }
template <> __device__ __forceinline__ float ldf<half_t>(const half_t* p, size_t i) { return h2f(p[i]); }
template <typename T> __device__ __forceinline__ void stf(T* p, size_t i, float v);
template <> __device__ __forceinline__ void stf<float>(float* p, size_t i, float v) { p[i] = v; }
template <> __device__ __forceinline__ void stf<bf16_t>(bf16_t* p, size_t i, float v) { p[i] = f2bf(v); }
template <> __device__ __forceinline__ void stf<half_t>(half_t* p, size_t i, float v) { p[i] = f2h(v); }

// normalize_actions / denormalize_actions of one value (controller_dataset.py:303-346: <1e-6 range guard / :349-384: no guard): the padded
// min-max range of its column mapped to [-1, 1].  One statement for actnorm_kernel (vt_kernels.hip) and ctrl_batch_kernel (vt_ctrl_data.hip),
// so that a batch assembled on the device carries the bits vt_action_normalize gives.
__device__ __forceinline__ float vt_actnorm(float x, float mn, float mx, float pad, int denorm) {
  const float pr = (mx - mn) * pad;
  const float ctr = (mn + mx) / 2;
  const float pmin = ctr - pr / 2, pmax = ctr + pr / 2;
  float rng = pmax - pmin;
  if (denorm) return (x + 1.0f) / 2.0f * rng + pmin;
  if (rng < 1e-6f) rng = 1.0f;
  return 2.0f * (x - pmin) / rng - 1.0f;
}

// (bit values: include/vlatouch.h)
#ifndef VT_RANGE_XN_SAT
#define VT_RANGE_XN_SAT 1u
#define VT_RANGE_NONFINITE 2u
#define VT_RANGE_GATE_SAT 4u
#define VT_RANGE_ATTN_EMPTY 8u
#endif
// sticky range-guard word of an engine (include/vlatouch.h: vt_rdt_set_range_flag): kernels OR bits in where a value left the 16-bit type's range; rare, relaxed, no return value
__device__ __forceinline__ void vt_range_note(unsigned* flag, unsigned bit) {
  if (flag) __hip_atomic_fetch_or(flag, bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ bool vt_nonfinite(float v) { return !(fabsf(v) <= 3.4028234664e38f); }      // inf or NaN

static inline int vt_check_launch() { return hipGetLastError() == hipSuccess ? VT_OK : VT_ERR_LAUNCH; }

// Host-side dispatch on a storage dtype code: the statement is compiled once per element type, with `T` naming it.  An unknown code falls to
// bf16_t, so an entry point that has to refuse one tests the code first (vt_is_act_dtype, or a condition of its own).  DISPATCH_T16 is the
// form for the kernels that exist for the two 16-bit types only (nothing is instantiated for float).
#define DISPATCH_T(dt, T, ...) \
  if ((dt) == VT_F32) { using T = float; __VA_ARGS__; } else if ((dt) == VT_F16) { using T = half_t; __VA_ARGS__; } else { using T = bf16_t; __VA_ARGS__; }
#define DISPATCH_T16(dt, T, ...) \
  if ((dt) == VT_F16) { using T = half_t; __VA_ARGS__; } else { using T = bf16_t; __VA_ARGS__; }
static inline bool vt_is_act_dtype(int dt) { return dt == VT_F32 || dt == VT_BF16 || dt == VT_F16; }      // the activation types of training: what DISPATCH_T names
