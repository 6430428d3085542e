// vt_gemm_tn.hip — the weight gradient of a Linear on 16-bit MFMA without a transposed copy of either operand (gfx950):
//   dW[N][K] = sum_m dy[m][n] x[m][k]   and, from the same launch,   db[N] = sum_m dy[m][n]
// for dy [M][N] and x [M][K], both bf16 or both fp16, token-major rows with unit inner stride and a row pitch of their own.  The product reduces
// over the LEADING index of both operands, the form vt_gemm (a[M][K] w[N][K]^T) does not have: the 16-bit trainer used to write dy^T and x^T to HBM
// (vt_transpose_pad), multiply them and sum dy's columns in a fourth launch.
//
// Tiling: a workgroup of 4 waves owns a 128 (n) x 128 (k) tile of dW for one row split; wave (wn, wk) owns its 64 x 64 quarter as 4 x 4 accumulators
// of v_mfma_f32_16x16x32.  The token rows are walked in m-steps of 32.  Per m-step both operand tiles, dy [32][128] and x [32][128], are staged
// ROW-MAJOR from HBM into LDS in 16-byte pieces (register prefetch of the next step, two LDS buffers, one barrier per step) and BOTH fragments are
// read with ds_read_b64_tr_b16: A = dy^T (n on the lane, m in the registers), B = x (k on the lane, m in the registers).  The 16 lanes of group g
// address rows hh * 16 + g * 4 + (l15 >> 2), columns c0 + (l15 & 3) * 4 .. + 3, and lane l15 receives rows hh * 16 + g * 4 .. + 3 of column
// c0 + l15; two reads (hh = 0, 1) fill the 8 elements of a fragment.  A and B use the same m -> (g, element) assignment, which is all an MFMA needs.
// Every lane always issues its read (EXEC all ones: the m-loop's trip count is uniform and nothing is predicated); ragged M / N / K edges are ZEROS
// in the LDS tile ("pad, don't mask"), and only the final global stores are predicated.
//
// LDS row pitch 288 B = 128 elements + 32 B of padding.  Bank rule (64 banks of 4 B for ds_read_b64_tr_b16, conflicts per 32-lane half): a half is two
// 16-lane groups = 8 tile rows r .. r + 7, in each of which 4 lanes read 32 contiguous bytes = 8 banks.  Row r's first bank is
// (288 r / 4 + c0 / 2) mod 64 = (8 r + 64 r + c0 / 2) mod 64 = (8 r + const) mod 64: eight consecutive rows start 8 banks apart and tile the 64 banks
// exactly once, so the transposed reads are conflict-free; 288 is a multiple of 16, so the 16-byte staging writes and the 8-byte read addresses
// stay aligned.
//
// db: the waves wk = 0 of the workgroups of the first k-tile column multiply their A fragments by a fragment of ones (1.0 is exact in both types),
// so db is summed by the same MFMA in the same order as a column of dW.
//
// Split over M (vt_gemm_tn_plan, a pure function of M, N, K): S row splits of `rows_per_split` rows on gridDim.z.  S = 1 stores dW / db directly.
// S > 1: split s stores its fp32 partial [N][K] and db partial [N] at ws + s (N K + N); gemm_tn_reduce_kernel then adds the S partials in split
// order and stores once.  No atomics, no counters, no flags, no hand-off inside a launch: the bits depend on the shapes only.
// Accumulation is fp32 throughout; the products are exact, so the only rounding is fp32 addition.
#include "vt_common.h"
#include "vt_host.h"
#include "../../include/vlatouch.h"

namespace {

constexpr int TN = 128, TK = 128;       // the workgroup's tile of dW
constexpr int BM = 32;                  // m-step: one MFMA k-step
constexpr int PITCH = 288;              // LDS row pitch in bytes (see the bank rule above)
constexpr int IMG = BM * PITCH;         // one operand tile
constexpr int FULL_WAVE = 256;          // workgroups the grid should reach: one per CU
constexpr int MIN_STEPS = 4;            // a split walks at least this many m-steps
constexpr int MAX_SPLITS = 16;

// fragment [column c0 + l15][rows (j >> 2) * 16 + g * 4 + (j & 3)] of a row-major [32][128] image; `off` = the lane's offset inside a 16-row slab
template <typename T>
__device__ __forceinline__ void tr_frag(Frag<T>& f, const char* img, unsigned off) {
#pragma unroll
  for (int hh = 0; hh < 2; ++hh) tr_frag_half(f, hh, img + hh * 16 * PITCH + off);
}

// out / dbout: dW and db (gridDim.z = 1, part_stride = 0) or the first split's partials in the workspace (part_stride = N K + N); dbout may be null
template <typename T>
__global__ __launch_bounds__(256) void gemm_tn_kernel(const T* __restrict__ dy, long ld_dy, const T* __restrict__ x, long ld_x, int M, int N, int K,
                                                      int rows_per_split, float* __restrict__ out, float* __restrict__ dbout, long part_stride) {
  __shared__ __attribute__((aligned(16))) char lds[2 * 2 * IMG];      // [buffer][dy tile | x tile]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, g = lane >> 4;
  const int wn = wave >> 1, wk = wave & 1;
  const int n0 = blockIdx.y * TN, k0 = blockIdx.x * TK;
  const int m_begin = blockIdx.z * rows_per_split, m_end = min(M, m_begin + rows_per_split);
  const int steps = (m_end - m_begin + BM - 1) / BM;
  float* o = out + blockIdx.z * part_stride;
  float* ob = dbout ? dbout + blockIdx.z * part_stride : nullptr;

  // staging: thread -> 16-byte chunk `sch` of tile rows srow and srow + 16 of both operands; N and K are multiples of 8, so a chunk is all in or all out
  const int srow = tid >> 4, sch = tid & 15;
  const bool dy_in = n0 + sch * 8 < N, x_in = k0 + sch * 8 < K;
  const T* dyp = dy + (long)(m_begin + srow) * ld_dy + n0 + sch * 8;
  const T* xp = x + (long)(m_begin + srow) * ld_x + k0 + sch * 8;
  uint4 rd[2], rx[2];
  auto fetch = [&](int step) {
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int r = step * BM + c * 16;                               // tile row srow + c * 16 of this step, relative to dyp / xp
      const bool live = m_begin + srow + r < m_end;
      rd[c] = make_uint4(0, 0, 0, 0);
      rx[c] = make_uint4(0, 0, 0, 0);
      if (live && dy_in) rd[c] = *reinterpret_cast<const uint4*>(dyp + (long)r * ld_dy);
      if (live && x_in) rx[c] = *reinterpret_cast<const uint4*>(xp + (long)r * ld_x);
    }
  };
  auto stash = [&](int buf) {
    char* base = lds + buf * 2 * IMG + srow * PITCH + sch * 16;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      *reinterpret_cast<uint4*>(base + c * 16 * PITCH) = rd[c];
      *reinterpret_cast<uint4*>(base + IMG + c * 16 * PITCH) = rx[c];
    }
  };

  float4_t acc[4][4], accb[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    accb[i] = (float4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (float4_t){0.f, 0.f, 0.f, 0.f};
  }
  const bool do_db = ob != nullptr && blockIdx.x == 0 && wk == 0;     // wave-uniform
  Frag<T> ones;
#pragma unroll
  for (int j = 0; j < 8; ++j) ones.v[j] = one16<T>();
  const unsigned troff = (unsigned)((g * 4 + (l15 >> 2)) * PITCH + (l15 & 3) * 8);
  const unsigned aoff = troff + (unsigned)(wn * 64 * 2), boff = troff + (unsigned)(IMG + wk * 64 * 2);

  fetch(0);
  stash(0);
  __syncthreads();
  for (int s = 0; s < steps; ++s) {
    const bool more = s + 1 < steps;                                  // uniform
    if (more) fetch(s + 1);
    const char* img = lds + (s & 1) * 2 * IMG;
    Frag<T> a[4], b[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      tr_frag(a[i], img, aoff + i * 32);
      tr_frag(b[i], img, boff + i * 32);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) mma16(acc[i][j], a[i], b[j]);
    if (do_db) {
#pragma unroll
      for (int i = 0; i < 4; ++i) mma16(accb[i], a[i], ones);
    }
    if (more) stash((s + 1) & 1);      // the other buffer: last read in step s - 1, which every wave left through the barrier below
    __syncthreads();
  }

  // accumulator (i, j), element r: dW[n0 + wn * 64 + i * 16 + g * 4 + r][k0 + wk * 64 + j * 16 + l15]
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int n = n0 + wn * 64 + i * 16 + g * 4 + r;
      if (n >= N) continue;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = k0 + wk * 64 + j * 16 + l15;
        if (k < K) o[(long)n * K + k] = acc[i][j][r];
      }
      if (do_db && l15 == 0) ob[n] = accb[i][r];
    }
  }
}

// dW = sum over the splits, in split order, of the partials at ws + s * part_stride (4 floats per thread); db likewise from offset N K when n4 > 0
__global__ __launch_bounds__(256) void gemm_tn_reduce_kernel(const float* __restrict__ ws, long part_stride, int S, float* __restrict__ dw, long nk4,
                                                             float* __restrict__ db, long n4) {
  const long i = blockIdx.x * 256L + threadIdx.x;
  if (i >= nk4 + n4) return;
  const bool is_db = i >= nk4;
  const long off = is_db ? nk4 * 4 + (i - nk4) * 4 : i * 4;
  float4_t v = *reinterpret_cast<const float4_t*>(ws + off);
  for (int s = 1; s < S; ++s) v += *reinterpret_cast<const float4_t*>(ws + s * part_stride + off);
  *reinterpret_cast<float4_t*>(is_db ? db + (i - nk4) * 4 : dw + off) = v;
}

}  // namespace

int vt_gemm_tn_plan(int M, int N, int K, VtGemmTnPlan* plan) {
  if (!plan) return vt_fail(VT_ERR_ARG, "vt_gemm_tn_plan: null plan");
  plan->splits = 0, plan->rows_per_split = 0, plan->m_step = BM, plan->ws_bytes = 0;
  if (M < 1 || N < 8 || K < 8 || N % 8 || K % 8)
    return vt_fail(VT_ERR_ARG, "vt_gemm_tn_plan: M = %d, N = %d, K = %d (M >= 1, N and K positive multiples of 8)", M, N, K);
  const long tn = (N + TN - 1) / TN, tk = (K + TK - 1) / TK;
  if (tn > 65535) return vt_fail(VT_ERR_ARG, "vt_gemm_tn_plan: N = %d is more than 65535 tiles", N);
  const long tiles = tn * tk, steps = ((long)M + BM - 1) / BM;
  long S = (FULL_WAVE + tiles - 1) / tiles;                 // splits that bring the grid to one workgroup per CU ...
  if (S > steps / MIN_STEPS) S = steps / MIN_STEPS;         // ... as far as every split still walks MIN_STEPS m-steps ...
  if (S > MAX_SPLITS) S = MAX_SPLITS;                       // ... and the workspace stays small
  if (S < 1) S = 1;
  const long rps = (steps + S - 1) / S * BM;
  S = ((long)M + rps - 1) / rps;                            // no empty split
  plan->splits = (int)S;
  plan->rows_per_split = (int)rps;
  plan->ws_bytes = S == 1 ? 0 : (long)vt_round256((size_t)(S * ((long)N * K + N) * 4));
  return VT_OK;
}

int vt_gemm_tn(const void* dy, long ld_dy, const void* x, long ld_x, int dt, int M, int N, int K, float* dw, float* db, void* ws, long ws_bytes,
               vt_stream_t s) {
  if (!dy || !x || !dw) return vt_fail(VT_ERR_ARG, "vt_gemm_tn: null pointer");
  if (dt != VT_BF16 && dt != VT_F16) return vt_fail(VT_ERR_ARG, "vt_gemm_tn: bf16 or fp16 operands only (dtype code %d)", dt);
  VtGemmTnPlan plan;
  if (vt_gemm_tn_plan(M, N, K, &plan) != VT_OK) return VT_ERR_ARG;
  if (ld_dy < N || ld_x < K || ld_dy % 8 || ld_x % 8)
    return vt_fail(VT_ERR_ARG, "vt_gemm_tn: row pitches %ld, %ld must be multiples of 8 elements and at least N = %d, K = %d", ld_dy, ld_x, N, K);
  if (((uintptr_t)dy | (uintptr_t)x | (uintptr_t)dw | (uintptr_t)db | (uintptr_t)ws) & 15)
    return vt_fail(VT_ERR_ARG, "vt_gemm_tn: base pointer not 16-byte aligned");
  if (plan.splits > 1 && (!ws || ws_bytes < plan.ws_bytes))
    return vt_fail(VT_ERR_ARG, "vt_gemm_tn: workspace has %ld bytes, %ld needed for %d row splits", ws ? ws_bytes : 0L, plan.ws_bytes, plan.splits);
  const dim3 grid((unsigned)((K + TK - 1) / TK), (unsigned)((N + TN - 1) / TN), (unsigned)plan.splits);
  const long nk = (long)N * K, part = plan.splits > 1 ? nk + N : 0;
  float* out = plan.splits > 1 ? (float*)ws : dw;
  float* dbout = !db ? nullptr : plan.splits > 1 ? (float*)ws + nk : db;
  DISPATCH_T16(dt, T, {                                    // bf16 or fp16: checked above
    hipLaunchKernelGGL(gemm_tn_kernel<T>, grid, dim3(256), 0, (hipStream_t)s, (const T*)dy, ld_dy, (const T*)x, ld_x, M, N, K, plan.rows_per_split,
                       out, dbout, part);
  })
  if (plan.splits > 1) {
    const long nk4 = nk / 4, n4 = db ? N / 4 : 0;
    hipLaunchKernelGGL(gemm_tn_reduce_kernel, dim3((unsigned)((nk4 + n4 + 255) / 256)), dim3(256), 0, (hipStream_t)s, (const float*)ws, part,
                       plan.splits, dw, nk4, db, n4);
  }
  return vt_check_launch();
}
