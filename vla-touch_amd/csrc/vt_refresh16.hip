// vt_refresh16.hip — the 16-bit trainer's weight refresh in one pass (gfx950): one read of an fp32 master W [N][K] (row pitch ldw) writes every 16-bit
// form the step multiplies with, whichever the caller asks for:
//   w16  [N][K]   row-major, the bits of vt_cast (act_copy_kernel: Elem<T>::from_f, round to nearest even, NaN as the conversion instruction gives it)
//   w16t [K][Np]  its transpose, Np = N rounded up to 8, the padding columns zero (vt_transpose_pad of w16)
//   wp            w16 in MFMA fragment order (vt_pack.h; what vt_pack_w32 writes for w16)
//   wtp           w16t, viewed [K][Np], in fragment order
// It replaces a cast launch, a transpose launch and (for the packed-weight small-M tile, vt_gemm_pws.hip) two packing launches per weight, and reads
// 4 bytes and writes up to 8 per parameter where those move 4 + 2, 2 + 2 and 2 x (2 + 2).  Bandwidth-bound: no arithmetic but the conversion.
//
// Tiling: a workgroup of 256 threads owns a 64 (n) x 64 (k) tile.
//   Pass 1, row-wise: thread t holds the 16-byte chunk k8 = t & 7 (8 consecutive k) of tile rows t >> 3 and (t >> 3) + 32: two 16-byte loads of the
//   master per chunk (8 lanes cover 256 contiguous bytes of a row), 8 conversions, and from the registers one 16-byte store each to w16 (8 lanes =
//   one whole 128-byte line of a row) and to wp (the chunk is the layout's unit: the 8 lanes that share k8 over 8 consecutive rows fill one
//   128-byte line of a fragment).  The chunk also goes to LDS, row-major, as 4 dwords (k, k + 1 in one dword).
//   Pass 2, transposed: thread t takes the k-pair kp = 8 * wave + ((lane >> 2) & 7) and the n-chunk c = (lane & 3) + 4 * (lane >> 5); it reads the
//   dwords (row 8 c + j, pair kp), j = 0 .. 7, regroups their low halves into the chunk (k = 2 kp, n = 8 c .. 8 c + 7) and their high halves into
//   the chunk of k + 1, and stores each with one 16-byte store to w16t (the lanes c = 0 .. 3 and, from the other half of the wave, c = 4 .. 7 fill the
//   128-byte line of a k row) and to wtp.  Rows n >= N are ZEROS in the LDS tile ("pad, don't mask"), which is w16t's zero padding.
//
// LDS row pitch 33 dwords = the tile's 32 dwords + 1 of padding (132 B; 8 448 B per workgroup).  Bank rule (ds_read_b32 / ds_write_b32: bank =
// dword address mod 32, conflicts among the 32 lanes of a wave half):
//   transposed read j: a half holds c = c0 .. c0 + 3 (c0 = 0 or 4) and eight consecutive pairs kp; the lane's dword is (8 c + j) 33 + kp, whose bank is
//   (8 c + j + kp) mod 32 because 8 * 33 = 264 = 8 (mod 32).  8 c takes {0, 8, 16, 24} (for c0 = 4: {32, 40, 48, 56} = the same residues) and kp adds
//   eight consecutive values, so the 32 lanes read 32 different banks: conflict-free.
//   row-wise write i: a half holds k8 = 0 .. 7 and four consecutive rows r; the dword is 33 r + 4 k8 + i, bank (r + 4 k8 + i) mod 32: four
//   consecutive values of r inside each step of 4: again 32 different banks.
// An unpadded pitch of 32 dwords would put all eight rows 8 c + j of a transposed read on one bank (8-way).  The 132-byte pitch is not a multiple of 16,
// so the tile is written with 4-byte and not 16-byte LDS stores; every global store is 16 bytes.
//
// Odd shapes: K % 8 != 0, a pitch that is not a multiple of 4 or a base that is not 16-byte aligned take the element-wise instantiation (VEC = false:
// scalar loads, scalar w16 stores); the packed forms do not exist there (vt_pack_w32 wants whole chunks) and w16t rows are always whole chunks (Np % 8 == 0).
#include "vt_common.h"
#include "vt_host.h"
#include "vt_pack.h"
#include "../../include/vlatouch.h"

namespace {

constexpr int TILE = 64;                // rows (n) and columns (k) of the workgroup's tile
constexpr int PITCH = TILE / 2 + 1;     // LDS row pitch in dwords (see the bank rule above)

template <typename T>
__device__ __forceinline__ uint32_t cvt2(float lo, float hi) {
  return (uint32_t)__builtin_bit_cast(uint16_t, Elem<T>::from_f(lo)) | ((uint32_t)__builtin_bit_cast(uint16_t, Elem<T>::from_f(hi)) << 16);
}

template <typename T, bool VEC>
__global__ __launch_bounds__(256) void refresh16_kernel(const float* __restrict__ W, const long ldw, const int N, const int K, const int Np,
                                                        uint16_t* __restrict__ w16, uint16_t* __restrict__ w16t, uint16_t* __restrict__ wp,
                                                        uint16_t* __restrict__ wtp) {
  __shared__ uint32_t tile[TILE * PITCH];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int k0 = blockIdx.x * TILE, n0 = blockIdx.y * TILE;

  // pass 1: row-wise
  const int k8 = tid & 7, k = k0 + k8 * 8;
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const int r = (tid >> 3) + 32 * e, n = n0 + r;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (n < N && k < K) {
      const float* src = W + (long)n * ldw + k;
      if constexpr (VEC) {                                          // K % 8 == 0: the chunk is all inside
        const float4 a = *reinterpret_cast<const float4*>(src), b = *reinterpret_cast<const float4*>(src + 4);
        v = make_uint4(cvt2<T>(a.x, a.y), cvt2<T>(a.z, a.w), cvt2<T>(b.x, b.y), cvt2<T>(b.z, b.w));
        if (w16) *reinterpret_cast<uint4*>(w16 + (long)n * K + k) = v;
        if (wp) *reinterpret_cast<uint4*>(wp + vt_pack_w32_chunk(n, k >> 3, K)) = v;
      } else {
        float f[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) f[i] = k + i < K ? src[i] : 0.f;
        v = make_uint4(cvt2<T>(f[0], f[1]), cvt2<T>(f[2], f[3]), cvt2<T>(f[4], f[5]), cvt2<T>(f[6], f[7]));
        if (w16) {
          const uint32_t d[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
          for (int i = 0; i < 8; ++i)
            if (k + i < K) w16[(long)n * K + k + i] = (uint16_t)(d[i >> 1] >> (16 * (i & 1)));
        }
      }
    }
    uint32_t* dst = tile + r * PITCH + k8 * 4;
    dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w;
  }
  if (!w16t && !wtp) return;                                        // uniform over the grid
  __syncthreads();

  // pass 2: transposed
  const int c = (lane & 3) + 4 * (lane >> 5), kp = 8 * wave + ((lane >> 2) & 7);
  const int kk = k0 + 2 * kp, nc = n0 + 8 * c;
  if (nc >= Np || kk >= K) return;
  uint32_t d[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) d[j] = tile[(8 * c + j) * PITCH + kp];
  uint4 o[2];
  o[0] = make_uint4((d[0] & 0xffffu) | (d[1] << 16), (d[2] & 0xffffu) | (d[3] << 16), (d[4] & 0xffffu) | (d[5] << 16), (d[6] & 0xffffu) | (d[7] << 16));
  o[1] = make_uint4((d[0] >> 16) | (d[1] & 0xffff0000u), (d[2] >> 16) | (d[3] & 0xffff0000u), (d[4] >> 16) | (d[5] & 0xffff0000u),
                    (d[6] >> 16) | (d[7] & 0xffff0000u));
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    if (kk + h >= K) break;
    if (w16t) *reinterpret_cast<uint4*>(w16t + (long)(kk + h) * Np + nc) = o[h];
    if (wtp) *reinterpret_cast<uint4*>(wtp + vt_pack_w32_chunk(kk + h, nc >> 3, Np)) = o[h];
  }
}

inline bool aligned16(const void* p) { return ((size_t)p & 15) == 0; }

}  // namespace

extern "C" int vt_refresh16(const float* W, long ldw, int N, int K, int dt, void* w16, void* w16t, void* wp, void* wtp, vt_stream_t stream) {
  if (!W || N < 1 || K < 1 || ldw < K) return vt_fail(VT_ERR_ARG, "vt_refresh16: null master, N or K below 1, or a pitch below K");
  if (dt != VT_BF16 && dt != VT_F16) return vt_fail(VT_ERR_ARG, "vt_refresh16: dtype %d is not a 16-bit type (1 bf16, 3 fp16)", dt);
  const int Np = (N + 7) / 8 * 8;
  if (wp && !vt_pack_w32_shape_ok(N, K)) return vt_fail(VT_ERR_ARG, "vt_refresh16: wp wants N %% 32 == 0 and K %% 16 == 0, got N = %d, K = %d", N, K);
  if (wtp && !vt_pack_w32_shape_ok(K, Np)) return vt_fail(VT_ERR_ARG, "vt_refresh16: wtp wants K %% 32 == 0 and Np %% 16 == 0, got K = %d, Np = %d", K, Np);
  if (!aligned16(w16t) || !aligned16(wp) || !aligned16(wtp)) return vt_fail(VT_ERR_ARG, "vt_refresh16: w16t, wp and wtp must be 16-byte aligned");
  if (!w16 && !w16t && !wp && !wtp) return VT_OK;
  const bool vec = K % 8 == 0 && ldw % 4 == 0 && aligned16(W) && aligned16(w16);
  if (!vec && wp) return vt_fail(VT_ERR_ARG, "vt_refresh16: wp wants a 16-byte aligned master and w16 and a pitch that is a multiple of 4");
  const dim3 grid((unsigned)((K + TILE - 1) / TILE), (unsigned)((N + TILE - 1) / TILE));
  if (grid.y > 65535u) return vt_fail(VT_ERR_ARG, "vt_refresh16: N = %d is above 64 * 65535", N);
#define VT_REFRESH16_GO(T, VEC) hipLaunchKernelGGL((refresh16_kernel<T, VEC>), grid, dim3(256), 0, (hipStream_t)stream, W, ldw, N, K, Np, \
                                                   (uint16_t*)w16, (uint16_t*)w16t, (uint16_t*)wp, (uint16_t*)wtp)
  DISPATCH_T16(dt, T, if (vec) VT_REFRESH16_GO(T, true); else VT_REFRESH16_GO(T, false))
#undef VT_REFRESH16_GO
  return vt_check_launch();
}
