// vt_jpegdec.hip — baseline JPEG files decoded on the device, bit-identical to libjpeg's default decompress (islow inverse DCT, fancy h2v2
// up-sampling), so that camera frames can stay in HBM as the bitstreams they were recorded as (vlatouch/jpegdec.py).  The host parses the
// markers, un-stuffs FF 00, removes the RSTn markers and builds the tables; everything behind that runs here.  Three components, 4:2:0 or
// 4:4:4, one interleaved scan.  Everything behind the entropy decoder is shared with vt_jpegmap.hip (vt_jpeg.h).
//
// A frame is one row of an int64 [n][VT_JPEG_K] table (include/vlatouch.h): device pointers of its un-stuffed stream, its table set, its
// entries and its restart starts, and its sizes and offsets.  An ENTRY is {bit offset in the stream, the three DC predictors} before MCU
// e * interval: a lane that starts there decodes what a sequential decoder would.
//   table set (kTsBytes, built by the host, copied to LDS by every workgroup of the two entropy kernels):
//     int32 sel[8]            DC table 0 | 1 of component 0..2, AC table 0 | 1 of component 0..2
//     uint16 q[3][64]         the quantisation table of component 0..2, natural order
//     4 Huffman tables (DC 0, DC 1, AC 0, AC 1), each: uint16 lut[512] = length << 8 | symbol by the next 9 bits (0: the code is longer or
//                             undefined), int32 maxcode[17], int32 valoff[17] (= valptr - mincode), uint8 huffval[256]: jdhuff.c's tables
//     uint8 zz[64]            zig-zag position -> natural order
//
// Launches:
//   jpeg_index_kernel     (vt_jpeg_index, once per upload) one lane per restart interval (a stream without DRI is one interval): walks its
//                         MCUs without storing coefficients and writes the entry of every MCU that is a multiple of `interval`.
//   jpeg_entropy_kernel   one lane per entry, 64 consecutive entries of one frame per wave: Huffman-decodes its MCUs into int16 coefficients
//                         in natural order (zero the block, then scatter).  The bit reader is a 64-bit register buffer refilled by
//                         byte-swapped word loads; a symbol's extra bits come out of the same buffer as its code.
//   jpeg_idct_kernel      64 lanes = 8 blocks: dequantise, inverse columns | LDS ([8][9] words a block, as vt_jpegmap) | inverse rows -> 8
//                         decoded bytes of the planes Y' | Cb' | Cr' (4:2:0: vt_jpegmap's layout; 4:4:4: three planes [H8][W8]).
//   jpeg_upsample_kernel  4:2:0: vt_jpegmap's up-sampling + conversion item.      jpeg_colour_kernel  4:4:4: the conversion alone.
// Reads are bounded by construction: a stream word is loaded only below the stream's padded length (the host pads with FF to a multiple of
// 4; past it the reader sees 1-bits, as libjpeg pads), a coefficient index is checked against 63 before it is used, a lane's MCU count comes
// from the table.  An undefined code, a run past coefficient 63 or the stream's end before a lane's MCUs are done sets status[frame] (plain
// store, only ever non-zero) and the lane zero-fills the rest of its MCUs.
#include <stdint.h>
#include <initializer_list>
#include "vt_common.h"
#include "vt_frames.h"
#include "vt_jpeg.h"
#include "vt_pixel.h"
#include "../../include/vlatouch.h"

namespace {
constexpr int kK = VT_JPEG_K;
// columns of a table row
enum { cStream, cLen, cH, cW, cSamp, cTset, cEntries, cInterval, cRi, cRst, cOutOff, cCoefOff, cPlanesOff };
// byte offsets inside a table set
constexpr int kTsSel = 0, kTsQ = 32, kTsHuff = 416, kHuffBytes = 1416, kHuffMax = 1024, kHuffOff = 1092, kHuffVal = 1160;
constexpr int kTsZZ = kTsHuff + 4 * kHuffBytes, kTsBytes = kTsZZ + 64;
static_assert(kTsBytes == VT_JPEG_TABLESET_BYTES, "the table set of include/vlatouch.h");
constexpr int kNT = 256;             // threads per block of the pixel launches
constexpr long kMaxStream = 1L << 28;

struct Frame {
  const uint8_t* s;
  uint32_t len, plen;      // true and padded (multiple of 4) bytes of the un-stuffed stream
  int h, w, samp;
  const uint8_t* tset;
  int4* entries;
  int interval, ri;
  const int* rst;
  long out_off, coef_off, planes_off;
  int mw, mcus, bpm, nent, nrst;
};
__host__ __device__ inline Frame frame_of(const long long* r) {
  Frame f;
  f.s = (const uint8_t*)r[cStream]; f.len = (uint32_t)r[cLen]; f.plen = (f.len + 3u) & ~3u;
  f.h = (int)r[cH]; f.w = (int)r[cW]; f.samp = (int)r[cSamp];
  f.tset = (const uint8_t*)r[cTset]; f.entries = (int4*)r[cEntries];
  f.interval = (int)r[cInterval]; f.ri = (int)r[cRi]; f.rst = (const int*)r[cRst];
  f.out_off = r[cOutOff]; f.coef_off = r[cCoefOff]; f.planes_off = r[cPlanesOff];
  const int sh = f.samp ? 4 : 3;                       // MCU side: 16 or 8 pixels
  f.mw = (f.w + (1 << sh) - 1) >> sh;
  f.mcus = f.mw * ((f.h + (1 << sh) - 1) >> sh);
  f.bpm = f.samp ? 6 : 3;
  f.nent = (f.mcus + f.interval - 1) / f.interval;
  f.nrst = f.ri ? (f.mcus + f.ri - 1) / f.ri : 1;
  return f;
}
// bytes of a frame's coefficient and plane workspaces
inline size_t coef_bytes(const Frame& f) { return (size_t)f.mcus * f.bpm * 128; }
inline size_t planes_bytes(const Frame& f) { return (size_t)f.mcus * f.bpm * 64; }

struct BitReader {
  const uint8_t* s;
  uint32_t plen, wpos;     // padded stream bytes; byte offset of the next word
  uint64_t buf;            // the next `cnt` bits of the stream, left-aligned, zeros behind them
  int cnt;
  __device__ __forceinline__ uint32_t word() {
    uint32_t w = 0xffffffffu;
    if (wpos < plen) w = __builtin_bswap32(*(const uint32_t*)(s + wpos));
    wpos += 4;
    return w;
  }
  __device__ __forceinline__ void init(const uint8_t* s_, const uint32_t plen_, const uint32_t bitpos) {
    s = s_; plen = plen_; wpos = (bitpos >> 5) << 2;
    buf = (uint64_t)word() << 32;
    const int k = bitpos & 31;
    buf <<= k; cnt = 32 - k;
  }
  // at least 33 bits behind it: one code (<= 16) and its extra bits (<= 15)
  __device__ __forceinline__ void refill() {
    if (cnt <= 32) { buf |= (uint64_t)word() << (32 - cnt); cnt += 32; }
  }
  __device__ __forceinline__ void skip(const int n) { buf <<= n; cnt -= n; }
  __device__ __forceinline__ uint64_t consumed() const { return (uint64_t)wpos * 8 - (uint64_t)cnt; }
};

// the next symbol of Huffman table `tab` (LDS): its code length in l (0: undefined code)
__device__ __forceinline__ int next_symbol(const BitReader& br, const uint8_t* tab, int& l) {
  const uint32_t e = ((const uint16_t*)tab)[br.buf >> 55];
  l = e >> 8;
  if (l) return e & 255;
  const int* maxcode = (const int*)(tab + kHuffMax);
  int code = 0;
  for (l = 10; l <= 16; ++l) {
    code = (int)(br.buf >> (64 - l));
    if (code <= maxcode[l]) break;
  }
  if (l > 16) { l = 0; return 0; }
  return tab[kHuffVal + ((code + ((const int*)(tab + kHuffOff))[l]) & 255)];
}
// the s extra bits behind a code of l bits, sign-extended (jdhuff.c HUFF_EXTEND); s in 1..15
__device__ __forceinline__ int extra_bits(const BitReader& br, const int l, const int s) {
  const int v = (int)((br.buf << l) >> (64 - s));
  return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
}

// one 8 x 8 block; STORE: its non-zero coefficients go to cw[0..64) in natural order (zeroed by the caller).  false: the stream is broken.
template <bool STORE>
__device__ __forceinline__ bool decode_block(BitReader& br, const uint8_t* dc, const uint8_t* ac, const uint8_t* zz, int& pred, int16_t* cw) {
  int l;
  br.refill();
  int s = next_symbol(br, dc, l);
  if (l == 0 || s > 15) return false;
  if (s) pred += extra_bits(br, l, s);
  br.skip(l + s);
  if (STORE) cw[0] = (int16_t)pred;
  for (int k = 1; k < 64;) {
    br.refill();
    const int rs = next_symbol(br, ac, l);
    if (l == 0) return false;
    s = rs & 15;
    if (s == 0) {
      br.skip(l);
      if ((rs >> 4) != 15) break;      // end of block
      k += 16;
      continue;
    }
    k += rs >> 4;
    if (k > 63) return false;
    if (STORE) cw[zz[k]] = (int16_t)extra_bits(br, l, s);
    br.skip(l + s);
    ++k;
  }
  return true;
}

// MCUs [m0, m1) of frame f from reader / predictor state; STORE: into coefficients; else entries are written.  Returns whether it broke.
template <bool STORE>
__device__ __forceinline__ bool walk_mcus(const Frame& f, const uint8_t* ts, BitReader& br, int p0, int p1, int p2, const int m0, const int m1,
                                          uint8_t* ws) {
  const int* sel = (const int*)(ts + kTsSel);
  const uint8_t* zz = ts + kTsZZ;
  int16_t* cw = STORE ? (int16_t*)(ws + f.coef_off) + (long)m0 * f.bpm * 64 : nullptr;
  bool bad = false;
  for (int m = m0; m < m1; ++m) {
    if (STORE && f.ri && m > m0 && m % f.ri == 0) {      // an entry that straddles a restart: byte aligned, predictors 0
      br.init(f.s, f.plen, (uint32_t)f.rst[m / f.ri] << 3);
      p0 = p1 = p2 = 0;
    }
    if (!STORE && m % f.interval == 0) f.entries[m / f.interval] = make_int4((int)(uint32_t)br.consumed(), p0, p1, p2);
    for (int k = 0; k < f.bpm; ++k, cw += STORE ? 64 : 0) {
      const int c = f.samp ? (k < 4 ? 0 : k - 3) : k;
      if (STORE) {
#pragma unroll
        for (int q = 0; q < 8; ++q) ((uint4*)cw)[q] = make_uint4(0, 0, 0, 0);
      }
      if (bad) continue;
      int pred = c == 0 ? p0 : (c == 1 ? p1 : p2);
      bad = !decode_block<STORE>(br, ts + kTsHuff + sel[c] * kHuffBytes, ts + kTsHuff + (2 + sel[3 + c]) * kHuffBytes, zz, pred, cw);
      bad = bad || br.consumed() > (uint64_t)f.len * 8;
      if (c == 0) p0 = pred; else if (c == 1) p1 = pred; else p2 = pred;
      if (STORE && bad) {
#pragma unroll
        for (int q = 0; q < 8; ++q) ((uint4*)cw)[q] = make_uint4(0, 0, 0, 0);
      }
    }
  }
  return bad;
}

__device__ __forceinline__ void load_tableset(const uint8_t* tset, uint32_t* lds) {
  for (int i = threadIdx.x; i < kTsBytes / 4; i += 64) lds[i] = ((const uint32_t*)tset)[i];
  __syncthreads();
}

__global__ void __launch_bounds__(64) jpeg_index_kernel(const long long* __restrict__ table, int* __restrict__ status) {
  const Frame f = frame_of(table + (long)blockIdx.y * kK);
  if ((int)blockIdx.x * 64 >= f.nrst) return;            // block-uniform
  __shared__ uint32_t lds[kTsBytes / 4];
  load_tableset(f.tset, lds);
  const int r = blockIdx.x * 64 + threadIdx.x;
  if (r >= f.nrst) return;
  const int m0 = f.ri ? r * f.ri : 0, m1 = f.ri ? min(m0 + f.ri, f.mcus) : f.mcus;
  BitReader br;
  br.init(f.s, f.plen, (uint32_t)f.rst[r] << 3);
  if (walk_mcus<false>(f, (const uint8_t*)lds, br, 0, 0, 0, m0, m1, nullptr)) status[blockIdx.y] = 1;
}

__global__ void __launch_bounds__(64) jpeg_entropy_kernel(const long long* __restrict__ table, uint8_t* __restrict__ ws, int* __restrict__ status) {
  const Frame f = frame_of(table + (long)blockIdx.y * kK);
  if ((int)blockIdx.x * 64 >= f.nent) return;            // block-uniform
  __shared__ uint32_t lds[kTsBytes / 4];
  load_tableset(f.tset, lds);
  const int e = blockIdx.x * 64 + threadIdx.x;
  if (e >= f.nent) return;
  const int4 en = f.entries[e];
  BitReader br;
  br.init(f.s, f.plen, (uint32_t)en.x);
  const int m0 = e * f.interval;
  if (walk_mcus<true>(f, (const uint8_t*)lds, br, en.y, en.z, en.w, m0, min(m0 + f.interval, f.mcus), ws)) status[blockIdx.y] = 1;
}

__global__ void __launch_bounds__(64) jpeg_idct_kernel(const long long* __restrict__ table, uint8_t* __restrict__ ws) {
  const Frame f = frame_of(table + (long)blockIdx.y * kK);
  const int nblk = f.mcus * f.bpm;
  if ((int)blockIdx.x * 8 >= nblk) return;               // block-uniform
  constexpr int kRow = 9, kBlk = 8 * kRow;               // words per row and per block in LDS: both passes touch every bank once per 32 lanes
  __shared__ int blk[8 * kBlk];
  const int b = threadIdx.x >> 3, v = threadIdx.x & 7;
  const int gb = blockIdx.x * 8 + b;
  const bool live = gb < nblk;
  const int mcu = live ? gb / f.bpm : 0, k = live ? gb - mcu * f.bpm : 0;
  const int c = f.samp ? (k < 4 ? 0 : k - 3) : k;
  int d[8];
  if (live) {        // column v: dequantise, inverse columns
    const int16_t* cw = (const int16_t*)(ws + f.coef_off) + (long)gb * 64 + v;
    const uint16_t* q = (const uint16_t*)(f.tset + kTsQ) + c * 64 + v;
#pragma unroll
    for (int j = 0; j < 8; ++j) d[j] = (int)cw[8 * j] * (int)q[8 * j];
    idct8<11>(d);
#pragma unroll
    for (int j = 0; j < 8; ++j) blk[b * kBlk + j * kRow + v] = d[j];
  }
  __syncthreads();
  if (!live) return;
#pragma unroll
  for (int j = 0; j < 8; ++j) d[j] = blk[b * kBlk + v * kRow + j];      // row v: inverse rows -> 8 decoded samples
  idct8<18>(d);
  uint32_t lo = 0, hi = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    lo |= (uint32_t)clip8(d[j] + 128) << (8 * j);
    hi |= (uint32_t)clip8(d[j + 4] + 128) << (8 * j);
  }
  const int my = mcu / f.mw, mx = mcu - my * f.mw;
  uint8_t* base = ws + f.planes_off;
  uint8_t* dp;
  if (f.samp) {
    const PlaneGeom g = plane_geom(f.h, f.w);
    if (k < 4) dp = base + (long)(my * 16 + (k >> 1) * 8 + v) * g.W16 + mx * 16 + (k & 1) * 8;
    else dp = base + (k == 4 ? g.cb : g.cr) + (long)(my * 8 + v) * (g.W16 >> 1) + mx * 8;
  } else {
    const long W8 = (long)f.mw * 8;
    dp = base + (long)c * (f.mcus * 64L) + (my * 8 + v) * W8 + mx * 8;
  }
  *(uint2*)dp = make_uint2(lo, hi);      // 8-byte aligned: planes_off is a multiple of 256, every plane pitch of 8
}

__global__ void __launch_bounds__(kNT) jpeg_upsample_kernel(const long long* __restrict__ table, const uint8_t* __restrict__ ws, uint8_t* __restrict__ out) {
  const Frame f = frame_of(table + (long)blockIdx.y * kK);
  if (!f.samp) return;
  jpeg_upsample_item(ws + f.planes_off, f.h, f.w, 0, (long)blockIdx.x * kNT + threadIdx.x, out + f.out_off);
}

// 4:4:4: one lane = 4 pixels of a row
__global__ void __launch_bounds__(kNT) jpeg_colour_kernel(const long long* __restrict__ table, const uint8_t* __restrict__ ws, uint8_t* __restrict__ out) {
  const Frame f = frame_of(table + (long)blockIdx.y * kK);
  if (f.samp) return;
  const int ipr = (f.w + 3) >> 2;
  const long it = (long)blockIdx.x * kNT + threadIdx.x;
  if (it >= (long)f.h * ipr) return;
  const int y = (int)(it / ipr), x0 = (int)(it - (long)y * ipr) * 4;
  const long W8 = (long)f.mw * 8, plane = f.mcus * 64L;
  const uint8_t* p = ws + f.planes_off + y * W8 + x0;          // x0 is a multiple of 4 inside the padded plane
  const uint32_t yw = *(const uint32_t*)p, bw = *(const uint32_t*)(p + plane), rw = *(const uint32_t*)(p + 2 * plane);
  uint32_t px[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) px[k] = ycc_px((yw >> (8 * k)) & 255, (int)((bw >> (8 * k)) & 255) - 128, (int)((rw >> (8 * k)) & 255) - 128, 0);
  store_px4(out + f.out_off + ((long)y * f.w + x0) * 3, px, min(4, f.w - x0));
}

// the checks of one row that every entry point makes; 0 or VT_ERR_ARG with the message set
int check_row(const char* fn, const long long* r, const int i) {
  if (r[cH] < 1 || r[cW] < 1) return vt_fail(VT_ERR_ARG, "%s: frame %d has a zero size (%lld x %lld)", fn, i, r[cH], r[cW]);
  if (r[cH] > kJpegMaxSide || r[cW] > kJpegMaxSide)
    return vt_fail(VT_ERR_ARG, "%s: frame %d of %lld x %lld is too large (at most %d a side)", fn, i, r[cH], r[cW], kJpegMaxSide);
  if (r[cSamp] != VT_JPEG_444 && r[cSamp] != VT_JPEG_420) return vt_fail(VT_ERR_ARG, "%s: frame %d: sampling code %lld", fn, i, r[cSamp]);
  for (const int c : {cStream, cTset, cEntries, cRst})
    if (!r[c] || (r[c] & (c == cEntries ? 15 : 3)))
      return vt_fail(VT_ERR_ARG, "%s: frame %d: column %d is a null or misaligned device pointer", fn, i, c);
  if (r[cLen] < 0 || r[cLen] >= kMaxStream) return vt_fail(VT_ERR_ARG, "%s: frame %d: stream of %lld bytes", fn, i, r[cLen]);
  if (r[cInterval] < 1 || r[cInterval] > INT32_MAX) return vt_fail(VT_ERR_ARG, "%s: frame %d: entry interval %lld", fn, i, r[cInterval]);
  const Frame f = frame_of(r);
  if (r[cInterval] > f.mcus) return vt_fail(VT_ERR_ARG, "%s: frame %d: entry interval %lld is not in 1..%d MCUs", fn, i, r[cInterval], f.mcus);
  if (r[cRi] < 0 || r[cRi] > 65535) return vt_fail(VT_ERR_ARG, "%s: frame %d: restart interval %lld", fn, i, r[cRi]);
  return VT_OK;
}
int check_table(const char* fn, const long long* table_host, int n) {
  CK(vt_frames_call_check(fn, table_host, n, 0, 0));
  for (int i = 0; i < n; ++i) CK(check_row(fn, table_host + (long)i * kK, i));
  return VT_OK;
}
}  // namespace

extern "C" size_t vt_jpeg_workspace_bytes(long long* table_host, int n) {
  if (check_table("vt_jpeg_workspace_bytes", table_host, n)) return 0;
  VtCarver ws;
  for (int i = 0; i < n; ++i) {
    long long* r = table_host + (long)i * kK;
    const Frame f = frame_of(r);
    r[cCoefOff] = (long long)ws.take(coef_bytes(f));
    r[cPlanesOff] = (long long)ws.take(planes_bytes(f));
  }
  return ws.o;
}

extern "C" int vt_jpeg_index(const long long* table_host, const void* table_dev, int n, void* status, vt_stream_t stream) {
  CK(check_table("vt_jpeg_index", table_host, n));
  if (!table_dev || !status) return vt_fail(VT_ERR_ARG, "vt_jpeg_index: null device table or status");
  int max_rst = 1;
  for (int i = 0; i < n; ++i) {
    const Frame f = frame_of(table_host + (long)i * kK);
    max_rst = f.nrst > max_rst ? f.nrst : max_rst;
  }
  hipLaunchKernelGGL(jpeg_index_kernel, dim3((unsigned)((max_rst + 63) / 64), n), dim3(64), 0, (hipStream_t)stream, (const long long*)table_dev,
                     (int*)status);
  return vt_frames_launched("vt_jpeg_index");
}

extern "C" int vt_jpeg_decode(const long long* table_host, const void* table_dev, int n, void* out, void* ws, size_t ws_bytes, void* status,
                              vt_stream_t stream) {
  CK(check_table("vt_jpeg_decode", table_host, n));
  if (!status) return vt_fail(VT_ERR_ARG, "vt_jpeg_decode: null status");
  int max_ent = 1, max_blk = 1;
  long items420 = 0, items444 = 0;
  VtCarver need;
  for (int i = 0; i < n; ++i) {
    const long long* r = table_host + (long)i * kK;
    const Frame f = frame_of(r);
    if (r[cOutOff] < 0) return vt_fail(VT_ERR_ARG, "vt_jpeg_decode: frame %d: negative out_off", i);
    // the layout vt_jpeg_workspace_bytes wrote: the kernels store there, so a table that did not pass through it is refused
    const long long co = (long long)need.take(coef_bytes(f)), po = (long long)need.take(planes_bytes(f));
    if (r[cCoefOff] != co || r[cPlanesOff] != po)
      return vt_fail(VT_ERR_ARG, "vt_jpeg_decode: frame %d: workspace offsets %lld, %lld are not the ones vt_jpeg_workspace_bytes writes", i,
                     r[cCoefOff], r[cPlanesOff]);
    max_ent = f.nent > max_ent ? f.nent : max_ent;
    max_blk = f.mcus * f.bpm > max_blk ? f.mcus * f.bpm : max_blk;
    long& items = f.samp ? items420 : items444;
    const long it = f.samp ? jpeg_upsample_items(f.h, f.w) : (long)f.h * ((f.w + 3) >> 2);
    items = it > items ? it : items;
  }
  CK(vt_frames_buffers_check("vt_jpeg_decode", table_dev, out, ws, ws_bytes, need.o, true));
  if ((uintptr_t)ws & 15) return vt_fail(VT_ERR_ARG, "vt_jpeg_decode: the workspace must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const long long* td = (const long long*)table_dev;
  hipLaunchKernelGGL(jpeg_entropy_kernel, dim3((unsigned)((max_ent + 63) / 64), n), dim3(64), 0, st, td, (uint8_t*)ws, (int*)status);
  hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)((max_blk + 7) / 8), n), dim3(64), 0, st, td, (uint8_t*)ws);
  if (items420)
    hipLaunchKernelGGL(jpeg_upsample_kernel, dim3((unsigned)((items420 + kNT - 1) / kNT), n), dim3(kNT), 0, st, td, (const uint8_t*)ws, (uint8_t*)out);
  if (items444)
    hipLaunchKernelGGL(jpeg_colour_kernel, dim3((unsigned)((items444 + kNT - 1) / kNT), n), dim3(kNT), 0, st, td, (const uint8_t*)ws, (uint8_t*)out);
  return vt_frames_launched("vt_jpeg_decode");
}
