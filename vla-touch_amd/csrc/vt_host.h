// vt_host.h — what the host drivers share, stated once: error plumbing (thread-local last-error string), CK, the element size of a dtype code, the
// workspace carver, and the checks and weight cursor of a `create`.  (The zeroed Linear parameter block sits beside VtGemmParams: vt_gemm.h.)
#pragma once
#include <stdarg.h>
#include <stddef.h>
#include <stdio.h>
#include "vt_common.h"

inline char* vt_errbuf() { static thread_local char buf[512] = "ok"; return buf; }
inline int vt_fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(vt_errbuf(), 512, fmt, ap);
  va_end(ap);
  return code;
}
// annotate a failing launch code from a lower layer
inline int vt_wrap(int code, const char* what) {
  if (code) {
    char tmp[400];
    snprintf(tmp, sizeof(tmp), "%s", vt_errbuf());
    snprintf(vt_errbuf(), 512, "%s failed (%d): %s", what, code, tmp);
  }
  return code;
}
// return a callee's non-zero code
#define CK(x) do { int _r = (x); if (_r) return _r; } while (0)

// bytes per element of a storage dtype code, for all four: VT_F32 4, VT_BF16 2, VT_F32X3 4 (split-bf16 arithmetic on fp32 storage), VT_F16 2
inline int vt_dt_bytes(int dt) { return (dt == VT_BF16 || dt == VT_F16) ? 2 : 4; }
inline bool vt_is16(int dt) { return dt == VT_BF16 || dt == VT_F16; }

// workspace carve: every buffer starts on a 256-byte boundary; `o` ends as the total
inline size_t vt_round256(size_t bytes) { return (bytes + 255) / 256 * 256; }
struct VtCarver {
  size_t o = 0;
  size_t take(size_t bytes) { const size_t r = o; o += vt_round256(bytes); return r; }
};

// vt_<X>_create: the argument check, then (behind the driver's own configuration checks) the count and null checks, which open a cursor
// over the weight pointers.  `fn` = the entry point's name, as the messages spell it.
inline int vt_create_args(const char* fn, const void* desc, const void* const* w, const void* out) {
  return (desc && w && out) ? VT_OK : vt_fail(VT_ERR_ARG, "%s: null argument", fn);
}
struct VtWeights {
  const void* const* w = nullptr;
  int i = 0;
  // noun: what the count message calls the entries; nullable: the table has optional slots (the U-Net's residual convolutions)
  int open(const char* fn, const void* const* w_, int n, int want, const char* noun = "weights", bool nullable = false) {
    if (n != want) return vt_fail(VT_ERR_ARG, "%s: expected %d %s, got %d", fn, want, noun, n);
    for (int k = 0; k < n && !nullable; ++k)
      if (!w_[k]) return vt_fail(VT_ERR_ARG, "%s: weight %d is null", fn, k);
    w = w_; i = 0;
    return VT_OK;
  }
  const void* next() { return w[i++]; }
  const float* next_f32() { return (const float*)w[i++]; }
};
