// vt_frames.h — the host checks the drivers of frame tables share (vt_imgprep.hip, vt_colorjitter.hip, vt_jpegmap.hip), stated once.  A record
// is a uint8 HWC frame {src, pitch, h, w, out_off, ...}; `fn` = the entry point's name, as the messages spell it.  Each returns VT_OK or
// VT_ERR_ARG with the message set.
#pragma once
#include "vt_host.h"

// frames of one output, and scratch rows of one workspace, start 16 bytes apart at least
inline size_t vt_round16(size_t bytes) { return (bytes + 15) / 16 * 16; }

template <typename F> int vt_frame_pitch_check(const char* fn, const F& f, int i) {
  return f.pitch < 3L * f.w ? vt_fail(VT_ERR_ARG, "%s: frame %d: row pitch %ld < 3 * width %d", fn, i, f.pitch, f.w) : VT_OK;
}
// a frame that must exist, written at out_off
template <typename F> int vt_frame_check(const char* fn, const F& f, int i) {
  if (!f.src) return vt_fail(VT_ERR_ARG, "%s: frame %d has a null source", fn, i);
  if (f.h < 1 || f.w < 1) return vt_fail(VT_ERR_ARG, "%s: frame %d has a zero size (%d x %d)", fn, i, f.h, f.w);
  CK(vt_frame_pitch_check(fn, f, i));
  return f.out_off < 0 ? vt_fail(VT_ERR_ARG, "%s: frame %d: negative out_off", fn, i) : VT_OK;
}

inline int vt_frames_table_check(const char* fn, const void* frames_host, int n) {
  return (frames_host && n >= 1) ? VT_OK : vt_fail(VT_ERR_ARG, "%s: null frame table or n < 1", fn);
}
// the head of a call whose grid has one row of blocks per frame: the table, the count, the flag bits
inline int vt_frames_call_check(const char* fn, const void* frames_host, int n, int flags, int known_flags) {
  CK(vt_frames_table_check(fn, frames_host, n));
  if (n > 65535) return vt_fail(VT_ERR_ARG, "%s: %d frames, at most 65535 in one call", fn, n);
  return (flags & ~known_flags) ? vt_fail(VT_ERR_ARG, "%s: unknown flag bits %#x", fn, flags) : VT_OK;
}
// the device side of a call; ws_align8: the kernels keep uint64 sums or 8-byte stores at offsets of the workspace
inline int vt_frames_buffers_check(const char* fn, const void* frames_dev, const void* out, const void* ws, size_t ws_bytes, size_t need, bool ws_align8) {
  if (!frames_dev || !out || !ws) return vt_fail(VT_ERR_ARG, "%s: null device frame table, output or workspace", fn);
  if (ws_bytes < need) return vt_fail(VT_ERR_ARG, "%s: workspace of %zu bytes, %zu needed", fn, ws_bytes, need);
  return (ws_align8 && ((uintptr_t)ws & 7)) ? vt_fail(VT_ERR_ARG, "%s: the workspace must be 8-byte aligned", fn) : VT_OK;
}
// the closing of a driver: whether every launch above was accepted
inline int vt_frames_launched(const char* fn) { return vt_check_launch() ? vt_fail(VT_ERR_LAUNCH, "%s: launch failure", fn) : VT_OK; }
