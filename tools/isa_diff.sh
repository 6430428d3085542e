#!/bin/bash
# Device assembly of every csrc/*.hip, this tree against a git revision (default HEAD~1): the referee of a refactor that must not change a kernel.
# Needs hipcc, no GPU.  Both sides are compiled with the Makefile's flags plus `--cuda-device-only -S`; the revision is checked out into a
# `git worktree` under a temporary directory.  Per file: `identical` (the `__hip_cuid_<hash>` symbol, which hashes the source, aside), or, for
# every kernel whose text differs, registers / scratch / LDS / code size on both sides.  A plain text diff and a metadata print, nothing else.
#   tools/isa_diff.sh [REV] [file.hip ...]          DEFS=-DVLATOUCH_DRAIN_WAITS tools/isa_diff.sh    (DEFS applies to both sides)
set -u
ROOT=$(cd "$(dirname "$0")/.." && pwd)
REV=HEAD~1
if [ $# -gt 0 ] && [[ $1 != *.hip ]]; then REV=$1; shift; fi
TMP=$(mktemp -d)
trap 'git -C "$ROOT" worktree remove --force "$TMP/old" >/dev/null 2>&1; rm -rf "$TMP"' EXIT
git -C "$ROOT" worktree add --detach "$TMP/old" "$REV" >/dev/null 2>&1 || { echo "cannot check out $REV"; exit 2; }
FILES=${*:-$(cd "$ROOT/vla-touch_amd/csrc" && ls *.hip)}
FLAGS="--offload-arch=${ARCH:-gfx950} -O3 -std=c++17 -fPIC -fno-gpu-rdc -Wall -Wno-unused-function ${DEFS:-} --cuda-device-only -S"

asm() {      # $1 = tree, $2 = output directory
  mkdir -p "$2"
  for f in $FILES; do
    [ -f "$1/vla-touch_amd/csrc/$f" ] || continue
    e=""; [ "$f" = vt_uconv.hip ] && e="-Xclang -target-feature -Xclang -packed-fp32-ops"
    echo "cd '$1/vla-touch_amd/csrc' && ${HIPCC:-/opt/rocm/bin/hipcc} $FLAGS $e $f -o '$2/${f%.hip}.s' 2>'$2/${f%.hip}.err'"
  done | xargs -P "${JOBS:-16}" -I{} bash -c {}
}
# one kernel's text per file, and "kernel .vgpr_count .sgpr_count .private_segment_fixed_size .group_segment_fixed_size code-bytes" lines from the metadata hipcc prints
split() { awk -v d="$2" '/^[A-Za-z_][A-Za-z0-9_$.]*:/ { name = $1; sub(/:.*/, "", name) } /^\t\.section|^\t\.amdgpu_metadata/ { name = "" } name != "" { print > (d "/" name ".k") }' "$1"; }
meta() {
  awk '/^[A-Za-z_][A-Za-z0-9_$.]*:/ { f = $1; sub(/:.*/, "", f) } /^; codeLenInByte = / { len[f] = $4 }
       /^    \.group_segment_fixed_size:/ { lds = $2 } /^    \.private_segment_fixed_size:/ { scr = $2 } /^    \.name:/ { n = $2 }
       /^    \.sgpr_count:/ { s = $2 } /^    \.vgpr_count:/ { v = $2 } /^    \.wavefront_size:/ { print n, v, s, scr, lds, len[n] }' "$1"
}

asm "$TMP/old" "$TMP/a"; asm "$ROOT" "$TMP/b"
status=0
for f in $FILES; do
  b=${f%.hip}
  if [ ! -s "$TMP/b/$b.s" ]; then echo "$f: DOES NOT COMPILE"; cat "$TMP/b/$b.err"; status=1; continue; fi
  if [ ! -s "$TMP/a/$b.s" ]; then echo "$f: not in $REV (or does not compile there)"; continue; fi
  if diff <(grep -v __hip_cuid_ "$TMP/a/$b.s") <(grep -v __hip_cuid_ "$TMP/b/$b.s") >/dev/null; then echo "$f: identical"; continue; fi
  echo "$f: DIFFERENT            kernel: vgpr sgpr scratch lds code-bytes, $REV -> this tree"
  status=1
  mkdir -p "$TMP/ka/$b" "$TMP/kb/$b"; split "$TMP/a/$b.s" "$TMP/ka/$b"; split "$TMP/b/$b.s" "$TMP/kb/$b"
  meta "$TMP/a/$b.s" > "$TMP/a/$b.meta"; meta "$TMP/b/$b.s" > "$TMP/b/$b.meta"
  while read -r k rest; do
    old=$(awk -v k="$k" '$1 == k { $1 = ""; print }' "$TMP/a/$b.meta")
    if [ -f "$TMP/ka/$b/$k.k" ] && diff "$TMP/ka/$b/$k.k" "$TMP/kb/$b/$k.k" >/dev/null; then continue; fi
    echo "  $(echo "$k" | c++filt 2>/dev/null || echo "$k"):${old:- (new)} -> $rest"
  done < "$TMP/b/$b.meta"
done
exit $status
