"""The ctypes binding of vlatouch/_lib.py against C, stated once (tests/test_abi_host.py asserts it; no pytest here, so a tool can import it):
  * `declared_functions()`: every function include/vlatouch.h declares, as the (restype, argtypes) ctypes has to carry;
  * `STRUCTS`: each `ctypes.Structure` of `_lib` and the C type it mirrors;
  * `CONSTANTS`: each integer code the Python side restates and the C name that defines it;
  * `c_facts(tmpdir)`: sizeof / offsetof / values of all of these as the C++ compiler sees them, from one host-only probe.
A disagreement between the mirror and C raises no error at run time: the library reads the wrong bytes."""
import ctypes as C
import os
import re
import shutil
import subprocess

from tests import cases
from vlatouch import _lib, ctrl_data, imgaug, imgprep, rdt_data, train

HEADER = os.path.join(cases.ROOT, "include", "vlatouch.h")
CSRC = os.path.join(cases.PKG, "csrc")
UNBOUND = ("vt_last_error", "vt_version")      # declared, but set by hand in _lib.lib() instead of through SIGNATURES

_SCALARS = {"void": None, "int": C.c_int, "long": C.c_long, "long long": C.c_longlong, "unsigned": C.c_uint, "unsigned long long": C.c_ulonglong,
            "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t}
_HANDLES = ("vt_stream_t", "vt_unet_t", "vt_dino_t", "vt_lstm_t", "vt_rdt_t", "vt_t5_t")


def _ctype(decl: str, named: bool):
    """One parameter (`named`) or return type -> ctypes.  A pointer of any kind is c_void_p; everything else must be a known scalar or handle."""
    if "*" in decl:
        return C.c_void_p
    words = [w for w in decl.split() if w != "const"]
    if named:
        if len(words) < 2:
            raise ValueError(f"parameter without a name or a type: {decl!r}")
        words = words[:-1]
    t = " ".join(words)
    if t in _HANDLES:
        return C.c_void_p
    if t not in _SCALARS:
        raise ValueError(f"unknown C type {t!r} in {decl!r}")
    return _SCALARS[t]


def declared_functions(header: str = HEADER):
    """{name: (restype, argtypes)} of every function the header declares; raises on anything it cannot read as one."""
    src = re.sub(r"/\*.*?\*/", " ", open(header).read(), flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    src = re.sub(r"^[ \t]*#[^\n]*$", " ", src, flags=re.M)                                  # include guards, #define, #ifdef
    src = re.sub(r'extern\s+"C"\s*\{', " ", src)
    src = re.sub(r"typedef\s+struct\s*\{[^}]*\}\s*\w+\s*;", " ", src)                       # the parameter records (STRUCTS checks them)
    src = re.sub(r"enum\s*\{[^}]*\}\s*;", " ", src)
    src = re.sub(r"typedef\s+[^;{}]*;", " ", src)                                           # vt_stream_t and the handles
    out = {}
    for stmt in src.split(";"):
        stmt = " ".join(stmt.split())
        if stmt in ("", "}"):                                                               # "}" closes extern "C"
            continue
        m = re.fullmatch(r"(.+?)\b(\w+) ?\((.*)\)", stmt)
        if not m or "(" in m.group(3):
            raise ValueError(f"not a function declaration: {stmt!r}")
        ret, name, params = m.group(1), m.group(2), m.group(3).strip()
        if name in out:
            raise ValueError(f"{name} is declared twice")
        out[name] = (_ctype(ret, named=False), [] if params == "void" else [_ctype(p, named=True) for p in params.split(",")])
    return out


STRUCTS = [
    (_lib.GemmParams, "VtGemmParams"), (_lib.GnParams, "VtGnParams"), (_lib.AttnParams, "VtAttnParams"), (_lib.AttnKvtParams, "VtAttnKvtParams"),
    (_lib.AttnBwdParams, "VtAttnBwdParams"), (_lib.GemmTnPlan, "VtGemmTnPlan"), (_lib.UnetDesc, "vt_unet_desc"), (_lib.DinoDesc, "vt_dino_desc"),
    (_lib.T5Desc, "vt_t5_desc"), (_lib.LstmDesc, "vt_lstm_desc"), (_lib.RdtDesc, "vt_rdt_desc"), (_lib.ImgprepFrame, "vt_imgprep_frame"),
    (_lib.ColorJitterFrame, "vt_colorjitter_frame"), (_lib.AreaFrame, "vt_area_frame"), (_lib.JpegmapFrame, "vt_jpegmap_frame"),
    (_lib.CorruptFrame, "vt_corrupt_frame"),
]

MT_ENTRY = ("p", "g", "m", "v", "shadow", "n", "first_chunk")      # MtEntry of csrc/vt_optim.h; train.mt_table writes one int64 per field


def _named(mod, prefix: str, names: str, strip: str = ""):
    """Rows for module constants whose C name is `prefix` + the Python name without its own prefix `strip`."""
    return [(f"{mod.__name__}.{n}", getattr(mod, n), prefix + n[len(strip):]) for n in names.split()]


def _keyed(mod, table: str, prefix: str):
    return [(f"{mod.__name__}.{table}[{k!r}]", v, prefix + k.upper()) for k, v in getattr(mod, table).items()]


# (what Python calls it, Python's value, the C name that defines it): dtype / activation codes in csrc/vt_common.h, the norm codes in
# csrc/vt_kernels.h, MT_CHUNK in csrc/vt_optim.h, the rest in include/vlatouch.h
CONSTANTS = (
    _named(_lib, "VT_", "F32 BF16 F32X3 F16") +
    _named(_lib, "VT_", "ACT_NONE ACT_GELU_ERF ACT_GELU_TANH ACT_SILU ACT_MISH ACT_SWIGLU ACT_GEGLU") +
    _named(_lib, "VT_", "NORM_LAYER NORM_RMS_MEANSQ NORM_RMS_VAR IMGNORM_AUTO IMGNORM_ON IMGNORM_OFF IMGNORM_RAW") +
    _named(_lib, "VT_", "RANGE_XN_SAT RANGE_NONFINITE RANGE_GATE_SAT RANGE_ATTN_EMPTY") +
    [(f"vlatouch._lib.ROUTE_NAMES[{i}]", i, "VT_ROUTE_" + n) for i, n in enumerate(_lib.ROUTE_NAMES)] +
    _named(_lib, "VT_", "IMGPREP_PAD IMGPREP_BRIGHT IMGPREP_OUT_BF16 IMGPREP_OUT_U8 IMGPREP_TWO_PASS COLORJITTER_LIFT JPEGMAP_CV2_ORDER") +
    _named(rdt_data, "VT_RDT_", "MASK_FREQ MASK_STATE MASK_ELEM NOISE") +
    _named(imgaug, "VT_COLORJITTER_", "OP_BRIGHTNESS OP_CONTRAST OP_SATURATION OP_HUE OP_NONE", strip="OP_") +
    _keyed(imgaug, "NOISE_KINDS", "VT_CORRUPT_NOISE_") + _keyed(imgaug, "BLUR_KINDS", "VT_CORRUPT_BLUR_") +
    _named(imgaug, "VT_CORRUPT_", "THRESHOLDS MAX_RADIUS") +
    _keyed(ctrl_data, "LAYOUTS", "VT_CTRL_") +
    _named(imgprep, "VT_", "AREA_MAX_ISCALE") +
    _named(train, "", "MT_CHUNK")
)


def field_names(cls):
    return [f[0] for f in cls._fields_]


def hipcc():
    """The compiler the library was built with, or None if there is none at all."""
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):       # __graft_entry__.build()'s choice first
        if c and shutil.which(c):
            return shutil.which(c)
    return None


class ProbeError(RuntimeError):
    """The probe did not build or run: the binding or the headers are broken (the message is the compiler's)."""


def c_facts(tmpdir):
    """Compile and run one host-only C++ probe generated from STRUCTS (with each class's `_fields_`), MT_ENTRY and CONSTANTS ->
    {"sizeof": {ctype: bytes}, "fields": {(ctype, field): (offset, bytes)}, "constants": {cname: value}}."""
    lines = ["#include <cstdio>", "#include <cstddef>", '#include "vt_common.h"', '#include "vt_kernels.h"', '#include "vt_gemm.h"',
             '#include "vt_optim.h"', '#include "vlatouch.h"', "int main() {"]
    for ctype, fields in [(ct, field_names(cls)) for cls, ct in STRUCTS] + [("MtEntry", MT_ENTRY)]:
        lines.append(f'  printf("sizeof {ctype} %zu\\n", sizeof({ctype}));')
        for f in fields:
            lines.append(f'  printf("field {ctype} {f} %zu %zu\\n", offsetof({ctype}, {f}), sizeof((({ctype}*)0)->{f}));')
    for cname in dict.fromkeys(row[2] for row in CONSTANTS):
        lines.append(f'  printf("const {cname} %lld\\n", (long long)({cname}));')
    lines += ["  return 0;", "}", ""]
    src, exe = os.path.join(str(tmpdir), "abi_probe.cpp"), os.path.join(str(tmpdir), "abi_probe")
    with open(src, "w") as f:
        f.write("\n".join(lines))
    if hipcc() is None:
        raise FileNotFoundError("no hipcc on this machine")
    cmd = [hipcc(), "-x", "hip", "--cuda-host-only", "-std=c++17", "-I", CSRC, "-I", os.path.dirname(HEADER), src, "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise ProbeError("the ABI probe does not compile against csrc/ and include/vlatouch.h:\n" + r.stderr[-4000:])
    r = subprocess.run([exe], capture_output=True, text=True)
    if r.returncode != 0:
        raise ProbeError(f"the ABI probe exited with {r.returncode}: {r.stderr[-1000:]}")
    facts = {"sizeof": {}, "fields": {}, "constants": {}}
    for kind, *rest in (ln.split() for ln in r.stdout.splitlines()):
        if kind == "sizeof":
            facts["sizeof"][rest[0]] = int(rest[1])
        elif kind == "field":
            facts["fields"][rest[0], rest[1]] = (int(rest[2]), int(rest[3]))
        else:
            facts["constants"][rest[0]] = int(rest[1])
    return facts
