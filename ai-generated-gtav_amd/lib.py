"""ctypes binding of libgtav_amd.so, derived from the C headers that declare its ABI.

include/gtav_amd.h and include/gtav_amd_testing.h (and csrc/experiments.h for the experiments build) are the ONLY source of the binding: `parse_header`
reads every function declaration, the two config structs and the integer #defines, and SIGNATURES / _RESTYPES / EXP_SIGNATURES / DitConfig / VaeConfig /
CONSTANTS are computed from that at import.  The mapping is fixed:

    int32_t c_int32   int64_t c_int64   uint32_t c_uint32   uint64_t c_uint64   float c_float   double c_double
    const char* c_char_p          any other pointer, of any depth and pointee: c_void_p
    return: int c_int, void None, const char* c_char_p

Host out-parameters (`int64_t* bytes`, `float* out4_host`, `gtav_dit** out`, ...) are therefore c_void_p like device pointers: a header cannot say which
scalar pointers are host pointers.  c_void_p takes what the call sites pass (byref(...), a ctypes array, cast(...), None, an integer address); ctypes no
longer checks the pointee of those few pointers, and in exchange every argument of every entry point is typed by the header itself.  A declaration
the reader cannot type (another scalar type, a function pointer, `...`, an array, unbalanced parentheses) fails the import by name: it never guesses.

There is NO fallback: if the shared library is missing or a symbol is absent, import of this module
raises.  `build()` compiles it in-tree with hipcc for gfx950 (a GPU is not needed to build).
"""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libgtav_amd.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "gtav_amd.h")
TESTING_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "gtav_amd_testing.h")      # csrc/api_internal.h includes it
EXP_HEADER_PATH = os.path.join(_HERE, "csrc", "experiments.h")


class GtavError(RuntimeError):
    pass


class GtavRangeSwitch(GtavError):
    """check() under range_policy="auto": fp16 stores saturated, the layer groups in `.groups` were moved to bf16 operands; recompute."""

    def __init__(self, msg, groups=()):
        super().__init__(msg)
        self.groups = list(groups)


def build(force: bool = False) -> str:
    """Compile csrc/*.hip into libgtav_amd.so (hipcc --offload-arch=gfx950). Returns the library path."""
    src_dir = os.path.join(_HERE, "csrc")
    srcs = [os.path.join(src_dir, f) for f in os.listdir(src_dir)] + [HEADER_PATH, TESTING_HEADER_PATH]
    if not force and os.path.exists(LIB_PATH):
        if os.path.getmtime(LIB_PATH) >= max(os.path.getmtime(s) for s in srcs):
            return LIB_PATH
    subprocess.run(["bash", os.path.join(src_dir, "build.sh")], check=True)
    return LIB_PATH


_SCALARS = {"int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "float": C.c_float, "double": C.c_double}
_RETURNS = {"int": C.c_int, "void": None, "const char*": C.c_char_p}
_IDENT = r"[A-Za-z_]\w*"


def ctype_of(ctype: str, where: str = "?"):
    """The ctypes type of a parameter or field of C type `ctype` (the mapping of the module docstring); GtavError for a type outside it."""
    if ctype == "const char*":
        return C.c_char_p
    if ctype.endswith("*"):
        return C.c_void_p
    if ctype.removeprefix("const ") not in _SCALARS:
        raise GtavError(f"{where}: no ctypes mapping for the C type `{ctype}`")
    return _SCALARS[ctype.removeprefix("const ")]


def _declarator(text, where):
    """`const float* const* ws` -> ("const float* const*", "ws"); the name may be absent (""); anything but words and `*` is refused."""
    toks = re.findall(r"\w+|\S", text)
    if not toks or any(t != "*" and not re.fullmatch(_IDENT, t) for t in toks):
        raise GtavError(f"{where}: cannot type `{' '.join(text.split())}`")
    named = len(toks) > 1 and toks[-1] != "*" and toks[-1] not in _SCALARS and toks[-1] not in ("const", "void", "char", "int")
    name = toks.pop() if named else ""
    ctype = ""
    for t in toks:
        ctype += t if t == "*" or not ctype else " " + t
    return ctype, name


def parse_header(text: str):
    """The declarations of one plain-C header -> (functions, structs, constants):
    functions  [(name, return type, [(C type, parameter name), ...]), ...] in header order
    structs    {NAME: [(C type, field), ...]} of every `typedef struct NAME { ... } NAME;` (forward declarations are skipped)
    constants  {NAME: int} of every `#define NAME <integer literal>` (a #define without a value, such as an include guard, is skipped)
    Raises GtavError, naming the declaration, for whatever ctype_of / _declarator cannot type and for anything that is none of the above."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    constants = {}
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(\S.*?)[ \t]*$", text, flags=re.M):
        try:
            constants[name] = int(value, 0)
        except ValueError:
            raise GtavError(f"#define {name}: `{value}` is not an integer literal") from None
    text = re.sub(r'extern\s+"C"\s*\{', " ", re.sub(r"^[ \t]*#.*$", "", text, flags=re.M))
    structs = {}

    def struct(m):
        fields = structs.setdefault(m.group(3), [])
        for decl in filter(str.strip, m.group(2).split(";")):               # `int32_t a, b, c` is three fields
            first, *more = decl.split(",")
            ctype, name = _declarator(first, m.group(3))
            ctype_of(ctype, f"{m.group(3)}.{name}")
            for field in [name] + [f.strip() for f in more]:
                if not re.fullmatch(_IDENT, field):
                    raise GtavError(f"{m.group(3)}: cannot type the field `{' '.join(decl.split())}`")
                fields.append((ctype, field))
        return " "
    text = re.sub(rf"typedef\s+struct\s+({_IDENT})\s*\{{([^{{}}]*)\}}\s*({_IDENT})\s*;", struct, text)
    functions = []
    for stmt in text.replace("}", " ").split(";"):                           # (the brace that closes extern "C")
        stmt = " ".join(stmt.split())
        if not stmt or re.fullmatch(rf"typedef struct {_IDENT} {_IDENT}|struct {_IDENT}", stmt):
            continue
        m = re.fullmatch(rf"([^()]+?)\b({_IDENT}) ?\(([^()]*)\)", stmt)
        if not m:                                                            # function pointers, unbalanced parentheses, anything that is no prototype
            named = re.search(rf"({_IDENT}) ?\(", stmt)
            raise GtavError(f"{named.group(1) if named else stmt[:60]}: cannot parse the declaration `{stmt[:120]}`")
        name, (ret, _) = m.group(2), _declarator(m.group(1), m.group(2))
        if ret not in _RETURNS:
            raise GtavError(f"{name}: no ctypes mapping for the return type `{ret}`")
        params = [] if m.group(3).strip() in ("", "void") else [_declarator(p, name) for p in m.group(3).split(",")]
        for ctype, pname in params:
            ctype_of(ctype, f"{name}({pname})")
        functions.append((name, ret, params))
    return functions, structs, constants


DECLARATIONS = {}      # name -> (return type, [(C type, parameter name), ...]) of every entry point of the three headers, as the headers spell them
STRUCTS = {}           # gtav_dit_config, gtav_vae_config -> [(C type, field), ...]
CONSTANTS = {}         # the integer #defines: GTAV_PROFILE_CLASSES, GTAV_OPERAND_F16 / _BF16, GTAV_GEMM_WM_NT_WEIGHT_FILLS


def _signatures(*paths):
    """Reads the headers into DECLARATIONS / STRUCTS / CONSTANTS and returns their functions' name -> argtypes."""
    table = {}
    for path in paths:
        with open(path) as f:
            functions, structs, constants = parse_header(f.read())
        STRUCTS.update(structs)
        CONSTANTS.update(constants)
        for name, ret, params in functions:
            DECLARATIONS[name] = (ret, params)
            table[name] = [ctype_of(ctype) for ctype, _ in params]
    return table


SIGNATURES = _signatures(HEADER_PATH, TESTING_HEADER_PATH)        # name -> argtypes
EXP_SIGNATURES = _signatures(EXP_HEADER_PATH)                     # entry points of the experiments build only: the LayerNorm fold, set_debug, set_stamps
_RESTYPES = {name: _RETURNS[ret] for name, (ret, _) in DECLARATIONS.items()}
DitConfig = type("DitConfig", (C.Structure,), {"_fields_": [(f, ctype_of(t)) for t, f in STRUCTS["gtav_dit_config"]]})
VaeConfig = type("VaeConfig", (C.Structure,), {"_fields_": [(f, ctype_of(t)) for t, f in STRUCTS["gtav_vae_config"]]})

_lib = None


def _bind(lib, table):
    for name, argtypes in table.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.argtypes, fn.restype = argtypes, _RESTYPES[name]


def load() -> C.CDLL:
    """Loads the shared library (once) and binds every symbol of SIGNATURES; raises if anything is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise GtavError(f"{LIB_PATH} not found: run `python -c 'import __graft_entry__ as g; g.build()'` "
                        f"(hipcc --offload-arch=gfx950). gtav_amd has no CPU fallback.")
    # torch's wheel bundles its own libamdhip64: it must be in the process BEFORE this library's dependency on libamdhip64 is resolved, or the process ends
    # up with two HIP runtimes — torch's sees the GPU, the one this library was bound to reports "no ROCm-capable device" (seen as build(); smoke() in one process)
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    _bind(lib, SIGNATURES)
    _lib = lib
    return lib


EXP_LIB_PATH = os.environ.get("GTAV_EXP_LIB") or os.path.join(_HERE, "libgtav_amd_exp.so")    # the override: A/B of two experiment builds (tools/ only)


def load_experiments(build_if_missing: bool = True) -> C.CDLL:
    """tools/ only: the -DGTAV_EXPERIMENTS build (csrc/build.sh exp), which adds gtav_op_gemm_set_debug (timing runs with
    skipped fills / MFMAs: WRONG results) and reads the GTAV_* environment knobs.  It becomes the library every gtav_amd
    class of this process uses, so one process never mixes the two builds.  Never imported by the product or the tests."""
    global _lib
    if _lib is not None and getattr(_lib, "_gtav_experiments", False):
        return _lib
    if _lib is not None:
        raise GtavError("load_experiments() must be called before anything loaded the product library")
    if build_if_missing and not os.path.exists(EXP_LIB_PATH):
        subprocess.run(["bash", os.path.join(_HERE, "csrc", "build.sh"), "exp"], check=True)
    import torch  # noqa: F401   (torch's HIP runtime first: see load())
    lib = C.CDLL(EXP_LIB_PATH)
    _bind(lib, SIGNATURES)
    _bind(lib, EXP_SIGNATURES)     # csrc/experiments.h
    lib._gtav_experiments = True
    _lib = lib
    return lib


def check(rc: int) -> None:
    if rc != 0:
        raise GtavError(load().gtav_last_error().decode() or f"gtav_amd call failed with code {rc}")


def ptr(t) -> int:
    """Device/host address of a torch tensor (0 for None)."""
    return 0 if t is None else t.data_ptr()


def current_stream() -> int:
    import torch
    return torch.cuda.current_stream().cuda_stream
