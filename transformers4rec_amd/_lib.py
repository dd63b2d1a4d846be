"""ctypes binding of libt4r_hip.so.  The C ABI is declared in the headers under include/ (HEADERS); the ctypes prototypes are
derived from those declarations (signatures()), so a new header is registered by adding its file name to HEADERS.
EXTENSION_HEADERS are headers of the same library that are bound after the main ones (extension_signatures()): their names
are not part of signatures() / header_symbols() / HEADERS, and may not repeat one of those.  FEATURE_HEADERS are bound after
both (feature_signatures()), under the same rule: a later feature's header is added to that tuple (its order is not an
interface: t4r_hip_gru.h stands between the two earlier ones) and changes neither of the other two.

There is NO fallback: if the shared library is missing or a call fails the product path
raises.  Build with `python -m transformers4rec_amd.build` (or __graft_entry__.build()).
"""
import ctypes
import functools
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
# T4R_HIP_LIB selects another build of the same ABI (A/B timing of kernel variants on one box)
LIB_PATH = os.environ.get("T4R_HIP_LIB") or os.path.join(_HERE, "lib", "libt4r_hip.so")
HEADERS = ("t4r_hip.h", "t4r_hip_sampling.h", "t4r_hip_filter.h", "t4r_hip_optim.h", "t4r_hip_pretrained.h", "t4r_hip_attn.h",
           "t4r_hip_rows.h", "t4r_hip_rowadam.h", "t4r_hip_contproj.h", "t4r_hip_rowclip.h", "t4r_hip_seqtask.h", "t4r_hip_rtd.h")
EXTENSION_HEADERS = ("t4r_hip_uni.h",)
FEATURE_HEADERS = ("t4r_hip_postfusion.h", "t4r_hip_gru.h", "t4r_hip_mlpblock.h")


def header_path(name):
    """Path of include/<name>."""
    return os.path.join(os.path.dirname(_HERE), "include", name)


HEADER_PATH = header_path(HEADERS[0])

# code -> ctypes type; a parameter with a `*` is "p", and these are the only C types the ABI passes and returns by value: the
# prototypes are derived from the headers with these two tables and nothing is guessed
_C = {"p": ctypes.c_void_p, "i": ctypes.c_int, "l": ctypes.c_long, "f": ctypes.c_float, "Q": ctypes.c_ulonglong,
      "s": ctypes.c_char_p, "v": None}
_ARG = {"unsigned long long": "Q", "long": "l", "int": "i", "float": "f"}
_RET = {"unsigned long long": "Q", "long": "l", "int": "i", "void": "v", "const char*": "s"}

_lib = None


class T4RHipError(RuntimeError):
    pass


def parse_header(text, header="<text>"):
    """name -> (restype code, argtype codes) of every function declared in the text of a C header, in the order declared.
    Codes: p pointer, i int, l long, f float, Q unsigned long long; returns also v void, s const char*.  A declaration that
    uses anything else (double, size_t, a struct by value, a function pointer, varargs) raises T4RHipError."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)                     # comments, also inside a parameter list
    text = re.sub(r"^[ \t]*#(?:[^\n]*\\\n)*[^\n]*", "", text, flags=re.M)          # preprocessor lines with their continuations
    text = re.sub(r"\btypedef\s+struct\b[^{;]*(?:\{[^}]*\})?[^;]*;", "", text)
    text, n_extern = re.subn(r'\bextern\s+"C"\s*\{', "", text)
    *decls, rest = (" ".join(d.split()) for d in text.split(";"))                   # what is left is `declaration;` ... `}`
    if rest != "}" * n_extern:
        raise T4RHipError(f"{header}: cannot parse the text after the last declaration: {rest!r}")
    sigs = {}
    for decl in filter(None, decls):
        m = re.fullmatch(r"(.*?)\b(\w+) ?\(([^()]*)\)", decl)
        ret = _RET.get(re.sub(r" ?\* ?", "*", m.group(1)).strip()) if m else None
        if ret is None:
            raise T4RHipError(f"{header}: cannot derive a ctypes prototype for `{decl}`")
        name, params = m.group(2), m.group(3).strip()
        codes = ""
        for param in ([] if params == "void" else params.split(",")):
            words = [w for w in param.split() if w != "const"]
            if "*" not in param and len(words) > 1 and words[-1] not in ("unsigned", "long", "int"):
                words.pop()                                            # the parameter's name
            code = "p" if "*" in param else _ARG.get(" ".join(words))
            if code is None or "..." in param or "[" in param:
                raise T4RHipError(f"{header}: cannot derive a ctypes code for parameter `{param.strip()}` of `{decl}`")
            codes += code
        if name in sigs:
            raise T4RHipError(f"{header}: `{name}` is declared twice")
        sigs[name] = (ret, codes)
    return sigs


@functools.lru_cache(maxsize=None)
def _header_signatures(header):
    path = header_path(header)
    try:
        with open(path) as f:
            text = f.read()
    except OSError as e:
        raise T4RHipError(f"{path} is missing ({e.strerror}): the ctypes prototypes are derived from the C headers "
                          "under include/") from e
    return parse_header(text, header)


@functools.lru_cache(maxsize=None)
def signatures():
    """name -> (restype code, argtype codes) of the whole C ABI: the union over HEADERS."""
    sigs, where = {}, {}
    for header in HEADERS:
        for name, sig in _header_signatures(header).items():
            if name in sigs:
                raise T4RHipError(f"`{name}` is declared in both {where[name]} and {header}")
            sigs[name], where[name] = sig, header
    return sigs


@functools.lru_cache(maxsize=None)
def extension_signatures():
    """name -> (restype code, argtype codes) of the entries declared in EXTENSION_HEADERS (same parser); a name that
    signatures() or another extension header already has is an error."""
    main = signatures()
    sigs, where = {}, {}
    for header in EXTENSION_HEADERS:
        for name, sig in _header_signatures(header).items():
            if name in main:
                raise T4RHipError(f"`{name}` of the extension header {header} is already declared in the main headers")
            if name in sigs:
                raise T4RHipError(f"`{name}` is declared in both {where[name]} and {header}")
            sigs[name], where[name] = sig, header
    return sigs


@functools.lru_cache(maxsize=None)
def feature_signatures():
    """name -> (restype code, argtype codes) of the entries declared in FEATURE_HEADERS (same parser); a name that
    signatures(), extension_signatures() or another feature header already has is an error."""
    taken = {name: "the main headers" for name in signatures()}
    taken.update({name: "the extension headers" for name in extension_signatures()})
    sigs, where = {}, {}
    for header in FEATURE_HEADERS:
        for name, sig in _header_signatures(header).items():
            if name in taken:
                raise T4RHipError(f"`{name}` of the feature header {header} is already declared in {taken[name]}")
            if name in sigs:
                raise T4RHipError(f"`{name}` is declared in both {where[name]} and {header}")
            sigs[name], where[name] = sig, header
    return sigs


def header_symbols(header=HEADERS[0]):
    """Sorted function names declared in include/<header>."""
    return sorted(_header_signatures(header))


def load():
    """Loads the library and sets ctypes prototypes.  Raises if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise T4RHipError(
            f"{LIB_PATH} not found: the HIP extension is not built "
            "(run `python -m transformers4rec_amd.build`). There is no CPU fallback.")
    sigs = dict(signatures())
    sigs.update(extension_signatures())                # bound after the main ones
    sigs.update(feature_signatures())                  # and these after both
    lib = ctypes.CDLL(LIB_PATH)
    for name, (ret, args) in sigs.items():
        fn = getattr(lib, name)
        fn.restype = _C[ret]
        fn.argtypes = [_C[a] for a in args]
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        msg = load().t4r_last_error()
        raise T4RHipError(f"{what} failed (rc={rc}): {msg.decode() if msg else ''}")


def call(name, *args):
    rc = getattr(load(), name)(*args)
    if rc != 0:
        check(rc, name)


def ptr_array(ptrs):
    """host array of device pointers (const T* const*)"""
    arr = (ctypes.c_void_p * len(ptrs))(*ptrs)
    return ctypes.cast(arr, ctypes.c_void_p), arr


def int_array(vals):
    arr = (ctypes.c_int * len(vals))(*vals)
    return ctypes.cast(arr, ctypes.c_void_p), arr


def long_array(vals):
    arr = (ctypes.c_long * len(vals))(*vals)
    return ctypes.cast(arr, ctypes.c_void_p), arr


def exp_env(name, default=None):
    """value of an EXPERIMENT switch: the environment variable `name` when the loaded library is an experiment build
    (-DT4R_EXPERIMENTAL, tools/experimental/build_variant.sh), else `default`.  The product build ignores these names on both
    sides of the C ABI (csrc/t4r_common.h: t4r_exp_getenv), so that the host never plans for a kernel family the library
    will not run.  The switches the product DOES read are listed in INTEGRATION.md section 5."""
    v = os.environ.get(name)
    if v is None:
        return default
    try:
        return v if load().t4r_experimental_build() else default
    except Exception:       # noqa: BLE001  (library not built yet: CPU-only import)
        return default
