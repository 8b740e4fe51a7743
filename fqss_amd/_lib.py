"""ctypes binding of csrc/libfqss_hip.so.  The C ABI is written down once, in include/fqss.h: the argtypes, restypes, descriptor
structs and integer constants below are read from that header at import."""
import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.environ.get("FQSS_LIB") or os.path.join(_HERE, "csrc", "libfqss_hip.so")   # FQSS_LIB: kernel A/B experiments
HEADER_PATH = os.path.normpath(os.path.join(_HERE, "..", "include", "fqss.h"))            # as csrc/Makefile finds it


class FqssError(RuntimeError):
    pass


_BY_VALUE = {"int": C.c_int, "int32_t": C.c_int, "int64_t": C.c_int64, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t}
_RETURNS = {"int": C.c_int, "int64_t": C.c_int64, "const char*": C.c_char_p}
_HANDLE = "fqss_stream_t"
_DIRECTIVE = re.compile(r"#\s*(?:include\b.*|ifndef\s+\w+_H|ifdef\s+__cplusplus|endif|define\s+(\w+)\s*(.*))$")
_STRUCT = re.compile(r"typedef\s+struct(?:\s+\w+)?\s*\{([^{}]*)\}\s*(\w+)\s*;")
_FIELD = re.compile(r"(?:const\s+)?(\w+)\s*((?:\*\s*)?\w+(?:\s*\[\d+\])?(?:\s*,\s*(?:\*\s*)?\w+(?:\s*\[\d+\])?)*)")
_PROTO = re.compile(r"(int|int64_t|const char\s*\*)\s*(\w+)\s*\(([^()]*)\)")
_POINTER_PARAM = re.compile(r"(?:const\s+)?\w+(?:\s*\*(?:\s*const)?)+\s*\w+")
_STRING_PARAM = re.compile(r"const char\s*\*\s*\w+")
_VALUE_PARAM = re.compile(r"(\w+)\s+\w+")


def parse_header(text):
    """The C ABI of a header in the grammar include/fqss.h uses -> (protos {name: argtypes}, restypes {name: restype},
    structs {name: ctypes.Structure subclass}, constants {name: int}).  Anything outside that grammar raises FqssError naming the
    declaration: nothing is guessed and nothing is skipped."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    constants, code = {}, []
    for line in text.splitlines():
        if not line.lstrip().startswith("#"):
            code.append(line)
            continue
        m = _DIRECTIVE.fullmatch(line.strip())
        if m is None:
            raise FqssError(f"fqss.h reader: unsupported preprocessor line {line.strip()!r}")
        name, value = m.groups()
        if name is not None and value:            # a #define without a value is the include guard
            v = re.fullmatch(r"(\d+)|\((-\d+)\)", value.strip())
            if v is None:
                raise FqssError(f"fqss.h reader: #define {name} is not an integer constant: {value.strip()!r}")
            constants[name] = int(v.group(1) or v.group(2))
    text = "\n".join(code)

    structs = {}

    def struct(m):
        body, name = m.groups()
        fields = []
        for decl in filter(None, (" ".join(d.split()) for d in body.split(";"))):
            f = _FIELD.fullmatch(decl)
            if f is None:
                raise FqssError(f"fqss.h reader: cannot classify field {decl!r} of struct {name}")
            base = f.group(1)
            for d in f.group(2).split(","):
                field, _, count = d.replace("*", " ").replace("]", "").partition("[")
                if "*" in d:
                    ctype = C.POINTER(structs[base]) if base in structs else C.c_void_p
                elif base in _BY_VALUE:
                    ctype = _BY_VALUE[base]
                else:
                    raise FqssError(f"fqss.h reader: field {decl!r} of struct {name} has the unsupported by-value type {base}")
                fields.append((field.strip(), ctype * int(count) if count else ctype))
        structs[name] = type(name, (C.Structure,), {"_fields_": fields})
        return ""

    text = _STRUCT.sub(struct, text)
    block = re.fullmatch(r'\s*extern\s+"C"\s*\{(.*)\}\s*', text, flags=re.S)
    protos, restypes = {}, {}
    for decl in filter(None, (" ".join(d.split()) for d in (block.group(1) if block else text).split(";"))):
        if re.fullmatch(r"typedef void\s*\* " + _HANDLE, decl):
            continue                              # the stream handle: c_void_p wherever a parameter names it
        m = _PROTO.fullmatch(decl)
        if m is None:
            raise FqssError(f"fqss.h reader: cannot classify declaration {decl[:120]!r}")
        ret, name, params = m.groups()
        args = []
        for p in ([] if params.strip() == "void" else (q.strip() for q in params.split(","))):
            ptr, val = _POINTER_PARAM.fullmatch(p), _VALUE_PARAM.fullmatch(p)
            if ptr:
                args.append(C.c_char_p if _STRING_PARAM.fullmatch(p) else C.c_void_p)
            elif val and val.group(1) == _HANDLE:
                args.append(C.c_void_p)
            elif val and val.group(1) in _BY_VALUE:
                args.append(_BY_VALUE[val.group(1)])
            else:
                raise FqssError(f"fqss.h reader: cannot classify parameter {p!r} of {name}")
        protos[name], restypes[name] = args, _RETURNS["const char*" if "*" in ret else ret]
    return protos, restypes, structs, constants


def _read_header():
    try:
        with open(HEADER_PATH) as f:
            return parse_header(f.read())
    except OSError as e:
        raise FqssError(f"{HEADER_PATH} not found: the binding is read from it ({e})") from None


# name -> argtypes / name -> restype / struct classes under their header names / every integer #define
_PROTOS, _RESTYPE, STRUCTS, CONSTANTS = _read_header()
globals().update(STRUCTS)
globals().update({k[len("FQSS_"):]: v for k, v in CONSTANTS.items() if k.startswith("FQSS_DT_")})   # DT_F32 .. DT_I64
EXPORTS = tuple(_PROTOS)


_lib = None
BACKEND = "hip"           # "hip": csrc/libfqss_hip.so on MI355X (the product) | "cpu": csrc/cpu/libfqss_cpu.so (cfg 1: `--use_cpu`)
CPU_SO_PATH = os.path.join(_HERE, "csrc", "cpu", "libfqss_cpu.so")
_cpu = None


def set_backend(name):
    """`--use_cpu` (reference train.py:31) selects the CPU backend behind the same C ABI: a build-owned plain-C++ library that serves the
    entry points of the un-fused ConvTasNet QAT step (BASELINE.json configs[0]).  It is chosen EXPLICITLY, never as a fallback: with the
    HIP backend selected a CPU tensor or a missing .so still raises."""
    global BACKEND
    if name not in ("hip", "cpu"):
        raise FqssError(f"unknown backend {name!r}")
    if name == "cpu":
        load_cpu()
    BACKEND = name
    _bound.clear()
    from . import ops
    ops.CODED = name != "cpu"        # the CPU backend has the fp32 per-layer kernels only: no layer output carries codes there


def load_cpu():
    global _cpu
    if _cpu is None:
        if not os.path.exists(CPU_SO_PATH):
            raise FqssError(f"{CPU_SO_PATH} not found: build it with `make -C fqss_amd/csrc/cpu` (or __graft_entry__.build())")
        _cpu = C.CDLL(CPU_SO_PATH)
        _cpu.fqss_last_error.restype = C.c_char_p
    return _cpu


def load(strict=False):
    """Load the HIP library; fail LOUDLY when it is missing (no CPU fallback exists).
    strict=True additionally requires every symbol declared in include/fqss.h to be exported."""
    global _lib
    if BACKEND == "cpu" and not strict:
        return load_cpu()
    if _lib is None:
        if not os.path.exists(SO_PATH):
            raise FqssError(
                f"{SO_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(or `make -C fqss_amd/csrc`). fqss_amd has no CPU fallback.")
        _lib = C.CDLL(SO_PATH)
        _lib.fqss_last_error.restype = C.c_char_p
    if strict:
        missing = [n for n in EXPORTS if not hasattr(_lib, n)]
        if missing:
            raise FqssError(f"{SO_PATH} does not export: {missing}")
    return _lib


_bound = {}


def _bind(name):
    fn = _bound.get(name)
    if fn is None:
        lib = load()
        if not hasattr(lib, name):
            raise FqssError(f"{name} is not built for the {BACKEND} backend" + (
                " (the CPU backend serves the un-fused ConvTasNet QAT step only: cfg 1 of BASELINE.json)" if BACKEND == "cpu" else ""))
        fn = getattr(lib, name)
        fn.argtypes = _PROTOS[name]
        fn.restype = _RESTYPE[name]
        _bound[name] = fn
    return fn


def call(name, *args):
    rc = _bind(name)(*args)
    if rc != 0:
        raise FqssError(f"{name} failed ({rc}): {load().fqss_last_error().decode()}")


def query(name, *args):
    """entry points that return a count instead of a status (fqss_*_stat_slots, fqss_workspace_bytes)"""
    return _bind(name)(*args)
