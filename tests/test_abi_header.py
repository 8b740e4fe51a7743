"""fqss_amd/_lib.py reads the C ABI from include/fqss.h: the struct layouts it derives against the host compiler's own sizeof /
offsetof (a check that does not go through the reader, and that keeps the header valid plain C), and the reader on synthetic
header text -- every accepted form maps to the ctypes type the ABI needs, everything else is refused by name.  No library is loaded."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_struct_layouts_match_the_compiler(tmp_path):
    """sizeof and every field's offsetof of every struct the reader found, printed by a C program that includes fqss.h, built with
    the compiler of fqss_amd/csrc/cpu/Makefile"""
    from fqss_amd import _lib
    hdr = open(_lib.HEADER_PATH).read()
    assert len(_lib.STRUCTS) == len(re.findall(r"\btypedef\s+struct\b", hdr)) >= 11
    want, prints = {}, []
    for name, cls in _lib.STRUCTS.items():
        want[name, "sizeof"] = C.sizeof(cls)
        prints.append(f'    printf("{name} sizeof %zu\\n", sizeof({name}));')
        for field, _ in cls._fields_:
            want[name, field] = getattr(cls, field).offset
            prints.append(f'    printf("{name} {field} %zu\\n", offsetof({name}, {field}));')
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include "fqss.h"\nint main(void) {\n' + "\n".join(prints) + "\n    return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-x", "c", "-std=c11", "-Wall", "-Werror", "-I", os.path.dirname(_lib.HEADER_PATH),
                           str(src), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    got = {(s, f): int(v) for s, f, v in (line.split() for line in out.splitlines())}
    assert got == want, {k: (got.get(k), want.get(k)) for k in set(got) | set(want) if got.get(k) != want.get(k)}


ACCEPTED = """
/* every form the reader accepts */
#ifndef SYNTH_H
#define SYNTH_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define FQSS_SEVEN 7 /* a trailing comment */
#define FQSS_EMINUS (-22)
typedef void* fqss_stream_t;
typedef struct FqssT {
    void* data;       /* a pointer */
    int dtype; int32_t n, m;
    int64_t shape[4];
    float f; double d; size_t s;
} FqssT;
typedef struct {
    const FqssT* t; FqssT* u;
    const float *a, *b;
    const uint8_t* c;
} FqssU;
int fqss_a(void);
const char* fqss_b(void);   // a line comment
int64_t fqss_c(const char* op, const float* x, uint8_t* y, const float* const* r, const FqssT* t, void* ws, int a, int32_t b,
               int64_t c, float d, double e, size_t f, fqss_stream_t stream);
#ifdef __cplusplus
}
#endif
#endif
"""


def test_reader_maps_every_accepted_form():
    from fqss_amd import _lib
    protos, restypes, structs, constants = _lib.parse_header(ACCEPTED)
    assert constants == {"FQSS_SEVEN": 7, "FQSS_EMINUS": -22}
    assert protos == {"fqss_a": [], "fqss_b": [],
                      "fqss_c": [C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int64,
                                 C.c_float, C.c_double, C.c_size_t, C.c_void_p]}
    assert restypes == {"fqss_a": C.c_int, "fqss_b": C.c_char_p, "fqss_c": C.c_int64}
    assert list(structs) == ["FqssT", "FqssU"] and all(issubclass(s, C.Structure) for s in structs.values())
    T, U = structs["FqssT"], structs["FqssU"]
    assert T._fields_ == [("data", C.c_void_p), ("dtype", C.c_int), ("n", C.c_int), ("m", C.c_int), ("shape", C.c_int64 * 4),
                          ("f", C.c_float), ("d", C.c_double), ("s", C.c_size_t)]
    assert U._fields_ == [("t", C.POINTER(T)), ("u", C.POINTER(T)), ("a", C.c_void_p), ("b", C.c_void_p), ("c", C.c_void_p)]


@pytest.mark.parametrize("text, named", [
    ("int fqss_f(uint8_t v);", "uint8_t v"),                                        # a by-value type outside the list
    ("typedef struct { int a; } FqssT; int fqss_f(FqssT t);", "FqssT t"),          # a struct by value
    ("int fqss_f(const float* x, ...);", "fqss_f"),                                 # variadic
    ("int fqss_f(int (*cb)(int), int n);", "fqss_f"),                               # a function-pointer parameter
    ("typedef struct { int a : 3; } FqssT;", "a : 3"),                              # a bit-field
    ("typedef struct { int (*cb)(int); } FqssT;", "cb"),                            # a function-pointer field
    ("typedef struct { struct { int a; } in; int b; } FqssT;", "struct"),           # a nested struct
    ("typedef struct { int a; } FqssA; typedef struct { FqssA a; } FqssB;", "FqssA"),   # a struct field by value
    ("typedef struct { unsigned a; } FqssT;", "unsigned"),                          # a by-value field type outside the list
    ("float fqss_f(int n);", "fqss_f"),                                             # a return type outside the list
    ("typedef int fqss_int;", "fqss_int"),                                          # a typedef other than the stream handle
    ("#define FQSS_MASK 0x10", "FQSS_MASK"),                                        # a constant that is not a decimal integer
    ("#define FQSS_F(x) 1", "FQSS_F"),                                              # a function-like macro
    ("#if FQSS_WIDE\nint fqss_f(int64_t n);\n#endif", "#if"),                       # conditional declarations
])
def test_reader_refuses_what_it_cannot_classify(text, named):
    from fqss_amd import _lib
    with pytest.raises(_lib.FqssError, match=re.escape(named)):
        _lib.parse_header(text)


def test_missing_header_names_the_path(monkeypatch, tmp_path):
    from fqss_amd import _lib
    gone = str(tmp_path / "include" / "fqss.h")
    monkeypatch.setattr(_lib, "HEADER_PATH", gone)
    with pytest.raises(_lib.FqssError, match=re.escape(gone)):
        _lib._read_header()
