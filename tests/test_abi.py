"""The C-ABI libraries load and export every symbol the headers declare (no compute, no GPU)."""
import ctypes as C
import os
import re

from amplisolve_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(ampli_[A-Za-z0-9_]+)\s*\(", txt)))


def test_hip_header_symbols_exported():
    names = declared("amplisolve_hip.h")
    assert len(names) >= 25
    lib = C.CDLL(_lib.HIP_LIB_PATH)
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/amplisolve_hip.h but not exported"
    assert set(names) == set(_lib.HIP_SYMBOLS), set(names) ^ set(_lib.HIP_SYMBOLS)


def test_host_header_symbols_exported():
    names = declared("amplisolve_host.h")
    lib = C.CDLL(_lib.HOST_LIB_PATH)
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/amplisolve_host.h but not exported"
    assert set(names) == set(_lib.HOST_SYMBOLS), set(names) ^ set(_lib.HOST_SYMBOLS)


def test_abi_version_and_strerror():
    lib = _lib.hip_lib()
    assert lib.ampli_abi_version() == 5  # AMPLI_ABI_VERSION (5: ampli_error_sums_inorder, round 6)
    assert lib.ampli_strerror(0) == b"ok"
    assert b"HIP" in lib.ampli_strerror(-2)


def test_acc_layout_is_plane_aligned():
    lib = _lib.hip_lib()
    P = 1000
    n = lib.ampli_acc_bytes(P)
    assert n >= P * (64 + 64 + 16 + 4 + 16 * 4)
    t = _lib.AccTable()
    base = 1 << 20
    assert lib.ampli_acc_bind(C.c_void_p(base), P, C.byref(t)) == 0
    ptrs = [t.snt, t.srd, t.cnt, t.nrec, t.gm_n, t.gm_first_af, t.gm_rest, t.gm_first]  # buffer order
    assert all(p % 256 == 0 for p in ptrs) and ptrs == sorted(ptrs) and ptrs[-1] + 16 * P <= base + n
    a, b, c = C.c_size_t(), C.c_size_t(), C.c_size_t()
    assert lib.ampli_acc_regions(P, C.byref(a), C.byref(b), C.byref(c)) == 0
    assert b.value == t.gm_n - base and b.value + c.value == t.gm_first - base and a.value == t.gm_first_af - base


def test_no_gpu_means_loud_failure():
    """Without a device the product must refuse to compute rather than fall back."""
    import torch

    if torch.cuda.is_available():
        return
    lib = _lib.hip_lib()
    h = C.c_void_p()
    assert lib.ampli_ctx_create(0, None, C.byref(h)) == -2
    import pytest

    from amplisolve_amd import AmpliError, Context

    with pytest.raises(AmpliError):
        Context(0)


# ---- the reader of the headers (amplisolve_amd/_headers.py), which the tables, structs and constants above come from ----

HEADER_TEXT = """
#ifndef X_H
#define X_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define AMPLI_T_COUNT 12u          /* a suffix */
#define AMPLI_T_NEG (-7)           /* in parentheses */
#define AMPLI_T_MASK 0xFFFF        /* hexadecimal, ends in F */
#define AMPLI_T_TAG 0x4D4F4E31u
#define AMPLI_T_NA (-999.0f)
#define AMPLI_T_EPS 1e-6
#define AMPLI_T_WORDS (AMPLI_T_COUNT * 16 + AMPLI_T_NEG)
#define AMPLI_T_MIN INT32_MIN
#define AMPLI_T_OWN ((void *)(intptr_t)-1)
typedef struct ampli_t_ctx ampli_t_ctx;
typedef struct ampli_t_pair {
    int32_t a, b; /* two in one declaration */
    double q;
    const float *p, *r;
} ampli_t_pair;
typedef struct ampli_t_outer {
    ampli_t_pair pair; /* an earlier struct */
    uint16_t code;
    int64_t n;
} ampli_t_outer;
typedef struct ampli_t_hooks {
    int (*hook)(void *user);
} ampli_t_hooks;
typedef int (*ampli_t_fn)(void *user, int32_t n);
int ampli_t_version(void);
const char *ampli_t_name(const char *key, char *out, size_t cap);
/* over several lines,
 * with comments inside */
double ampli_t_score(ampli_t_ctx *ctx, const int32_t *d_k /*[n]*/, int64_t n,
                     float err,        /* a scalar */
                     uint64_t out[3], const ampli_t_pair *prm, ampli_t_outer *d_list, ampli_t_ctx **made);
void *ampli_t_stream(ampli_t_ctx *ctx, ampli_t_fn fn, const ampli_t_hooks *hooks, unsigned long long *d_n);
#ifdef __cplusplus
static_assert(sizeof(ampli_t_pair) == 32, "ampli_t_pair is {int32 a; int32 b; double q; ...}, 32 bytes");
}
#endif
#endif
"""


def test_reader_on_literal_header_text():
    import pytest

    from amplisolve_amd._headers import Reader

    class Hooks(C.Structure):
        _fields_ = [("hook", C.CFUNCTYPE(C.c_int, C.c_void_p))]

    FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int32)
    r = Reader(types={"ampli_t_fn": FN, "ampli_t_hooks": Hooks}, data=("ampli_t_outer",))
    protos = r.read(HEADER_TEXT)
    assert r.defines == {"AMPLI_T_COUNT": 12, "AMPLI_T_NEG": -7, "AMPLI_T_MASK": 0xFFFF, "AMPLI_T_TAG": 0x4D4F4E31, "AMPLI_T_NA": -999.0,
                         "AMPLI_T_EPS": 1e-6, "AMPLI_T_WORDS": 185, "AMPLI_T_MIN": -2 ** 31}
    assert {k: type(v) for k, v in r.defines.items() if type(v) is float}.keys() == {"AMPLI_T_NA", "AMPLI_T_EPS"}
    assert set(r.structs) == {"ampli_t_pair", "ampli_t_outer"}
    pair, outer = r.structs["ampli_t_pair"], r.structs["ampli_t_outer"]
    assert pair._fields_ == [("a", C.c_int32), ("b", C.c_int32), ("q", C.c_double), ("p", C.c_void_p), ("r", C.c_void_p)]
    assert outer._fields_ == [("pair", pair), ("code", C.c_uint16), ("n", C.c_int64)]
    assert C.sizeof(pair) == 32 and outer.code.offset == 32 and C.sizeof(outer) == 48
    vp = C.c_void_p
    assert protos == {
        "ampli_t_version": (C.c_int, []),
        "ampli_t_name": (C.c_char_p, [C.c_char_p, C.c_char_p, C.c_size_t]),
        # handle, data pointer, scalars, array parameter, struct pointer, pointer to a struct of the data arrays, pointer to a handle
        "ampli_t_score": (C.c_double, [vp, vp, C.c_int64, C.c_float, vp, C.POINTER(pair), vp, vp]),
        "ampli_t_stream": (vp, [vp, FN, C.POINTER(Hooks), vp]),
    }
    # a name the reader does not know raises and says where; nothing is defaulted
    with pytest.raises(TypeError, match=r"ampli_t_f: parameter n: unknown type 'long'"):
        Reader().read("int ampli_t_f(void *ctx, long n);")
    with pytest.raises(TypeError, match=r"ampli_t_g: parameter h: unknown type 'ampli_t_handle'"):
        Reader().read("int ampli_t_g(ampli_t_handle *h);")
    with pytest.raises(TypeError, match=r"ampli_t_h: result: unknown type 'ssize_t'"):
        Reader().read("ssize_t ampli_t_h(void);")
    with pytest.raises(TypeError, match=r"struct ampli_t_s: member x: unknown type 'wchar_t'"):
        Reader().read("typedef struct ampli_t_s { wchar_t x; } ampli_t_s;")
    with pytest.raises(TypeError, match="by value"):
        Reader().read("typedef struct ampli_t_ctx ampli_t_ctx; int ampli_t_i(ampli_t_ctx ctx);")
    with pytest.raises(TypeError, match="cannot read"):
        Reader().read("int ampli_t_j(int);")


def test_missing_header_is_named(monkeypatch, tmp_path):
    import pytest

    monkeypatch.setattr(_lib, "INCLUDE", str(tmp_path))
    with pytest.raises(_lib.AmpliError, match=str(tmp_path / "amplisolve_hip.h")):
        _lib._header("amplisolve_hip.h")


STRUCTS = {"ampli_acc_table": _lib.AccTable, "ampli_call": _lib.Call, "ampli_loo_call": _lib.LooCall, "ampli_records": _lib.Records,
           "ampli_dilute_mix": _lib.DiluteMix, "ampli_monitor_params": _lib.MonitorParams, "ampli_allelic_params": _lib.AllelicParams,
           "ampli_genotype_params": _lib.GenotypeParams, "ampli_spectrum_params": _lib.SpectrumParams,
           "ampli_exceedance_params": _lib.ExceedanceParams, "ampli_host_shard": _lib.HostShard}
PRINTED = ("AMPLI_ABI_VERSION", "AMPLI_E_INVALID", "AMPLI_NB_NA", "AMPLI_PAIR_NA", "AMPLI_ABSENT", "AMPLI_CALL_COUNTER_WORDS", "AMPLI_EXCEEDANCE_NA",
           "AMPLI_CALL_GATE_EPS", "AMPLI_MON_CONTROL_TAG", "AMPLI_DILUTE_MAX_COUNT")


def test_struct_layouts_and_constants_against_the_compiler(tmp_path):
    """sizeof and every offsetof of the eleven structs, and a handful of constants, as the host compiler sees the three headers"""
    import subprocess

    from amplisolve_amd import build

    lines = ['#include <cstddef>', '#include <cstdio>', '#include "amplisolve_types.h"', '#include "amplisolve_hip.h"', '#include "amplisolve_host.h"',
             'int main() {']
    for cname, cls in STRUCTS.items():
        lines.append(f'    std::printf("{cname} %zu\\n", sizeof({cname}));')
        lines += [f'    std::printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in cls._fields_]
    lines += [f'    std::printf("{name} %.17g\\n", (double)({name}));' for name in PRINTED]
    src, exe = tmp_path / "layout.cpp", tmp_path / "layout"
    src.write_text("\n".join(lines + ["    return 0;", "}", ""]))
    subprocess.run(["g++", *build.CXX_FLAGS, "-I", build.INCLUDE, "-o", str(exe), str(src)], check=True)
    seen = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for cname, cls in STRUCTS.items():
        assert int(seen[cname]) == C.sizeof(cls), cname
        for f, _ in cls._fields_:
            assert int(seen[f"{cname}.{f}"]) == getattr(cls, f).offset, (cname, f)
    for name in PRINTED:
        assert float(seen[name]) == _lib.CONSTANTS[name], name
    assert _lib.CONSTANTS["AMPLI_ABI_VERSION"] == 5 and _lib.CONSTANTS["AMPLI_E_INVALID"] == -1 and _lib.CONSTANTS["AMPLI_ABSENT"] == -2 ** 31
    assert _lib.CONSTANTS["AMPLI_CALL_COUNTER_WORDS"] == 512 and _lib.CONSTANTS["AMPLI_EXCEEDANCE_NA"] == 65535
    assert type(_lib.CONSTANTS["AMPLI_NB_NA"]) is float and type(_lib.CONSTANTS["AMPLI_EXCEEDANCE_NA"]) is int


def test_every_numeric_define_is_read():
    """the independent scan: every #define AMPLI_* of the three headers has a value, but the one that is a cast"""
    names = set()
    for header in ("amplisolve_types.h", "amplisolve_hip.h", "amplisolve_host.h"):
        names |= set(re.findall(r"^#define (AMPLI_[A-Z0-9_]+) ", open(os.path.join(ROOT, "include", header)).read(), flags=re.M))
    assert names - set(_lib.CONSTANTS) == {"AMPLI_STREAM_OWN"} and set(_lib.CONSTANTS) <= names
