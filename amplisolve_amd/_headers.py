"""Reader of the project's C headers (include/amplisolve_*.h): constants, plain structs and prototypes as ctypes.

It reads these headers, not C.  What it relies on is listed in DESIGN 1.1: one declaration per `;`, named parameters, no macros
inside a declaration, function-pointer types only behind a typedef name.  Headers are read in include order, so that a name is
known before it is used.

Type rules:
  * the fixed-width and plain scalar names of SCALARS map to their ctypes; `void` is a result only;
  * `char *` / `const char *` are c_char_p, as argument and as result;
  * a pointer to a struct the reader holds is POINTER(Struct) -- unless the struct is named in `data`: those are the elements of
    data arrays (device buffers, numpy arrays), and a pointer to one is a data pointer like any other;
  * every other pointer is c_void_p: data pointers, the opaque handles (`typedef struct x x;`), pointers to pointers and array
    parameters (`uint64_t out[3]`).  byref(), ctypes arrays, data_ptr() integers and None all convert to it;
  * `types` names what the reader cannot parse (function-pointer typedefs, structs with such members) with its hand-written ctypes;
  * a name that is none of these raises TypeError with the function and the parameter: nothing is ever defaulted.
"""
from __future__ import annotations

import ctypes as C
import re

SCALARS = {"void": None, "char": C.c_char, "int": C.c_int, "unsigned": C.c_uint, "float": C.c_float, "double": C.c_double,
           "size_t": C.c_size_t, "unsigned long long": C.c_ulonglong,
           **{f"{u}int{n}_t": getattr(C, f"c_{u}int{n}") for u in ("", "u") for n in (8, 16, 32, 64)}}
_SUFFIXED = r"\b(0[xX][0-9a-fA-F]+)[uUlL]+\b|\b(\d+\.?\d*(?:[eE][-+]?\d+)?)[uUlLfF]+\b"  # a hexadecimal's F is a digit, a decimal's a suffix


class Reader:
    def __init__(self, types=(), data=()):
        self.types = {**SCALARS, **dict(types)}  # C name -> ctypes of a value; None: void or an opaque handle
        self.data = set(data)
        self.defines = {}                        # AMPLI_X -> int or float
        self.structs = {}                        # C name -> ctypes.Structure

    def ctype(self, spec: str, where: str, result: bool = False):
        """the ctypes type of `const float *`, `int32_t`, `ampli_ctx **`: a parameter's or member's type, or a result's"""
        base = " ".join(w for w in spec.replace("*", " ").split() if w not in ("const", "struct"))
        if base not in self.types:
            raise TypeError(f"{where}: unknown type {base!r}")
        t, stars = self.types[base], spec.count("*")
        if stars == 0 and t is None and not (result and base == "void"):
            raise TypeError(f"{where}: {base!r} by value")
        if stars == 0:
            return t
        if stars == 1 and base == "char":
            return C.c_char_p
        if stars == 1 and t is not None and issubclass(t, C.Structure) and base not in self.data:
            return C.POINTER(t)
        return C.c_void_p

    def declared(self, decl: str, where: str):
        """(name, ctypes type) of `const float *d_thr`, `int32_t S` or `uint64_t out[3]`"""
        m = re.fullmatch(r"(.*?[\s*])(\w+)\s*(\[\w*\])?", decl.strip())
        if not m:
            raise TypeError(f"{where}: cannot read {decl.strip()!r} as a type and a name")
        return m.group(2), self.ctype(m.group(1) + ("*" if m.group(3) else ""), f"{where} {m.group(2)}")

    def read(self, text: str) -> dict:
        """Take one header's constants and structs in; return its prototypes {name: (restype, [argtypes])}."""
        text = re.sub(r'/\*.*?\*/|//[^\n]*|extern\s*"C"\s*\{|"[^"\n]*"', " ", text, flags=re.S)
        for name, expr in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(AMPLI_\w+)[ \t]+(.+)$", text, flags=re.M):
            try:
                value = eval(re.sub(_SUFFIXED, lambda m: m.group(1) or m.group(2), expr), {"__builtins__": {}, "INT32_MIN": -2 ** 31}, self.defines)
            except Exception:
                continue  # not a number (AMPLI_STREAM_OWN is a cast)
            if isinstance(value, (int, float)):
                self.defines[name] = value
        text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)

        def struct(m):
            body, name = m.groups()
            if "(" not in body:  # a struct with function-pointer members is written by hand and named in `types`
                fields = []
                for stmt in filter(None, map(str.strip, body.split(";"))):  # `int32_t a, *b`: the type, then the declarators
                    spec = re.match(r"(?:(?:const|struct|unsigned)\s+)*\w+", stmt).group(0)
                    fields += [self.declared(spec + " " + d, f"struct {name}: member") for d in stmt[len(spec):].split(",")]
                self.types[name] = self.structs[name] = type(name, (C.Structure,), {"_fields_": fields, "__doc__": f"{name} of the headers"})
            return ""

        text = re.sub(r"typedef\s+struct\s+\w+\s*\{(.*?)\}\s*(\w+)\s*;", struct, text, flags=re.S)
        protos = {}
        for stmt in text.split(";"):
            if m := re.fullmatch(r"\s*typedef\s+struct\s+(\w+)\s+\1\s*", stmt):
                self.types.setdefault(m.group(1), None)
            elif m := re.fullmatch(r"\s*([\w\s*]+?)\s*\b(ampli_\w+)\s*\(([^()]*)\)\s*", stmt):
                res, name, args = m.groups()
                args = [] if args.strip() == "void" else [self.declared(a, f"{name}: parameter")[1] for a in args.split(",")]
                protos[name] = (self.ctype(res, f"{name}: result", result=True), args)
        return protos
