"""ctypes bindings of the two native libraries.  No arithmetic lives here.

libamplisolve_hip.so is the product's compute path; if it is missing or no
MI355X is visible, every compute call raises -- there is no CPU fallback.

Nothing of the ABI is written out here: the prototype tables HIP_SYMBOLS and HOST_SYMBOLS, the struct classes and CONSTANTS (the
value of every numeric #define AMPLI_*) are read from include/amplisolve_types.h, amplisolve_hip.h and amplisolve_host.h when the
module is imported (_headers.py states the type rules).  By hand stand only the function-pointer types, HostShard and CHUNK_FN,
which the headers' names are mapped to below (tests/test_abi.py holds their layout against the compiler's, like that of the rest).
"""
from __future__ import annotations

import ctypes as C
import os

from ._headers import Reader

PKG = os.path.dirname(os.path.abspath(__file__))
INCLUDE = os.path.join(os.path.dirname(PKG), "include")  # where build.py takes the headers from
HIP_LIB_PATH = os.environ.get("AMPLISOLVE_HIP_LIB") or os.path.join(PKG, "lib", "libamplisolve_hip.so")
HOST_LIB_PATH = os.environ.get("AMPLISOLVE_HOST_LIB") or os.path.join(PKG, "lib", "libamplisolve_host.so")

vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64


class AmpliError(RuntimeError):
    pass


class AmpliNoDevice(AmpliError):
    """hipGetDeviceCount found nothing (or failed): the message carries HIP's own error name and text"""


class HostShard(C.Structure):
    """mirror of ampli_host_shard (include/amplisolve_host.h): one shard of a multi-process run + its collective hooks"""
    EE_BUFFERS = C.CFUNCTYPE(C.c_int, vp, i64, C.POINTER(vp))
    HOOK = C.CFUNCTYPE(C.c_int, vp)
    OR_FLAGS = C.CFUNCTYPE(C.c_int, vp, C.POINTER(i32))
    ROWS_BEFORE = C.CFUNCTYPE(C.c_int, vp, i64, C.POINTER(i64))
    _fields_ = [("index", i32), ("count", i32), ("user", vp), ("ee_buffers", EE_BUFFERS), ("ee_exchange", HOOK),
                ("ee_gather", HOOK), ("or_flags", OR_FLAGS), ("rows_before", ROWS_BEFORE), ("barrier", HOOK)]


CHUNK_FN = C.CFUNCTYPE(C.c_int, vp, i32, i32, i32, i64, i64, vp, vp, vp, vp, vp, vp, vp, i64)


def _header(name: str) -> str:
    path = os.path.join(INCLUDE, name)
    if not os.path.exists(path):
        raise AmpliError(f"{path} is missing: the bindings are read from the C headers")
    with open(path) as f:
        return f.read()


# what the reader cannot parse, by its name in the headers; and the structs that are elements of data arrays, not descriptors
_abi = Reader(types={"ampli_host_chunk_fn": CHUNK_FN, "ampli_host_shard": HostShard}, data=("ampli_call", "ampli_loo_call", "ampli_dilute_mix"))
_abi.read(_header("amplisolve_types.h"))
HIP_SYMBOLS = _abi.read(_header("amplisolve_hip.h"))    # every symbol include/amplisolve_hip.h declares: (restype, argtypes)
HOST_SYMBOLS = _abi.read(_header("amplisolve_host.h"))  # the same for include/amplisolve_host.h
CONSTANTS = _abi.defines
AccTable = _abi.structs["ampli_acc_table"]
Call = _abi.structs["ampli_call"]
LooCall = _abi.structs["ampli_loo_call"]
Records = _abi.structs["ampli_records"]
DiluteMix = _abi.structs["ampli_dilute_mix"]
MonitorParams = _abi.structs["ampli_monitor_params"]
AllelicParams = _abi.structs["ampli_allelic_params"]
FractionParams = _abi.structs["ampli_fraction_params"]
GenotypeParams = _abi.structs["ampli_genotype_params"]
SpectrumParams = _abi.structs["ampli_spectrum_params"]
ExceedanceParams = _abi.structs["ampli_exceedance_params"]

_hip = None
_host = None


def _bind(lib, table):
    for name, (res, args) in table.items():
        fn = getattr(lib, name)  # AttributeError = missing export: let it propagate
        fn.restype = res
        fn.argtypes = args
    return lib


def hip_lib():
    """Load libamplisolve_hip.so (needs the ROCm runtime, not a GPU, to load)."""
    global _hip
    if _hip is None:
        if not os.path.exists(HIP_LIB_PATH):
            raise AmpliError(f"{HIP_LIB_PATH} is not built: run `python -m amplisolve_amd.build`; there is no CPU fallback")
        _hip = _bind(C.CDLL(HIP_LIB_PATH), HIP_SYMBOLS)
    return _hip


def host_lib():
    global _host
    if _host is None:
        if not os.path.exists(HOST_LIB_PATH):
            raise AmpliError(f"{HOST_LIB_PATH} is not built: run `python -m amplisolve_amd.build`")
        _host = _bind(C.CDLL(HOST_LIB_PATH), HOST_SYMBOLS)
    return _host
