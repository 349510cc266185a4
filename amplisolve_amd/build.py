"""Build every native artefact of amplisolve_amd in-tree.

  lib/libamplisolve_hip.so   HIP kernels + C ABI (include/amplisolve_hip.h), hipcc --offload-arch=gfx950
  lib/libamplisolve_host.so  C++ host: BED / ASEQ / error-table parsers, SoA packer, writers (include/amplisolve_host.h)
  bin/<executable>           one per csrc/host/*_main.cpp (EXECUTABLES below): the drop-in command lines and the project's own

Both libraries take the constants and plain structs they share from include/amplisolve_types.h.

hipcc cross-compiles gfx950 without a GPU, so this runs in the CPU-only container too.
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG)
CSRC = os.path.join(PKG, "csrc")
LIB = os.path.join(PKG, "lib")
BIN = os.path.join(PKG, "bin")

HIP_LIB = os.path.join(LIB, "libamplisolve_hip.so")
HOST_LIB = os.path.join(LIB, "libamplisolve_host.so")

# The kernels + their C ABI, one translation unit per stage; what each one holds is the map at the head of csrc/ampli_kernels.hip
# (the timed step itself) and the first lines of each file.
HIP_SOURCES = ["ampli_kernels.hip", "ampli_exchange.hip", "ampli_loo.hip", "ampli_limits.hip", "ampli_dispersion.hip", "ampli_concordance.hip", "ampli_contamination.hip",
               "ampli_amplicon.hip", "ampli_spectrum.hip", "ampli_exceedance.hip", "ampli_overdispersion.hip", "ampli_paired.hip", "ampli_fdr.hip", "ampli_dilution.hip", "ampli_monitor.hip", "ampli_allelic.hip", "ampli_fraction.hip", "ampli_aux.hip",
               "ampli_runtime.hip", "ampli_pileup.hip", "ampli_indel.hip", "ampli_amplicon_count.hip", "ampli_evidence.hip", "ampli_phase.hip", "ampli_comm.hip"]
HIP_HEADERS = ["ampli_bam.h", "ampli_device.h", "ampli_internal.h", "ampli_math.h", "ampli_synth.h"]
# the public headers; amplisolve_types.h is included by the other two and by csrc/ampli_math.h, so both libraries depend on it
INCLUDE = os.path.join(ROOT, "include")
TYPES_H = os.path.join(INCLUDE, "amplisolve_types.h")
HIP_H = os.path.join(INCLUDE, "amplisolve_hip.h")
HOST_H = os.path.join(INCLUDE, "amplisolve_host.h")
# (executable, its main under csrc/host): the two drop-in command lines and computeCounts, then the project's own commands
EXECUTABLES = (("AmpliSolveErrorEstimation", "ee_main.cpp"), ("AmpliSolveVariantCalling", "vc_main.cpp"), ("computeCounts", "cc_main.cpp"),
               ("AmpliSolveLeaveOneOut", "loo_main.cpp"), ("AmpliSolveDetectionLimit", "dl_main.cpp"),
               ("AmpliSolveDetectionPower", "dp_main.cpp"), ("AmpliSolvePanelDispersion", "pd_main.cpp"),
               ("AmpliSolveSampleConcordance", "sc_main.cpp"), ("AmpliSolveContamination", "ct_main.cpp"),
               ("AmpliSolveAmpliconCoverage", "ac_main.cpp"), ("AmpliSolveSubstitutionSpectrum", "ss_main.cpp"),
               ("AmpliSolveNormalExceedance", "ex_main.cpp"), ("AmpliSolveOverdispersedCalling", "od_main.cpp"),
               ("AmpliSolvePairedComparison", "pc_main.cpp"), ("AmpliSolveFalseDiscovery", "fd_main.cpp"),
               ("AmpliSolveInSilicoDilution", "di_main.cpp"), ("AmpliSolveVariantMonitoring", "mo_main.cpp"),
               ("AmpliSolveAllelicImbalance", "ai_main.cpp"), ("AmpliSolveTumourFraction", "tf_main.cpp"),
               ("computeIndelCounts", "ci_main.cpp"), ("computeAmpliconCounts", "ca_main.cpp"),
               ("computeReadEvidence", "re_main.cpp"), ("computePhasing", "ph_main.cpp"))
OBJ = os.path.join(PKG, "build")
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off"]
CXX_FLAGS = ["-O2", "-fPIC", "-std=c++17", "-ffp-contract=off", "-Wall", "-pthread"]


def _newer(target: str, sources: list[str]) -> bool:
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(s) > t for s in sources if os.path.exists(s))


def _run(cmd: list[str]) -> None:
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(" ".join(cmd) + "\n" + r.stdout + r.stderr)
        raise RuntimeError(f"build step failed: {cmd[0]} (exit {r.returncode})")


def hipcc_path() -> str:
    for c in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("hipcc not found; the HIP kernels cannot be built")


def build_hip(force: bool = False) -> str:
    os.makedirs(LIB, exist_ok=True)
    srcs = [os.path.join(CSRC, f) for f in HIP_SOURCES]
    deps = srcs + [os.path.join(CSRC, h) for h in HIP_HEADERS] + [HIP_H, TYPES_H]
    if force or _newer(HIP_LIB, deps):
        # every translation unit to an object of its own, all at once (at most 16 compilers), then one link
        os.makedirs(OBJ, exist_ok=True)
        objs = [os.path.join(OBJ, os.path.splitext(f)[0] + ".o") for f in HIP_SOURCES]
        flags = [f for f in HIPCC_FLAGS if f != "-shared"]
        with ThreadPoolExecutor(max_workers=min(len(srcs), 16)) as pool:
            list(pool.map(lambda so: _run([hipcc_path(), *flags, "-c", "-o", so[1], so[0]]), zip(srcs, objs)))
        _run([hipcc_path(), *HIPCC_FLAGS, "-o", HIP_LIB, *objs])
    return HIP_LIB


def build_host(force: bool = False) -> str:
    os.makedirs(LIB, exist_ok=True)
    os.makedirs(BIN, exist_ok=True)
    hdir = os.path.join(CSRC, "host")
    srcs = [os.path.join(hdir, f) for f in sorted(os.listdir(hdir)) if f.endswith(".cpp") and not f.endswith("_main.cpp")]
    deps = srcs + [os.path.join(hdir, f) for f in os.listdir(hdir) if f.endswith(".hpp")] + [
        os.path.join(CSRC, "ampli_math.h"), os.path.join(CSRC, "ampli_synth.h"), HOST_H, HIP_H, TYPES_H]
    if force or _newer(HOST_LIB, deps):
        _run(["g++", *CXX_FLAGS, "-shared", "-o", HOST_LIB, *srcs, "-ldl", "-lz"])
    for exe, main in EXECUTABLES:
        msrc = os.path.join(hdir, main)
        out = os.path.join(BIN, exe)
        if os.path.exists(msrc) and (force or _newer(out, deps + [msrc, HOST_LIB])):
            _run(["g++", *CXX_FLAGS, "-o", out, msrc, "-L" + LIB, "-lamplisolve_host", "-ldl",
                  "-Wl,-rpath,$ORIGIN/../lib"])
    return HOST_LIB


def build_oracle() -> None:
    """Test infrastructure: the CPU oracle and (when /root/reference exists) the reference builds."""
    _run(["make", "-s", "-C", os.path.join(ROOT, "oracle")])


def build_all(force: bool = False) -> None:
    build_hip(force)
    build_host(force)
    build_oracle()


if __name__ == "__main__":
    build_all(force="--force" in sys.argv)
    print("built:", HIP_LIB, HOST_LIB)
