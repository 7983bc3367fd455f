"""Build the in-tree HIP library ``cmpc/lib/libcmpc.so`` for gfx950 (hipcc, no JIT cache)."""
from __future__ import annotations

import os
import subprocess
import sys
from pathlib import Path

PKG = Path(__file__).resolve().parent
ROOT = PKG.parent                       # convex-mpc-unitree-go2_amd/
REPO = ROOT.parent
CSRC = ROOT / "csrc"
LIB = PKG / "lib" / "libcmpc.so"
SOURCES = [CSRC / "cmpc_host.hip"]
# everything the one translation unit includes: a change to any of them rebuilds the library
DEPS = sorted(CSRC.glob("*.hip")) + sorted(CSRC.glob("*.h")) + [REPO / "include" / "cmpc.h"]
ARCH = os.environ.get("CMPC_OFFLOAD_ARCH", "gfx950")


def hipcc() -> str:
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc"):
        if c and Path(c).exists():
            return c
    return "hipcc"


def needs_build() -> bool:
    if not LIB.exists():
        return True
    t = LIB.stat().st_mtime
    return any(d.stat().st_mtime > t for d in DEPS if d.exists())


def build_library(force: bool = False, verbose: bool = False) -> Path:
    if not force and not needs_build():
        return LIB
    LIB.parent.mkdir(parents=True, exist_ok=True)
    cmd = [hipcc(), f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", "-shared",
           "-fno-slp-vectorize",  # keep f32 adds scalar so DPP operands fuse (no v_pk_*)
           # MFMA accumulators in VGPR form: the one-wave-per-SIMD kernels (512 registers) then
           # hold the NC 160 tiles without spilling (<160, 144>: 249 VGPRs spilled -> 0; config 3
           # 9.61 -> 9.33 ms, config 2 at 65,536 11.39 -> 10.83 ms, A/B in one gpurun call)
           "-mllvm", "-amdgpu-mfma-vgpr-form",
           f"-I{REPO / 'include'}", f"-I{CSRC}", *map(str, SOURCES), "-o", str(LIB) + ".tmp"]
    if verbose:
        print(" ".join(cmd))
    r = subprocess.run(cmd, stderr=subprocess.PIPE, text=True)
    if r.stderr:
        print(r.stderr, end="", file=sys.stderr)
    if r.returncode != 0:
        # -amdgpu-mfma-vgpr-form is an internal LLVM option.  Only a compiler that rejects it or
        # crashes (not a source error) is retried without it -- and only on explicit request,
        # since that library spills in the one-wave-per-SIMD kernels (slower, same results)
        flag_issue = ("amdgpu-mfma-vgpr-form" in r.stderr or r.returncode < 0 or
                      "PLEASE submit a bug report" in r.stderr)
        if not (flag_issue and os.environ.get("CMPC_BUILD_ALLOW_NO_VFORM") == "1"):
            hint = (" (the compiler rejected or crashed on -amdgpu-mfma-vgpr-form: set "
                    "CMPC_BUILD_ALLOW_NO_VFORM=1 to build without it, at the cost of spills)"
                    if flag_issue else "")
            raise RuntimeError(f"cmpc.build: hipcc failed with exit code {r.returncode}{hint}")
        vf = cmd.index("-amdgpu-mfma-vgpr-form")
        cmd = cmd[:vf - 1] + cmd[vf + 1:]
        print("cmpc.build: WARNING: retrying without -mllvm -amdgpu-mfma-vgpr-form "
              "(CMPC_BUILD_ALLOW_NO_VFORM=1): the one-wave-per-SIMD kernels will spill",
              file=sys.stderr)
        subprocess.run(cmd, check=True)
    os.replace(str(LIB) + ".tmp", LIB)
    return LIB


if __name__ == "__main__":
    print(build_library(force=True, verbose=True))
