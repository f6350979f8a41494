"""Build libkv.so (HIP, gfx950) in-tree. Used by __graft_entry__.build()."""
from __future__ import annotations

import glob
import os
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "libkv.so")
SRC = sorted(glob.glob(os.path.join(HERE, "csrc", "*.hip")) + glob.glob(os.path.join(HERE, "csrc", "*.cpp")))
HDR = sorted(glob.glob(os.path.join(HERE, "csrc", "*.h"))) + [os.path.join(HERE, "..", "include", "kv.h")]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function"]


def stale() -> bool:
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    return any(os.path.getmtime(f) > t for f in SRC + HDR)


def build(force: bool = False, verbose: bool = False) -> str:
    if not force and not stale():
        return LIB
    # the objects go to a directory of this build's own (another user's or a concurrent build's leftovers
    # under a fixed name could not be overwritten)
    with tempfile.TemporaryDirectory(prefix="kvbuild_") as tmp:
        objs = []
        procs = []
        for s in SRC:
            o = os.path.join(tmp, os.path.basename(s) + ".o")
            cmd = [HIPCC, *FLAGS, "-c", s, "-o", o]
            if verbose:
                print(" ".join(cmd))
            procs.append((subprocess.Popen(cmd), cmd))
            objs.append(o)
        for p, cmd in procs:
            if p.wait() != 0:
                raise RuntimeError("hipcc failed: " + " ".join(cmd))
        cmd = [HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB + ".tmp", *objs]
        subprocess.check_call(cmd)
    os.replace(LIB + ".tmp", LIB)
    return LIB


if __name__ == "__main__":
    print(build(force=True, verbose=True))
