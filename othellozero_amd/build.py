"""Builds libothellozero_amd.so for gfx950 with hipcc (cross-compiles without a GPU).

    python -m othellozero_amd.build [--force]

The library is built IN-TREE (othellozero_amd/lib/) so that it travels with the source tree.
-ffp-contract=off: the search kernels restate NumPy/Python float semantics that decide discrete
outcomes (SURVEY.md R-FP); the NN kernels spell their FMAs out explicitly.
"""
import concurrent.futures
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIBDIR = os.path.join(HERE, "lib")
LIB = os.path.join(LIBDIR, "libothellozero_amd.so")
SOURCES = ["oz_rules.hip", "oz_search.hip", "oz_net.hip", "oz_train.hip", "oz_replay.hip"]
HEADERS = ["oz_common.h", "oz_internal.h", "oz_minimax.h", "oz_solve.h", "oz_openings.h", "oz_net_h2.h", "oz_net_b3.h", "oz_train_fused.h", os.path.join("..", "..", "include", "othellozero_amd.h")]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fvisibility=hidden",
         "-Wall", "-Wno-unused-function", "-Wno-unused-result", "-Wno-unused-value"]


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    return "hipcc"


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=False):
    os.makedirs(LIBDIR, exist_ok=True)
    hdrs = [os.path.join(CSRC, h) for h in HEADERS]
    objs, jobs = [], []
    for src in SOURCES:
        s = os.path.join(CSRC, src)
        o = os.path.join(LIBDIR, src.replace(".hip", ".o"))
        objs.append(o)
        if force or _stale(o, [s] + hdrs):
            jobs.append([_hipcc()] + FLAGS + os.environ.get("OZ_EXTRA_FLAGS", "").split() + ["-c", s, "-o", o])

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed:\n" + " ".join(cmd) + "\n" + r.stdout + r.stderr)
        return r.stderr

    with concurrent.futures.ThreadPoolExecutor(max_workers=4) as ex:
        for warn in ex.map(run, jobs):
            if verbose and warn:
                print(warn)
    if jobs or force or _stale(LIB, objs):
        run([_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
