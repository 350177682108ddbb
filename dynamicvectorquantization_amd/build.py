"""Build libdvq_hip.so (gfx950) in-tree with hipcc.  No JIT cache: the .so lives next to this file so it
travels with the repo snapshot to the GPU box.

    python -m dynamicvectorquantization_amd.build [--force]

Sources compile in parallel, at most MAX_JOBS (default 16) at a time.  An object is rebuilt when its source, any header under csrc/ or
include/dvq_hip.h is newer than it.
"""
from __future__ import annotations

import concurrent.futures as cf
import glob
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OBJ = os.path.join(CSRC, "_obj")
LIB = os.path.join(HERE, "libdvq_hip.so")
SOURCES = ["vq.hip", "vq_trained.hip", "entropy.hip", "groupnorm.hip", "igemm.hip", "igemm_nt.hip", "igemm_tn.hip", "conv_halo.hip", "misc.hip", "lossnet.hip", "router.hip", "permuter.hip", "transformer.hip", "attention.hip", "attention2.hip", "imgproc.hip", "decode.hip", "cmdlist.hip", "metrics.hip", "nll.hip", "tokens.hip", "imagelog.hip", "trainlog.hip", "normtrack.hip", "jpeg.hip", "jpeg_host.cpp", "codec.hip", "png.hip", "sampleset.hip"]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-munsafe-fp-atomics", "-Wno-unused-result"]
# a .cpp source is host code with no HIP in it (jpeg_host.cpp: the Huffman pass, which also builds with g++ alone)
HOST_FLAGS = ["-O3", "-std=c++17", "-fPIC"]
# per-file additions.  vq.hip: no SLP vectorisation -- it pairs the scalar fp32 bookkeeping between the MFMAs of the argmin main loop
# into v_pk_fma_f32 / v_pk_add_f32, which issue more slowly beside a busy matrix pipe than the two instructions they replace
# imagelog.hip: no contraction -- its bytes are specified operation by operation in fp32 (docs/design/18-image-logging.md); an fma in
# place of a rounded product and a rounded sum changes some of them
EXTRA_FLAGS = {"vq.hip": ["-fno-slp-vectorize"], "imagelog.hip": ["-ffp-contract=off"]}


def _hipcc() -> str:
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(exe):
        raise RuntimeError("hipcc not found: libdvq_hip.so cannot be built on this machine")
    return exe


def headers() -> list:
    """what every object depends on besides its own source: each header under csrc/ and the public one"""
    return sorted(glob.glob(os.path.join(CSRC, "*.h"))) + [os.path.join(HERE, "..", "include", "dvq_hip.h")]


def _stale(target: str, deps) -> bool:
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build(force: bool = False, verbose: bool = True) -> str:
    # DVQ_BUILD_EXTRA_FLAGS: extra compiler flags for A/B builds on the GPU box (e.g. -DDVQ_STREAM_NT=0); use with --force
    flags = FLAGS + os.environ.get("DVQ_BUILD_EXTRA_FLAGS", "").split()
    os.makedirs(OBJ, exist_ok=True)
    hipcc = _hipcc()
    hdrs = headers()
    jobs = []
    objs = []
    for src in SOURCES:
        s = os.path.join(CSRC, src)
        o = os.path.join(OBJ, os.path.splitext(src)[0] + ".o")
        objs.append(o)
        if force or _stale(o, [s] + hdrs):
            jobs.append([hipcc] + (flags if src.endswith(".hip") else HOST_FLAGS) + EXTRA_FLAGS.get(src, []) + ["-c", s, "-o", o])

    def run(cmd):
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed:\n" + " ".join(cmd) + "\n" + r.stdout + r.stderr)
        return cmd[-1]

    if jobs:
        # MAX_JOBS: a shared machine reports every CPU of the host, not the share a command may use
        with cf.ThreadPoolExecutor(max_workers=min(len(jobs), int(os.environ.get("MAX_JOBS", 16)), os.cpu_count() or 4)) as ex:
            for done in ex.map(run, jobs):
                if verbose:
                    print("[dvq build] compiled", os.path.basename(done), flush=True)
    if jobs or force or _stale(LIB, objs):
        run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs)
        if verbose:
            print("[dvq build] linked", LIB, flush=True)
    return LIB


if __name__ == "__main__":
    build(force="--force" in sys.argv)
