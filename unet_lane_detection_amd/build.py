"""Compile the HIP library in-tree: unet_lane_detection_amd/csrc/libunet_hip.so.

hipcc cross-compiles for gfx950 without a GPU, so this runs in the build
container and the resulting .so travels to the GPU box with the snapshot.

Staleness is decided by content, not by mtimes: the SHA-256 over every source
the library is built from (csrc/*.cpp, *.h, *.inc, include/unet_hip.h) and the
compiler flags, plus the first line of `hipcc --version`, are stored next to
the .so in libunet_hip.so.srchash; the library is rebuilt whenever either
differs.  On a box without hipcc (nothing to rebuild with) a shipped .so whose
source digest matches is used as is and one that does not match is an error.
The build runs under a file lock into a temporary file that replaces the
library atomically, so concurrent ranks never load a half-written file.

A rebuild compiles each source of SOURCES to an object under csrc/build/ (kept
out of git), up to 16 at a time, and links the objects.  An object is kept when
the digest recorded beside it still holds: over the files the compiler's own
dependency list (-MD) names for it, the flags and the compiler's version line.
So a change to the host logic recompiles unet_hip.cpp alone, and a change to a
kernel structure's header the units that include it.
"""
from __future__ import annotations

import concurrent.futures
import fcntl
import glob
import hashlib
import os
import re
import shutil
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
ROOT = os.path.dirname(HERE)
LIB = os.path.join(CSRC, "libunet_hip.so")
HASHFILE = LIB + ".srchash"
OBJDIR = os.path.join(CSRC, "build")
# unet_hip.cpp: the host logic and the kernels no structure owns; launch_*.cpp: one unit per kernel structure of the bf16,
# f16x3 and f16q8 tiers, each behind the plain functions of launch.h (the longest compiles first: they start first);
# the others: kernels of the validation pass, of the general loss, of the augmentation stage, of the histogram
# calibration, of the int8 tier's hybrid (fp16) units, of the video path, of the ensemble combine and threshold
# sweep, of lane following (HSV extractor, scan-row centre), of the frame and output diagnostics, of the lane fit, of
# the component labelling, of the lane view, of the frame correction, of the polygon rasteriser and of the gradient
# pass (accumulation, norm, non-finite count), of the multi-class head, loss and confusion matrix and of the int8
# tier's K-class head, code objects of their own
SOURCES = ["unet_hip.cpp", "launch_conv_x3_r512.cpp", "launch_conv_x3_r512_w32.cpp", "launch_conv_x3_t448.cpp",
           "launch_conv_x3_t448_c.cpp", "launch_conv_x3_dec.cpp", "launch_conv_x3_ws.cpp", "launch_conv_q8_r512.cpp",
           "launch_upconv_x3.cpp", "launch_conv_bf16.cpp",
           "validate_kernels.cpp", "loss_kernels.cpp", "augment_kernels.cpp", "calib_kernels.cpp",
           "conv_h16.cpp", "video_kernels.cpp", "ensemble_kernels.cpp", "follow_kernels.cpp", "diagnose_kernels.cpp",
           "lanefit_kernels.cpp", "label_kernels.cpp", "laneview_kernels.cpp", "correct_kernels.cpp",
           "annotate_kernels.cpp", "grad_kernels.cpp", "multiclass_kernels.cpp", "i8_classes_kernels.cpp"]
FLAGS = ["-x", "hip", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-Wno-unused-result",
         "-Wno-unused-value"]


def hipcc_path(required: bool = True):
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if cand and os.path.exists(cand):
            return cand
    if required:
        raise RuntimeError("hipcc not found (set HIPCC)")
    return None


def dependency_files():
    deps = []
    for pat in ("*.cpp", "*.h", "*.inc"):
        deps += glob.glob(os.path.join(CSRC, pat))
    deps.append(os.path.join(ROOT, "include", "unet_hip.h"))
    return sorted(deps)


_HIPCC_VERSION = None


def hipcc_version() -> str:
    """The "HIP version: ..." line of `hipcc --version` (part of the digest: a library built by another compiler is stale); empty on a
    box without hipcc, where the shipped library's recorded digest is compared with the same empty string left out."""
    global _HIPCC_VERSION
    if _HIPCC_VERSION is None:
        cc = hipcc_path(required=False)
        v = ""
        if cc:
            try:
                out = subprocess.run([cc, "--version"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=60)
                lines = out.stdout.strip().splitlines() or [""]
                # the "HIP version:" line, not simply the first one: under rocprofv3 the profiler's preloaded tool
                # prints its own log lines ahead of hipcc's
                v = next((ln for ln in lines if ln.startswith("HIP version")), lines[0])
            except (OSError, subprocess.SubprocessError):
                v = ""
        _HIPCC_VERSION = v
    return _HIPCC_VERSION


def source_digest() -> str:
    h = hashlib.sha256()
    for path in dependency_files():
        h.update(os.path.relpath(path, ROOT).encode())
        with open(path, "rb") as f:
            h.update(hashlib.sha256(f.read()).digest())
    h.update(" ".join(FLAGS + os.environ.get("UNET_HIPCC_FLAGS", "").split()).encode())
    return h.hexdigest()


def _stored():
    """(source digest, compiler version line) recorded next to the library, or (None, None)"""
    try:
        with open(HASHFILE) as f:
            lines = f.read().splitlines()
        return (lines[0].strip() if lines else None), (lines[1].strip() if len(lines) > 1 else "")
    except OSError:
        return None, None


def is_stale() -> bool:
    if not os.path.exists(LIB):
        return True
    digest, compiler = _stored()
    if digest != source_digest():
        return True
    # the compiler is only compared where there is one to rebuild with (the GPU box may lack hipcc)
    return bool(hipcc_path(required=False)) and compiler != hipcc_version()


def user_flags():
    return os.environ.get("UNET_HIPCC_FLAGS", "").split()   # e.g. -DUNET_WS_STAMPS=1 (diagnostic builds only)


def compile_flags():
    return [f for f in FLAGS if f != "-shared"] + ["-c"] + user_flags()


def jobs() -> int:
    n = min(16, os.cpu_count() or 1)
    try:
        n = min(n, int(os.environ["MAX_JOBS"]))
    except (KeyError, ValueError):
        pass
    return max(1, n)


def object_digest(dep_hashes, flags, compiler: str) -> str:
    """Digest of one object: {dependency path: content hash}, the compile flags, the compiler's version line."""
    h = hashlib.sha256()
    for path in sorted(dep_hashes):
        h.update(f"{path}\0{dep_hashes[path]}\0".encode())
    h.update(("\0".join(flags) + "\0\0" + compiler).encode())
    return h.hexdigest()


def object_is_current(recorded, dep_hashes, flags, compiler: str) -> bool:
    """Whether an object whose record holds the digest `recorded` (None: no record) may be kept.  dep_hashes: the
    files its dependency list names, as they are now (None for a file that is gone)."""
    return recorded is not None and None not in dep_hashes.values() and recorded == object_digest(dep_hashes, flags, compiler)


def _dependencies(depfile: str):
    """The prerequisites of a make-style dependency file"""
    with open(depfile) as f:
        text = f.read().replace("\\\n", " ")
    return [d.replace("\\ ", " ") for d in re.findall(r"(?:[^\s\\]|\\.)+", text.split(":", 1)[1])]


def _dep_hashes(depfile: str):
    """{dependency: content hash, None for a file that is gone} and the newest modification time among them.  Every
    file is read anew: the 25 lists name some 8,000 files, ROCm's and the system's headers included, 0.2 s in all."""
    hashes, newest = {}, 0
    for d in _dependencies(depfile):
        try:
            path = os.path.join(CSRC, d)
            with open(path, "rb") as f:
                hashes[d] = hashlib.sha256(f.read()).hexdigest()
            newest = max(newest, os.stat(path).st_mtime_ns)
        except OSError:
            hashes[d] = None
    return hashes, newest


def _compile(cc: str, source: str, force: bool, verbose: bool) -> str:
    """Brings csrc/build/<source>.o up to date and returns its path"""
    obj = os.path.join(OBJDIR, source + ".o")
    flags = compile_flags()
    try:
        with open(obj + ".digest") as f:
            recorded = f.read().strip()
        if not force and os.path.exists(obj) and object_is_current(recorded, _dep_hashes(obj + ".d")[0], flags, hipcc_version()):
            return obj
    except OSError:
        pass
    if os.path.exists(obj + ".digest"):
        os.remove(obj + ".digest")   # a compile that stops half way leaves no record behind
    cmd = [cc] + flags + ["-MD", "-MF", obj + ".d", "-o", obj, source]
    if verbose:
        print(" ".join(cmd), flush=True)
    started = time.time_ns()
    subprocess.run(cmd, check=True, cwd=CSRC)
    if verbose:
        print(f"{source}: {(time.time_ns() - started) / 1e9:.1f} s", flush=True)
    hashes, newest = _dep_hashes(obj + ".d")
    # a dependency written while the compile ran may not be what the object was built from: no record, so the next
    # build compiles this unit again
    if newest < started:
        with open(obj + ".digest", "w") as f:
            f.write(object_digest(hashes, flags, hipcc_version()) + "\n")
    return obj


def build_library(force: bool = False, verbose: bool = False) -> str:
    if not force and not is_stale():
        return LIB
    cc = hipcc_path(required=False)
    if cc is None:
        raise RuntimeError(f"{LIB} is missing or does not match the sources, and there is no hipcc to rebuild it")
    # several ranks may get here at once (bench.py --gpus N, tests/dp_rehearsal.py): one builds, into a temporary file
    # that replaces the library atomically; the others wait on the lock and find it fresh
    with open(LIB + ".lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            if not force and not is_stale():
                return LIB
            tmp = f"{LIB}.tmp.{os.getpid()}"
            try:
                os.makedirs(OBJDIR, exist_ok=True)
                hipcc_version()   # asked once, before the pool's threads all want it
                with concurrent.futures.ThreadPoolExecutor(jobs()) as pool:
                    objs = list(pool.map(lambda src: _compile(cc, src, force, verbose), SOURCES))
                cmd = [cc] + [f for f in FLAGS if f not in ("-x", "hip")] + user_flags() + ["-o", tmp] + objs
                if verbose:
                    print(" ".join(cmd), flush=True)
                subprocess.run(cmd, check=True, cwd=CSRC)
                with open(HASHFILE + ".tmp", "w") as f:
                    f.write(source_digest() + "\n" + hipcc_version() + "\n")
                os.replace(tmp, LIB)
                os.replace(HASHFILE + ".tmp", HASHFILE)
            finally:
                if os.path.exists(tmp):
                    os.remove(tmp)
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)
    return LIB


if __name__ == "__main__":
    print(build_library(force="--force" in sys.argv, verbose=True))
