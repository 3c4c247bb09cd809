"""Build the HIP product for gfx950 with hipcc (in-tree, so the .so travels
with the repository snapshot to the GPU box)."""
from __future__ import annotations

import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OUT = os.path.join(CSRC, "librtlfm_hip.so")
# The translation units of librtlfm_hip.so - the ONLY list of them: tests and tools take theirs from here.  The .hip
# entries hold device code; FUSED_UNIT names the one that holds the k_fused instances - today the whole rtl_fm library -
# for the prefetch lint, which reads that unit's assembly (first: it compiles longest).
FUSED_UNIT = "rtlfm_hip.hip"
SOURCES = [FUSED_UNIT, "rtlpower_hip.hip", "rtlfm_place.hip", "monitor.cpp", "agc.cpp", "scan.cpp", "snapshot.cpp", "chansnap.cpp", "slots.cpp", "iq.cpp"]
DEVICE_UNITS = [s for s in SOURCES if s.endswith(".hip")]
ARCH = "gfx950"


def _hipcc() -> str:
    for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    raise FileNotFoundError("hipcc not found")


OBJDIR = os.path.join(CSRC, "build")
# -ffile-prefix-map: __FILE__ (HIP_TRY's messages) and every other path the compiler embeds are written relative to the
# repository, so that two checkouts in different directories build the same bytes (a rebuild under /tmp
# differed from the shipped library in its path strings)
ROOT = os.path.dirname(HERE)
FLAGS = [f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC",
         "-Wall", "-Wno-unused-function", "-Wno-unused-result", "-Wno-unused-value",
         f"-ffile-prefix-map={ROOT}=."]


def _obj(src: str) -> str:
    return os.path.join(OBJDIR, os.path.splitext(src)[0] + ".o")


def _flags_key(extra) -> str:
    """(without -ffile-prefix-map: it names the checkout's directory so that the output does NOT depend on it)"""
    return " ".join([f for f in FLAGS if not f.startswith("-ffile-prefix-map=")] + list(extra or []))


def _deps(src: str):
    """What the compiler read when it built the unit (_keep_deps), or None without such a list."""
    try:
        with open(_obj(src) + ".d") as f:
            return [os.path.join(ROOT, d) for d in f.read().split("\n") if d]
    except OSError:
        return None


def _keep_deps(src: str, depfile: str) -> None:
    """The compiler's -MMD depfile (make syntax) as one path per line, those inside the repository relative to it: the
    list still holds when the tree is copied elsewhere together with what was built from it."""
    with open(depfile) as f:
        deps = f.read().replace("\\\n", " ").split(":", 1)[1].split()
    os.remove(depfile)
    deps = sorted({os.path.relpath(d, ROOT) if os.path.abspath(d).startswith(ROOT + os.sep) else d for d in deps})
    with open(_obj(src) + ".d", "w") as f:
        f.write("\n".join(deps) + "\n")


def _unit_stale(src: str, extra=None, built: str | None = None) -> bool:
    """`built` (the unit's object; for needs_build the library) is reused only if it is newer than everything the unit was
    compiled from - the compiler's own list, no hand-kept one - AND was built with the same flags (an A/B build with -D...
    must not leave its objects to a later plain build)."""
    built = built or _obj(src)
    if not os.path.exists(built):
        return True
    try:
        with open(_obj(src) + ".flags") as f:
            if f.read() != _flags_key(extra):
                return True
    except OSError:
        return True
    deps = _deps(src)
    if deps is None:
        return True
    t = os.path.getmtime(built)
    return any(not os.path.exists(d) or os.path.getmtime(d) > t for d in deps)


def needs_build() -> bool:
    """The library is missing, or older than something one of its units was compiled from.  As before, the question is
    put to the library, not to the objects: the library travels with a snapshot of the tree (see the top of this file),
    the objects need not, and such a snapshot is up to date.  (build(extra=...) never asks: a variant is always built.)"""
    return any(_unit_stale(src, built=OUT) for src in SOURCES)


def build(force: bool = False, verbose: bool = False, extra: list[str] | None = None) -> str:
    """One object per translation unit (compiled side by side), then one link: librtlfm_hip.so.  Objects and the
    library are written under a temporary name and renamed, and the whole build holds a file lock: several test
    processes that find the library stale at once (pytest -n) neither link nor load half-written files."""
    if not force and not extra and not needs_build():
        return OUT
    import fcntl
    os.makedirs(OBJDIR, exist_ok=True)
    with open(os.path.join(OBJDIR, ".lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        if not force and not extra and not needs_build():
            return OUT  # another process built it while this one waited
        procs = []
        tag = f".tmp{os.getpid()}"
        for src in SOURCES:
            if not (force or _unit_stale(src, extra)):
                continue
            # -cuid: the compilation unit's id is otherwise a hash that takes the (temporary, per-process) output name in -
            # two builds of the same sources then differ in their symbol names and the library in its bytes
            cmd = ([_hipcc()] + FLAGS + [f"-cuid={os.path.splitext(src)[0]}", "-MMD", "-MF", _obj(src) + ".d" + tag,
                                         "-c", "-o", _obj(src) + tag, os.path.join(CSRC, src)] + (extra or []))
            if verbose:
                print(" ".join(cmd), file=sys.stderr)
            procs.append((src, cmd, subprocess.Popen(cmd)))
        failed = [(cmd, p.returncode) for src, cmd, p in procs if p.wait() != 0]  # (every child is waited for)
        if failed:
            for src, cmd, p in procs:
                for leftover in (_obj(src) + tag, _obj(src) + ".d" + tag):
                    if os.path.exists(leftover):
                        os.remove(leftover)
            raise subprocess.CalledProcessError(failed[0][1], failed[0][0])
        for src, cmd, p in procs:
            os.replace(_obj(src) + tag, _obj(src))
            _keep_deps(src, _obj(src) + ".d" + tag)
            with open(_obj(src) + ".flags", "w") as f:
                f.write(_flags_key(extra))
        cmd = [_hipcc(), f"--offload-arch={ARCH}", "-fPIC", "-shared", "-o", OUT + tag] + [_obj(s) for s in SOURCES]
        _run(cmd, verbose)
        os.replace(OUT + tag, OUT)
    return OUT


HOST = os.path.join(CSRC, "host")
SHIM_OUT = os.path.join(HOST, "librtlsdr_file.so")
CLI_OUT = os.path.join(HOST, "rtl_fm_hip")
POWER_CLI_OUT = os.path.join(HOST, "rtl_power_hip")
INGEST_OUT = os.path.join(HOST, "ingest_bench")


def _run(cmd, verbose: bool) -> None:
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.check_call(cmd)


def build_shim(force: bool = False, verbose: bool = False) -> str:
    """Only the file-backed librtlsdr device layer (plain gcc; no GPU library needed)."""
    inc = os.path.join(CSRC, "..", "..", "include")
    shim_src = os.path.join(HOST, "rtlsdr_file.c")
    deps = [shim_src, os.path.join(inc, "rtlsdr_file.h")]
    if force or not os.path.exists(SHIM_OUT) or any(os.path.getmtime(x) > os.path.getmtime(SHIM_OUT) for x in deps):
        cmd = ["gcc", "-O2", "-fPIC", "-shared", "-Wall", "-Wextra", "-o", SHIM_OUT, shim_src]
        _run(cmd, verbose)
    return SHIM_OUT


def build_host(force: bool = False, verbose: bool = False) -> tuple[str, str]:
    """The file-backed librtlsdr device layer (26 rtlsdr_* symbols) and the rtl_fm-shaped
    CLI that sits on it and on librtlfm_hip.so.  Plain gcc/g++."""
    def stale(out, srcs):
        return force or not os.path.exists(out) or any(os.path.getmtime(x) > os.path.getmtime(out) for x in srcs)
    inc = os.path.join(CSRC, "..", "..", "include")
    build_shim(force, verbose)
    cli_src = os.path.join(HOST, "rtl_fm_hip.cpp")
    if stale(CLI_OUT, [cli_src, SHIM_OUT, OUT, os.path.join(inc, "rtlfm_hip.h"), os.path.join(inc, "rtlfm_monitor.h"),
                       os.path.join(inc, "rtlfm_agc.h"), os.path.join(inc, "rtlfm_iq.h"), os.path.join(inc, "rtlfm_scan.h"), os.path.join(inc, "rtlfm_snapshot.h"),
                       os.path.join(inc, "rtlfm_chansnap.h"),
                       os.path.join(inc, "rtlsdr_file.h")]):
        cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-o", CLI_OUT, cli_src,
               "-L" + HOST, "-L" + CSRC, "-lrtlsdr_file", "-lrtlfm_hip", "-lpthread",
               "-Wl,-rpath,$ORIGIN", "-Wl,-rpath,$ORIGIN/..", "-Wl,-rpath,/opt/rocm/lib",
               "-Wl,--allow-shlib-undefined"]
        _run(cmd, verbose)
    pw_src = os.path.join(HOST, "rtl_power_hip.cpp")
    if stale(POWER_CLI_OUT, [pw_src, SHIM_OUT, OUT, os.path.join(inc, "rtlpower_hip.h")]):
        cmd = ["g++", "-O2", "-std=c++17", "-Wall", "-o", POWER_CLI_OUT, pw_src,
               "-L" + HOST, "-L" + CSRC, "-lrtlsdr_file", "-lrtlfm_hip", "-lm", "-lpthread",
               "-Wl,-rpath,$ORIGIN", "-Wl,-rpath,$ORIGIN/..", "-Wl,-rpath,/opt/rocm/lib",
               "-Wl,--allow-shlib-undefined"]
        _run(cmd, verbose)
    ib_src = os.path.join(HOST, "ingest_bench.cpp")
    if stale(INGEST_OUT, [ib_src, OUT, os.path.join(inc, "rtlfm_hip.h")]):
        # the PCIe-inclusive rate of the callback boundary from native threads (bench.py's e2e leg)
        cmd = ["g++", "-O2", "-std=c++20", "-Wall", "-o", INGEST_OUT, ib_src, "-L" + CSRC, "-lrtlfm_hip", "-lpthread",
               "-Wl,-rpath,$ORIGIN/..", "-Wl,-rpath,/opt/rocm/lib", "-Wl,--allow-shlib-undefined"]
        _run(cmd, verbose)
    return SHIM_OUT, CLI_OUT


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
    print(build_host(force="--force" in sys.argv, verbose=True))
