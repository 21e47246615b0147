"""Build recipe for libmetagym_hip.so (hipcc, gfx950 only, in-tree).

    python -m metagym_amd.build [--force]

The library is compiled into metagym_amd/lib/ so it travels with the source tree to the GPU box
(it is git-ignored, not gpurun-ignored). hipcc cross-compiles gfx950 without a GPU present.
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB_DIR = os.path.join(HERE, "lib")
LIB_PATH = os.path.join(LIB_DIR, "libmetagym_hip.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

# -ffp-contract=off: the reference is NumPy, which never fuses a*b+c; parity (bit-exact against the
# CPU oracle for everything but libm calls) depends on the kernels not fusing either.
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off",
         "-fno-fast-math", "-Wall", "-Wno-unused-function"]


# Per-file additions. quadrotor.hip: without the SLP vectoriser — left on, it packs ~45 of the sub-step's float32 operations into
# v_pk_mul_f32 / v_pk_add_f32 / v_pk_fma_f32 (the dynamic VALU count does not change, round 4), and the step kernel is 1 % slower:
# five alternating A/B pairs of `bench.py --steps 400 --launch eager`, 14.61 / 14.59 / 14.60 / 14.51 us per step with, 14.41 / 14.49 /
# 14.52 / 14.37 without (round 6). Bit-identical results (packed float32 arithmetic is IEEE per lane); the GPU parity tests run on it.
# quadrotor_tasks.hip and quadrotor_policy.hip are built from the same device functions (quadrotor_core.h) and take the same flag.
FILE_FLAGS = {"quadrotor.hip": ["-fno-slp-vectorize"], "quadrotor_tasks.hip": ["-fno-slp-vectorize"],
              "quadrotor_policy.hip": ["-fno-slp-vectorize"]}


def sources():
    return sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hip"))


def _deps():
    deps = [os.path.join(CSRC, f) for f in os.listdir(CSRC)]
    deps.append(os.path.join(os.path.dirname(HERE), "include", "metagym_hip.h"))
    deps.append(os.path.abspath(__file__))
    return deps


def is_stale():
    if not os.path.exists(LIB_PATH):
        return True
    # a library left behind by build(extra_flags=...) (a knock-out / experiment build) is stale for the default build
    flags_file = os.path.join(LIB_DIR, "obj", "flags.txt")
    if os.path.exists(flags_file) and open(flags_file).read() != " ".join(f for f in FLAGS if f != "-shared") + " | " + repr(sorted(FILE_FLAGS.items())):
        return True
    t = os.path.getmtime(LIB_PATH)
    return any(os.path.getmtime(d) > t for d in _deps())


OBJ_DIR = os.path.join(LIB_DIR, "obj")
COMPILE_FLAGS = [f for f in FLAGS if f != "-shared"]


def _object_of(src):
    return os.path.join(OBJ_DIR, os.path.basename(src)[:-4] + ".o")


def depfile_paths(text, base):
    """The files a compiler-written depfile (-MD, Make syntax) names as prerequisites: `\\`-continued lines, `\\ ` for a
    space inside a name, names relative to `base` (the directory the compiler ran in). A rule is split at its first colon:
    the target (our own object path) is assumed to contain none."""
    paths = []
    for rule in text.replace("\\\n", " ").split("\n"):
        if ": " not in rule and not rule.endswith(":"):
            continue
        for name in rule.split(":", 1)[1].replace("\\ ", "\0").split():
            paths.append(os.path.normpath(os.path.join(base, name.replace("\0", " "))))
    return paths


def object_is_stale(obj, depfile, base, recipe):
    """True when `obj` has to be compiled again: it or its depfile is missing or unreadable, or a file the depfile names
    (read relative to `base`) or `recipe` (this build script) is missing or newer than the object. Flags are not its business."""
    try:
        t = os.path.getmtime(obj)
        with open(depfile, errors="replace") as f:
            deps = depfile_paths(f.read(), base)
        return not deps or any(os.path.getmtime(d) > t for d in deps + [recipe])
    except OSError:
        return True


def build(force=False, verbose=True, extra_flags=()):
    """Compile in-tree: one object per .hip (only the stale ones, in parallel — walker.hip alone is minutes), then one link.
    Safe when several ranks of one job import the package at once: the build is serialised by a file lock, re-checked
    under the lock, and the library appears by atomic rename. `extra_flags` (experiments: -D knock-outs) force a rebuild."""
    if not force and not extra_flags and not is_stale():
        return LIB_PATH
    import fcntl
    os.makedirs(OBJ_DIR, exist_ok=True)
    with open(os.path.join(LIB_DIR, ".build.lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            if not force and not extra_flags and not is_stale():      # another process built it while we waited
                return LIB_PATH
            flags_file = os.path.join(OBJ_DIR, "flags.txt")
            flags_now = " ".join(COMPILE_FLAGS + list(extra_flags)) + " | " + repr(sorted(FILE_FLAGS.items()))
            same_flags = os.path.exists(flags_file) and open(flags_file).read() == flags_now
            jobs = []
            for src in sources():
                obj = _object_of(src)
                if force or not same_flags or object_is_stale(obj, obj + ".d", CSRC, os.path.abspath(__file__)):
                    cmd = [HIPCC] + COMPILE_FLAGS + FILE_FLAGS.get(os.path.basename(src), []) + list(extra_flags) + \
                          ["-MD", "-MF", obj + ".d", "-c", src, "-o", obj]
                    if verbose:
                        print(" ".join(cmd), flush=True)
                    jobs.append((cmd, subprocess.Popen(cmd, cwd=CSRC)))
            for cmd, proc in jobs:
                if proc.wait() != 0:
                    raise subprocess.CalledProcessError(proc.returncode, cmd)
            with open(flags_file, "w") as f:
                f.write(flags_now)
            tmp = LIB_PATH + ".tmp.%d" % os.getpid()
            cmd = [HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC"] + [_object_of(x) for x in sources()] + ["-o", tmp]
            if verbose:
                print(" ".join(cmd), flush=True)
            subprocess.check_call(cmd)
            os.replace(tmp, LIB_PATH)
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)
    return LIB_PATH


# The host half of every translation unit (argument validation, plan folding, LDS sizing, topology checks) under ASan + UBSan:
# -Xarch_host keeps the sanitizers off the device code, which is compiled as usual and never runs in this build.
HOST_CHECK_FLAGS = ["-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"]
HOST_CHECK_MAIN = os.path.join(os.path.dirname(HERE), "tests", "host_san", "host_paths.cpp")


def build_host_checked(out_dir, verbose=False):
    """Compile every csrc/*.hip with the normal flags (FILE_FLAGS kept) plus HOST_CHECK_FLAGS into `out_dir`/obj and link the
    objects with tests/host_san/host_paths.cpp — a program with its own main that walks the library's host-only paths — into
    `out_dir`/host_paths. Only stale objects are compiled again (object_is_stale; a change of flags recompiles all). Nothing
    under metagym_amd/lib/ is read or written. Returns the executable's path."""
    out_dir = os.path.abspath(out_dir)         # the compilers run in the sources' directories
    obj_dir = os.path.join(out_dir, "obj")
    os.makedirs(obj_dir, exist_ok=True)
    exe = os.path.join(out_dir, "host_paths")
    recipe = os.path.abspath(__file__)
    flags_file = os.path.join(obj_dir, "flags.txt")
    flags_now = " ".join(COMPILE_FLAGS + HOST_CHECK_FLAGS) + " | " + repr(sorted(FILE_FLAGS.items()))
    same_flags = os.path.exists(flags_file) and open(flags_file).read() == flags_now
    units = [(src, COMPILE_FLAGS + FILE_FLAGS.get(os.path.basename(src), []), CSRC) for src in sources()]
    units.append((HOST_CHECK_MAIN, ["--offload-arch=gfx950", "-std=c++17", "-Wall", "-I", os.path.join(os.path.dirname(HERE), "include")], os.path.dirname(HOST_CHECK_MAIN)))
    jobs, objects = [], []
    for src, flags, cwd in units:
        obj = os.path.join(obj_dir, os.path.splitext(os.path.basename(src))[0] + ".o")
        objects.append(obj)
        if not same_flags or object_is_stale(obj, obj + ".d", cwd, recipe):
            cmd = [HIPCC] + flags + HOST_CHECK_FLAGS + ["-MD", "-MF", obj + ".d", "-c", src, "-o", obj]
            if verbose:
                print(" ".join(cmd), flush=True)
            jobs.append((cmd, subprocess.Popen(cmd, cwd=cwd)))
    for cmd, proc in jobs:
        if proc.wait() != 0:
            raise subprocess.CalledProcessError(proc.returncode, cmd)
    with open(flags_file, "w") as f:
        f.write(flags_now)
    if jobs or not os.path.exists(exe) or any(os.path.getmtime(o) > os.path.getmtime(exe) for o in objects):
        cmd = [HIPCC, "--offload-arch=gfx950"] + HOST_CHECK_FLAGS[2:] + objects + ["-o", exe + ".tmp"]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
        os.replace(exe + ".tmp", exe)
    return exe


if __name__ == "__main__":
    build(force="--force" in sys.argv)
