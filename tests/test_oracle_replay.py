"""The C oracles (oracle/*_oracle.c) and the library's host half under sanitizers and across compilers. CPU only.

oracle/replay_main.c gives the three oracles a main of their own; tests/oracle_replay_cases.py writes the inputs the ctypes
front ends take into a case file. The replay is built five ways into a temporary directory (oracle/Makefile: clang -O1 with
ASan + UBSan, clang -O1 with MSan, gcc -O0, gcc with the library's flags, clang -O2) and run on every case:
  * the sanitized runs exit 0 and print nothing;
  * the five result files are byte-identical: what the oracle computes does not depend on the compiler or its optimiser (for
    cases with a NaN among their inputs: identical but for the sign and payload of NaNs, the byte identity kept as a strict xfail);
  * the result file of the library-flag build equals, call by call, what the ctypes front ends return for the same inputs, so the
    replay runs what the parity tests run;
  * at arguments where this libm's sincos differs from its sin / cos the gcc -O0 and -O2 builds agree (the oracle used to be
    compiled with sin and cos of one argument merged into one sincos, which NumPy never does);
  * a lying, folded centipede fills walker_oracle.c's contact table and overruns its candidate table (-DWO_COUNT_CAPS).
metagym_amd/build.py: build_host_checked links every csrc/*.hip, host code under ASan + UBSan, with tests/host_san/host_paths.cpp,
which walks the refusals and pure-host successes of include/metagym_hip.h without a device.

Nothing here loads sanitized code into python, so no sanitizer runtime is ever preloaded: the module skips when LD_PRELOAD is
set at all, and on a machine with a GPU (sanitizer runs belong to the CPU container)."""
import ctypes as C
import os
import subprocess
import time

import numpy as np
import pytest
import torch

import oracle_replay_cases as orc

if torch.cuda.is_available():
    pytest.skip("sanitizer and cross-compiler replays run on the CPU container, not on a machine with a GPU", allow_module_level=True)
if os.environ.get("LD_PRELOAD"):
    pytest.skip("LD_PRELOAD is set (%r): the sanitized programs are not run under a preloaded library" % os.environ["LD_PRELOAD"],
                allow_module_level=True)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE = os.path.join(ROOT, "oracle")
BUILDS = ("asan", "msan", "gcc_O0", "gcc", "clang_O2")
SANITIZED = ("asan", "msan")
FAMILIES = ("quadrotor", "maze", "walker")
RUN_TIMEOUT = 600


def _env():
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "detect_leaks=1"
    env["UBSAN_OPTIONS"] = "halt_on_error=1:print_stacktrace=1"
    return env


def _make(out_dir, *targets):
    t = time.time()
    p = subprocess.run(["make", "-s", "-C", ORACLE, "-j8", "OUT_DIR=%s" % out_dir] + list(targets), capture_output=True, text=True,
                       timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    return time.time() - t


def _replay(exe, cases, results):
    p = subprocess.run([exe, cases, results], capture_output=True, text=True, timeout=RUN_TIMEOUT, env=_env())
    return p


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    """The replay programs, built cold into a temporary directory, then once more (nothing to do)."""
    out = str(tmp_path_factory.mktemp("replay_build"))
    cold = _make(out, "asan", "msan", "replay", "caps")
    cached = _make(out, "asan", "msan", "replay", "caps")
    print("oracle replay builds: cold %.1f s, cached %.2f s" % (cold, cached))
    return out


@pytest.fixture(scope="module")
def calls():
    return {}


def _calls(calls, family):
    if family not in calls:
        calls[family] = getattr(orc, family + "_calls")()
    return calls[family]


@pytest.fixture(scope="module")
def runs(built, calls, tmp_path_factory):
    """{family: {build: (CompletedProcess, result file)}}: every build of the replay on every family's cases, run once."""
    work = str(tmp_path_factory.mktemp("replay_runs"))
    out = {}
    for family in FAMILIES:
        cases = os.path.join(work, family + ".cases")
        orc.write_cases(cases, _calls(calls, family))
        out[family] = {}
        for b in BUILDS:
            res = os.path.join(work, "%s.%s.res" % (family, b))
            t = time.time()
            out[family][b] = (_replay(os.path.join(built, "replay_" + b), cases, res), res)
            print("replay %s / %s: %d calls, %.1f s" % (family, b, len(calls[family]), time.time() - t))
    return out


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("build", SANITIZED)
def test_sanitized_replay_is_clean(runs, family, build):
    p, _ = runs[family][build]
    assert p.returncode == 0 and p.stderr == "" and p.stdout == "", (p.returncode, p.stdout[-2000:], p.stderr[-6000:])


def _first_difference(calls, a, b):
    ra, rb = orc.read_results(a), orc.read_results(b)
    assert len(ra) == len(rb) == len(calls)
    for c, (_, xa), (_, xb) in zip(calls, ra, rb):
        if xa != xb:
            k = next((i for i, (u, v) in enumerate(zip(xa, xb)) if u != v), min(len(xa), len(xb)))
            return "call %r, output blob %d" % (c.name, k)
    return "headers only"


def _disagreements(runs, calls, family, nan, same):
    """The calls of `family` with (nan) or without NaN inputs on which some build's outputs are not `same` as replay_gcc_O0's."""
    for b in BUILDS:
        assert runs[family][b][0].returncode == 0, (b, runs[family][b][0].stderr[-3000:])
    ref = orc.read_results(runs[family]["gcc_O0"][1])
    assert len(ref) == len(calls[family])
    bad = []
    for b in BUILDS:
        if b == "gcc_O0":
            continue
        got = orc.read_results(runs[family][b][1])
        assert len(got) == len(ref)
        for c, (_, xr), (_, xg) in zip(calls[family], ref, got):
            if c.nan == nan and not (len(xr) == len(xg) and all(same(c, k, len(xr), u, v) for k, (u, v) in enumerate(zip(xr, xg)))):
                bad.append((b, c.name))
    return bad


def _same_bytes(c, k, n_blobs, u, v):
    return u == v


def _same_but_nan_bits(c, k, n_blobs, u, v):
    """Equal bytes, except that a NaN may be another NaN. Only in the floating-point part of output blob k of call c: the
    integers (done, failed, ct, episode, steps and flags; Call.int_tail says where they are) have to be equal as they stand.
    The floats are read as float32 words, in which the high word of a float64 NaN is a NaN as well and its low word (zero in
    every NaN x86-64 arithmetic makes or passes on here) has to be equal."""
    if u == v:
        return True
    tail = c.int_tail(k, n_blobs)
    if tail < 0 or len(u) != len(v):
        return False
    if tail and u[-tail:] != v[-tail:]:
        return False
    u, v = u[:len(u) - tail], v[:len(v) - tail]
    if len(u) % 4:
        return False
    a, b = np.frombuffer(u, np.float32), np.frombuffer(v, np.float32)
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


@pytest.mark.parametrize("family", FAMILIES)
def test_all_builds_agree_byte_for_byte(runs, calls, family):
    """No tolerance: sanitizer, compiler and optimisation level change no byte of any output of any case without a NaN among
    its inputs (NaN, +-inf and out-of-range values that do not end in a NaN included)."""
    assert sum(not c.nan for c in calls[family]) >= {"quadrotor": 100, "maze": 2000, "walker": 240}[family]
    bad = _disagreements(runs, calls, family, False, _same_bytes)
    assert not bad, bad[:20]


NAN_FAMILIES = ("quadrotor", "walker")      # the maze oracle's inputs are integers and clipped actions


@pytest.mark.parametrize("family", NAN_FAMILIES)
def test_nan_cases_agree_in_everything_but_the_bits_of_a_nan(runs, calls, family):
    """Cases with a NaN or an infinity among their inputs (inf - inf and 0 * inf make a NaN, so an infinite state or action is
    treated like one): every build has a NaN where another has one, and every other value is the same to the bit (the finite
    entries of observations and states; failure codes, done flags and counters compared as the integers they are)."""
    assert sum(c.nan for c in calls[family]) >= 4
    bad = _disagreements(runs, calls, family, True, _same_but_nan_bits)
    assert not bad, bad[:20]


@pytest.mark.parametrize("family", NAN_FAMILIES)
@pytest.mark.xfail(strict=True, reason="sign and payload of a NaN that arithmetic propagates depend on which operand the compiler puts "
                   "first (x86-64 keeps the first operand's NaN, and makes a negative one from inf - inf); every float operation of "
                   "quadrotor_oracle.c:qo_substep / qo_observe and walker_oracle.c:wo_substep / calc_state that a NaN state or "
                   "action reaches is such a site (DESIGN.md §4.2)")
def test_nan_cases_agree_byte_for_byte(runs, calls, family):
    bad = _disagreements(runs, calls, family, True, _same_bytes)
    assert not bad, bad[:20]


@pytest.mark.parametrize("family", FAMILIES)
def test_replay_runs_what_the_ctypes_front_ends_run(runs, calls, family):
    """Every call of every family (so every entry point the front ends expose) through oracle/quadrotor.py, oracle/maze.py and
    oracle/walker_c.py on the same inputs: the same bytes as the replay built with the library's flags."""
    assert runs[family]["gcc"][0].returncode == 0
    results = orc.read_results(runs[family]["gcc"][1])
    assert len(results) == len(calls[family])
    ops = set()
    for c, (op, got) in zip(calls[family], results):
        want = c.expect()
        assert op == c.op and len(got) == len(want), (c.name, len(got), len(want))
        for k, (g, w) in enumerate(zip(got, want)):
            assert g == w, "%r: output blob %d of the replay is not what the ctypes front end returns" % (c.name, k)
        ops.add(op)
    assert ops == {"quadrotor": set(range(1, 10)), "maze": {16, 17}, "walker": {32, 33, 34}}[family]


def _undefined_symbols(lib):
    """The names `nm -u -D` lists, without their version suffix."""
    out = subprocess.run(["nm", "-u", "-D", lib], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1].split("@")[0] for line in out.splitlines() if line.split()}


def test_oracle_libraries_do_not_import_sincos():
    """The finding this module started from: gcc -O2 merged the oracle's sin(x) and cos(x) into sincos(x). Both compile lines:
    the library of oracle/Makefile and the counting build of walker_oracle.c in oracle/walker_c.py. This is also the only check
    that guards the maze oracle's two call sites (see test_sincos_regression)."""
    from oracle import quadrotor as qo
    from oracle import walker_c as wc
    for lib in (qo.build(), wc.build_count()):
        names = _undefined_symbols(lib)
        assert "sincos" not in names and "sincosf" not in names, (lib, sorted(names))
        assert "sin" in names and "cos" in names, (lib, sorted(names))


def _sincos_differs(x):
    """Where this libm's sincos(x) is not (sin(x), cos(x)): bool [len(x)]."""
    libm = C.CDLL("libm.so.6")
    libm.sincos.argtypes = [C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    libm.sincos.restype = None
    libm.sin.restype = libm.cos.restype = C.c_double
    libm.sin.argtypes = libm.cos.argtypes = [C.c_double]
    s, c = C.c_double(), C.c_double()
    out = np.zeros(len(x), bool)
    for i, v in enumerate(x):
        v = float(v)
        libm.sincos(v, C.byref(s), C.byref(c))
        out[i] = s.value != libm.sin(v) or c.value != libm.cos(v)
    return out


SINCOS_DRAWS = 1000000


@pytest.fixture(scope="module")
def sincos_arguments():
    """Headings in [0, 2 pi) and joint angles in [-1, 1] at which this libm's sincos differs from its sin / cos, found by search
    (libm called value by value through ctypes: numpy's own sine is not libm's)."""
    rs = np.random.RandomState(2024)
    headings, joints = rs.uniform(0.0, 6.2831852, SINCOS_DRAWS), rs.uniform(-1.0, 1.0, SINCOS_DRAWS)
    found = []
    for x in (headings, joints):
        found.append(x[_sincos_differs(x)])
    return found


def test_sincos_regression(built, sincos_arguments, tmp_path):
    """At >= 32 headings and >= 32 joint angles where sincos(x) != (sin(x), cos(x)) in this libm, mo_step_cont3d / mo_observe_3d and
    wo_env_step give the same bytes compiled by gcc -O0 (separate calls whatever the flags) and by gcc -O2 with the Makefile's flags.

    What this can catch: built without -fno-builtin-sin / -cos, the walker cases differ (first at 'joint angles 0'). The maze
    cases do not: without the flags maze_oracle.c does call sincos at both sites, but no output was seen to move at any of the
    1392 headings the search finds, with 32 x 32, 256 x 32 or 256 x 256 frames. mo_step_cont3d rounds cos(x) * off to float32
    (an ulp of the double survives one time in 2^29) and an ulp in mo_observe_3d's sin / cos moves a pixel only where a ray
    meets a texel or cell edge to within that ulp. The maze half is kept as the assertion the oracle is trusted under; what
    guards the maze call sites against the merge coming back is test_oracle_libraries_do_not_import_sincos."""
    import maze_large_cases as ml
    from oracle import maze as mo
    headings, joints = sincos_arguments
    print("sincos != sin, cos at %d of %d headings and %d of %d joint angles" % (len(headings), SINCOS_DRAWS, len(joints), SINCOS_DRAWS))
    assert len(headings) >= 32 and len(joints) >= 32
    cases = []
    task = orc._otask(ml.synthetic_task(15, 115))
    view = orc.maze_view(32, 32)
    cs = task.c.cell_size
    for k, h in enumerate(headings[:64]):
        # turn 0, so that every sub-step of the move evaluates sin and cos AT the heading; the frame is rendered from it
        start = dict(ori=float(h), loc=(float(np.float32(1.5 * cs)), float(np.float32(1.5 * cs))), grid=(1, 1))
        cases.append(orc.m_episode("heading %d" % k, task, mo.ESCAPE, 2, [(0.0, 1.0)], view=view, start=start))
    setup = orc.walker_setup("humanoid@mujoco")
    nj = setup[1].nj
    for k in range(0, min(len(joints), 64 * nj) - nj + 1, nj):
        env = orc.posed_env(setup, z=1.2, q=joints[k:k + nj])
        cases.append(orc.w_episode("joint angles %d" % k, setup, np.zeros((1, nj), np.float32), env=env))
    path = str(tmp_path / "sincos.cases")
    orc.write_cases(path, cases)
    res = {}
    for b in ("gcc_O0", "gcc"):
        res[b] = str(tmp_path / ("sincos.%s.res" % b))
        p = _replay(os.path.join(built, "replay_" + b), path, res[b])
        assert p.returncode == 0, p.stderr
    if open(res["gcc_O0"], "rb").read() != open(res["gcc"], "rb").read():
        pytest.fail("gcc -O0 and gcc -O2 differ at %s" % _first_difference(cases, res["gcc_O0"], res["gcc"]))


def test_contact_tables_reach_their_caps(built, calls, tmp_path):
    """The walker cases fill WO_MAX_CONTACTS (12 kept of more candidates) and overrun WO_MAX_CANDIDATES (48: self-collision pairs
    left untested because the table is full), so the sanitized runs above have been through both bounds. The third bound, a
    ground candidate dropped for a full table, cannot be reached: no robot has more than 29 collision proxies."""
    path = str(tmp_path / "walker.cases")
    orc.write_cases(path, _calls(calls, "walker"))
    p = _replay(os.path.join(built, "replay_caps"), path, str(tmp_path / "walker.res"))
    assert p.returncode == 0, p.stderr
    print(p.stdout.strip())
    caps = dict(kv.split("=") for kv in p.stdout.split()[1:])
    assert int(caps["max_contacts"]) == 12 and int(caps["max_candidates"]) == 48, caps
    assert int(caps["pairs_cut"]) > 0 and int(caps["ground_dropped"]) == 0, caps


# ---- the library's host half -------------------------------------------------------------------------------------------------

def test_host_paths_under_asan_and_ubsan():
    """build_host_checked compiles every csrc/*.hip with the host side under ASan + UBSan (objects cached under build/) and links
    tests/host_san/host_paths.cpp; the program checks every return code against the header's contract and exits non-zero on a
    mismatch. Leaks inside the HIP / HSA runtime are suppressed by library name (tests/host_san/lsan.supp), nothing else."""
    from metagym_amd import build as mb
    out_dir = os.path.join(ROOT, "build", "host_checked")
    lib_before = os.path.getmtime(mb.LIB_PATH) if os.path.exists(mb.LIB_PATH) else None
    t = time.time()
    exe = mb.build_host_checked(out_dir)
    first = time.time() - t
    t = time.time()
    assert mb.build_host_checked(out_dir) == exe
    print("build_host_checked: %.1f s, again %.2f s" % (first, time.time() - t))
    assert (os.path.getmtime(mb.LIB_PATH) if os.path.exists(mb.LIB_PATH) else None) == lib_before
    env = _env()
    env["LSAN_OPTIONS"] = "suppressions=%s:print_suppressions=0" % os.path.join(ROOT, "tests", "host_san", "lsan.supp")
    env["HIP_VISIBLE_DEVICES"] = ""
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stdout[-3000:], p.stderr[-6000:])
    assert "checks passed" in p.stdout
