"""How the library's translation units are built (metagym_amd/build.py): an object is stale by what the compiler's depfile
names, not by a hand-kept list of who includes whom, and a unit that sits on a family's core header emits its own kernels
and no copy of the family's. CPU only (hipcc cross-compiles without a GPU)."""
import os
import re
import subprocess

import pytest

from metagym_amd import build as hip_build


# ---- object_is_stale on fake files -------------------------------------------------------------------------------------

def _touch(path, t, text=""):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write(text)
    os.utime(path, (t, t))


@pytest.fixture
def unit(tmp_path):
    """A fake unit: sources at t = 1000, the depfile hipcc would write (continued lines; a relative name, an absolute one and
    one with `..`), the object at t = 2000. Returns the paths and a function that answers object_is_stale()."""
    src = tmp_path / "csrc"
    names = {"hip": src / "x_policy.hip", "core": src / "x_core.h", "common": src / "mg_common.h",
             "abi": tmp_path / "include" / "abi.h", "recipe": tmp_path / "build.py"}
    for p in names.values():
        _touch(str(p), 1000)
    obj = tmp_path / "obj" / "x_policy.o"
    dep = "%s: %s \\\n  x_core.h \\\n  %s \\\n  %s/../include/abi.h\n" % (obj, names["hip"], names["common"], src)
    _touch(str(obj) + ".d", 1000, dep)
    _touch(str(obj), 2000)
    names.update(obj=obj, dep=str(obj) + ".d", base=src)
    names["stale"] = lambda: hip_build.object_is_stale(str(obj), str(obj) + ".d", str(src), str(names["recipe"]))
    return names


def test_depfile_paths_reads_what_the_compiler_writes(unit):
    got = hip_build.depfile_paths(open(unit["dep"]).read(), str(unit["base"]))
    assert got == [str(unit[k]) for k in ("hip", "core", "common", "abi")]
    assert hip_build.depfile_paths("a.o: with\\ space.h b.h\n", "/d") == ["/d/with space.h", "/d/b.h"]


def test_fresh_when_every_dependency_is_older(unit):
    assert not unit["stale"]()


def test_stale_without_a_depfile(unit):
    os.remove(unit["dep"])
    assert unit["stale"]()


def test_stale_without_an_object(unit):
    os.remove(str(unit["obj"]))
    assert unit["stale"]()


def test_stale_when_the_depfile_names_a_missing_file(unit):
    os.remove(str(unit["abi"]))
    assert unit["stale"]()


@pytest.mark.parametrize("newer", ["hip", "core", "common", "abi", "recipe"])
def test_stale_for_one_newer_dependency(unit, newer):
    """Each file alone: the unit's own text, the core header named relative to the compiler's directory on a continued line
    (what "rebuilt when bandits.hip changes" was for the closed-loop units), an absolute name, one through `..`, the recipe."""
    os.utime(str(unit[newer]), (3000, 3000))
    assert unit["stale"]()


def test_stale_for_a_depfile_that_names_nothing(unit):
    _touch(unit["dep"], 1000, "")
    assert unit["stale"]()


# ---- one kernel per unit: a unit emits the kernels it launches ---------------------------------------------------------

def _kernels(tmp_path, src):
    """Demangled-prefix names of the kernels in the device assembly of one unit, compiled with build.py's own flags."""
    out = tmp_path / (src + ".s")
    cmd = [hip_build.HIPCC] + hip_build.COMPILE_FLAGS + hip_build.FILE_FLAGS.get(src, []) + \
          ["--cuda-device-only", "-S", os.path.join(hip_build.CSRC, src), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    symbols = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", out.read_text(), re.M)
    # _ZN12_GLOBAL__N_1<len><name>...: the name of a kernel in the unit's anonymous namespace
    names = []
    for s in symbols:
        m = re.match(r"_ZN12_GLOBAL__N_1(\d+)", s)
        assert m, s
        names.append(s[m.end():m.end() + int(m.group(1))])
    return sorted(names)


def test_bandits_policy_emits_its_own_kernel_only(tmp_path):
    assert _kernels(tmp_path, "bandits_policy.hip") == ["bandits_policy_rollout_kernel"]


def test_quadrotor_tasks_emits_its_own_kernels_only(tmp_path):
    assert _kernels(tmp_path, "quadrotor_tasks.hip") == ["quadrotor_tasks_reset_kernel", "quadrotor_tasks_step_kernel",
                                                         "quadrotor_tasks_step_kernel"]
