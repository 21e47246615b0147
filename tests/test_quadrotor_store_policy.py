"""The store / load policy macros of csrc/quadrotor_core.h (MG_QUAD_ST_*, MG_QUAD_STP_*, MG_QUAD_LD_STATE): the two quadrotor
translation units compile for gfx950 with every policy value, and a value that names no policy is a compile-time error
(static_assert). Compiles only (hipcc cross-compiles without a GPU); what the policies do on the device is
tests/test_quadrotor_store_policy_gpu.py."""
import os
import subprocess

import pytest

from metagym_amd import build as hip_build

ST_MACROS = ("MG_QUAD_ST_STATE", "MG_QUAD_ST_OBS", "MG_QUAD_ST_SCALAR", "MG_QUAD_STP_STATE", "MG_QUAD_STP_OBS", "MG_QUAD_STP_SCALAR")
ST_POLICIES = {"plain": 0, "nt": 2, "sc1": 16, "sc0_sc1": 17, "sc1_nt": 18}
SOURCES = ("quadrotor.hip", "quadrotor_tasks.hip")


def _compile(tmp_path, src, defines):
    """The device side of one translation unit with build.py's own flags plus `defines`; returns the finished process."""
    cmd = [hip_build.HIPCC] + hip_build.COMPILE_FLAGS + hip_build.FILE_FLAGS.get(src, []) + \
          ["-D%s=%d" % kv for kv in defines.items()] + \
          ["--cuda-device-only", "-c", os.path.join(hip_build.CSRC, src), "-o", str(tmp_path / (src + ".o"))]
    return subprocess.run(cmd, capture_output=True, text=True)


@pytest.mark.parametrize("name", list(ST_POLICIES))
def test_every_store_policy_compiles(tmp_path, name):
    """All six classes at once on the given policy, both translation units."""
    for src in SOURCES:
        r = _compile(tmp_path, src, {m: ST_POLICIES[name] for m in ST_MACROS})
        assert r.returncode == 0, r.stderr[-2000:]


def test_nt_state_loads_compile(tmp_path):
    r = _compile(tmp_path, "quadrotor.hip", {"MG_QUAD_LD_STATE": 2})
    assert r.returncode == 0, r.stderr[-2000:]


@pytest.mark.parametrize("macro,value", [(m, 3) for m in ST_MACROS] + [("MG_QUAD_ST_OBS", 1), ("MG_QUAD_ST_STATE", 32),
                                                                       ("MG_QUAD_LD_STATE", 16), ("MG_QUAD_LD_STATE", 1)])
def test_unknown_policy_is_a_compile_error(tmp_path, macro, value):
    r = _compile(tmp_path, "quadrotor.hip", {macro: value})
    assert r.returncode != 0
    assert "static assertion failed" in r.stderr and "policy" in r.stderr, r.stderr[-2000:]
