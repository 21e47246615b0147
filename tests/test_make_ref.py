"""oracle/make_ref.py — the recipe that byte-compiles the unmodified reference into oracle/_ref for bench.py's `cpu_baseline`
leg (north_star: "the reference CPU path timed on the same box's host cores in the same run"). The recipe is exercised on a
stand-in tree the test writes itself, with every module and data file the recipe takes."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# A stand-in for the reference tree, written by the test itself: every module and data file the recipe takes (make_ref.MODULES /
# DATA) at its place, the quadrotor modules a small env that reads its config.json next to it and imports its simulator module,
# so that the byte-compiled copy has to resolve both the way the reference's own modules do.
STAND_IN = {
    "metagym/quadrotor/env.py": (
        "import json\n"
        "import os\n"
        "import numpy as np\n"
        "from metagym.quadrotor.quadrotorsim import QuadrotorSim\n\n\n"
        "class Quadrotor(object):\n"
        "    def __init__(self, task='no_collision', nt=1000):\n"
        "        with open(os.path.join(os.path.dirname(__file__), 'config.json')) as f:\n"
        "            self.sim = QuadrotorSim(json.load(f), nt)\n"
        "        self.task = task\n\n"
        "    def reset(self):\n"
        "        self.sim.reset(np.random.random_sample(4))\n\n"
        "    def step(self, action):\n"
        "        return self.sim.step(np.asarray(action, np.float32))\n"),
    "metagym/quadrotor/quadrotorsim.py": (
        "import numpy as np\n\n\n"
        "class QuadrotorSim(object):\n"
        "    def __init__(self, cfg, nt):\n"
        "        self.k, self.nt = float(cfg['thrust']['k']), nt\n\n"
        "    def reset(self, x):\n"
        "        self.x, self.t = x, 0\n\n"
        "    def step(self, a):\n"
        "        self.x = self.x + self.k * a\n"
        "        self.t += 1\n"
        "        return self.x.copy(), float(-np.dot(self.x, self.x)), self.t >= self.nt, {}\n"),
    "metagym/metamaze/envs/maze_task.py": (
        "import os\n"
        "IMAGES = sorted(os.listdir(os.path.join(os.path.dirname(__file__), 'img')))\n"),
}


def write_stand_in_reference(root):
    from PIL import Image
    from oracle import make_ref
    for rel in make_ref.MODULES:
        path = os.path.join(root, rel)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            f.write(STAND_IN.get(rel, ""))
    for i, rel in enumerate(make_ref.DATA):
        path = os.path.join(root, rel)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        if rel.endswith(".json"):
            with open(path, "w") as f:
                json.dump({"thrust": {"k": 0.125}, "unused": [1, 2, 3]}, f, indent=4)
        else:
            Image.new("RGB", (64, 64), (16 * i, 255 - 16 * i, 7)).save(path)


def test_recipe_builds_sourceless_reference_that_steps(tmp_path):
    from oracle import make_ref
    ref = str(tmp_path / "reference")
    write_stand_in_reference(ref)
    out = str(tmp_path / "_ref")
    m = make_ref.build(reference=ref, out=out, quiet=True)
    assert make_ref.usable(out)
    # nothing but byte-code, the data files the modules read, and the manifest: no reference .py travels
    for dirpath, _d, files in os.walk(out):
        for f in files:
            assert not f.endswith(".py"), f
    assert "metagym/quadrotor/env.py" in m["files"] and len(m["files"]["metagym/quadrotor/env.py"]["sha256_source"]) == 64
    assert sorted(m["files"]) == sorted(make_ref.MODULES + make_ref.DATA)
    code = ("import sys, numpy as np\n"
            "sys.path.insert(0, %r)\n"
            "from metagym.quadrotor.env import Quadrotor\n"
            "import metagym.quadrotor.env as e\n"
            "import metagym.metamaze.envs.maze_task as t\n"
            "assert e.__file__.endswith('env.pyc'), e.__file__\n"
            "assert len(t.IMAGES) == 9, t.IMAGES\n"
            "np.random.seed(3)\n"
            "env = Quadrotor(task='hovering_control', nt=1000); env.reset()\n"
            "o, r, d, i = env.step(np.array([2.0, 2.1, 2.2, 2.3], np.float32))\n"
            "print(repr(float(r)))\n") % (out,)
    got = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=str(tmp_path))
    assert got.returncode == 0, got.stderr
    # the same call against the sources where they lie: identical reward
    code_src = code.replace(repr(out), repr(ref)).replace("assert e.__file__.endswith('env.pyc'), e.__file__\n", "")
    want = subprocess.run([sys.executable, "-c", code_src], capture_output=True, text=True, cwd=str(tmp_path))
    assert want.returncode == 0, want.stderr
    assert got.stdout == want.stdout


def test_bench_reference_root_falls_back_to_the_built_copy(monkeypatch):
    import bench
    monkeypatch.delenv("METAGYM_REFERENCE", raising=False)
    assert bench.reference_root() == os.path.join(ROOT, "oracle", "_ref")
    monkeypatch.setenv("METAGYM_REFERENCE", "/somewhere/else")
    assert bench.reference_root() == "/somewhere/else"
    # an absent tree is reported, not an exception (the C port then stays the baseline, labelled as such)
    res, why = bench.cpu_reference(seconds=0.1)
    assert res is None and "no importable reference" in why


def test_bench_never_reads_the_reference_tree_at_run_time():
    src = open(os.path.join(ROOT, "bench.py")).read()
    assert '"/root/reference"' not in src and "'/root/reference'" not in src


def test_ref_dir_is_ignored_by_git_but_ships_to_the_gpu_box():
    assert "oracle/_ref/" in open(os.path.join(ROOT, ".gitignore")).read().split()
    p = os.path.join(ROOT, ".gpurunignore")
    assert not os.path.exists(p) or "_ref" not in open(p).read()
