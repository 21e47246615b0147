#!/usr/bin/env python3
"""Kernel-by-kernel comparison of the gfx950 instruction streams of two trees (no GPU needed):

    scripts/isa_diff.py OTHER_TREE [unit.hip ...] [--keep DIR]

OTHER_TREE is a checkout of the commit to compare against (git worktree add --detach DIR REV). Every unit (default: the
five env families and their closed-loop units) is compiled device-only to assembly in both trees, each with its own
metagym_amd/build.py's flags for that file. A kernel's stream is the text between its label and its end label with
comments stripped, local labels renumbered in order of appearance and whitespace squeezed. One line per kernel:

    unit  identical | DIFFERS | removed (in OTHER_TREE only) | ADDED (here only)  lines of the stream  kernel

Exit status 1 when a kernel differs or was added. --keep DIR leaves the .s files there (DIR/other, DIR/here).
"""
import concurrent.futures
import importlib.util
import os
import re
import subprocess
import sys
import tempfile

UNITS = ["bandits.hip", "bandits_policy.hip", "bandits_learner.hip", "liftsim.hip", "liftsim_policy.hip",
         "liftsim_rpolicy.hip", "maze.hip", "maze_policy.hip", "maze_expert.hip", "maze3d_policy.hip", "quadrotor.hip",
         "quadrotor_tasks.hip", "quadrotor_policy.hip", "walker.hip", "walker_policy.hip", "walker_rpolicy.hip"]
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def recipe(side, tree):
    spec = importlib.util.spec_from_file_location("build_of_" + side, os.path.join(tree, "metagym_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def assemble(build, unit, out):
    cmd = [build.HIPCC] + build.COMPILE_FLAGS + build.FILE_FLAGS.get(unit, []) + \
          ["--cuda-device-only", "-S", os.path.join(build.CSRC, unit), "-o", out]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return out


def kernels(path):
    """{kernel symbol: normalised instruction stream} of one assembly file."""
    lines = open(path).read().split("\n")
    names = [ln.split()[1] for ln in lines if ln.strip().startswith(".amdhsa_kernel ")]
    out = {}
    for name in names:
        start = next(i for i, ln in enumerate(lines) if ln.startswith(name + ":"))
        body, labels = [], {}
        for ln in lines[start + 1:]:
            if ln.startswith(".Lfunc_end"):
                break
            ln = " ".join(ln.split(";")[0].split())
            if ln:
                body.append(ln)
        text = "\n".join(body)
        for lab in re.findall(r"\.L[A-Za-z_]+\d+(?:_\d+)?", text):
            labels.setdefault(lab, ".L%d" % len(labels))
        out[name] = re.sub(r"\.L[A-Za-z_]+\d+(?:_\d+)?", lambda m: labels[m.group(0)], text)
    return out


def demangle(names):
    if not names:
        return {}
    r = subprocess.run(["c++filt"] + list(names), capture_output=True, text=True)
    plain = r.stdout.split("\n") if r.returncode == 0 else list(names)
    return dict(zip(names, plain))


def main(argv):
    keep = None
    if "--keep" in argv:
        i = argv.index("--keep")
        keep = argv[i + 1]
        del argv[i:i + 2]
    if not argv:
        sys.exit(__doc__)
    other, units = os.path.abspath(argv[0]), argv[1:] or UNITS
    tmp = keep or tempfile.mkdtemp(prefix="isa_diff_")
    trees = {"other": recipe("other", other), "here": recipe("here", HERE)}
    for side in trees:
        os.makedirs(os.path.join(tmp, side), exist_ok=True)
    jobs = min(16, int(os.environ.get("MAX_JOBS") or os.cpu_count() or 4))   # compilers at once
    with concurrent.futures.ThreadPoolExecutor(max_workers=jobs) as pool:
        asm = {(side, u): pool.submit(assemble, trees[side], u, os.path.join(tmp, side, u[:-4] + ".s"))
               for side in trees for u in units}
        asm = {k: f.result() for k, f in asm.items()}
    bad = 0
    counts = {"identical": 0, "DIFFERS": 0, "removed": 0, "ADDED": 0}
    for u in units:
        a, b = kernels(asm["other", u]), kernels(asm["here", u])
        plain = demangle(sorted(set(a) | set(b)))
        for name in sorted(set(a) | set(b)):
            verdict = "removed" if name not in b else "ADDED" if name not in a else "identical" if a[name] == b[name] else "DIFFERS"
            counts[verdict] += 1
            bad += verdict in ("DIFFERS", "ADDED")
            short = plain[name].replace("(anonymous namespace)::", "").split("(")[0]
            print("%-22s %-10s %6d lines  %s" % (u, verdict, len((b.get(name) or a[name]).split("\n")), short[5:] if short.startswith("void ") else short))
    print("%d kernels: " % sum(counts.values()) + ", ".join("%d %s" % (v, k) for k, v in counts.items()))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
