#!/usr/bin/env python3
"""Golden data the MetaLocomotion tests read in place of the reference tree, recorded from the UNMODIFIED reference.

TEST INFRASTRUCTURE; runs only where the reference tree is present ($METAGYM_REFERENCE, same default as the other generators):

    python oracle/gen_golden_walker_world.py

Writes two files under tests/golden/:

  walker_assets.tar.xz   the shipped MJCF robot files the walker tests sample (metalocomotion/envs/assets/{humanoids,ants}:
                         every 16th file of the sorted listing, every 7th body variant, and the two base robots) plus
                         `listing.json`, the full sorted listing of both directories. Data only: the generator scripts
                         that also lie there are not taken.
  walker_world.json      what the unmodified Scene / StadiumScene / env code (scene_bases.py:52-56, stadium.py:19-25,
                         env_bases.py:47-48) tells the PyBullet stand-in (oracle/refstubs/pybullet) for meta-humanoid-v0
                         and meta-ant-v0 on their base robots: gravity, contact ERP, time step, sub-steps, solver
                         iterations, and the lateral friction of every floor body.

tests/test_walker_rules.py and tests/test_walker_variants.py read them.
"""
import io
import json
import os
import sys
import tarfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = os.environ.get("METAGYM_REFERENCE", "/root/reference")
ASSETS = os.path.join(REF, "metagym", "metalocomotion", "envs", "assets")
OUT_ASSETS = os.path.join(ROOT, "tests", "golden", "walker_assets.tar.xz")
OUT_WORLD = os.path.join(ROOT, "tests", "golden", "walker_world.json")
ROBOTS = (("humanoid", "humanoids"), ("ant", "ants"))


def sampled(robot, listing):
    """The files the tests open: what test_parser_joint_order_is_what_addToScene_enumerates takes (every 16th of the sorted
    listing) and what test_variants_equal_the_reference_files_array_for_array takes (every 7th body variant), base robot included."""
    variants = [f for f in listing if f.startswith(robot + "_var_")]
    return sorted(set(listing[::16]) | set(variants[::7]) | {robot + ".xml"})


def record_assets():
    listing, members = {}, []
    for robot, sub in ROBOTS:
        listing[sub] = sorted(f for f in os.listdir(os.path.join(ASSETS, sub)) if f.endswith(".xml"))
        members += [(sub + "/" + f, open(os.path.join(ASSETS, sub, f), "rb").read()) for f in sampled(robot, listing[sub])]
    members.append(("listing.json", json.dumps(listing, indent=1).encode()))
    with tarfile.open(OUT_ASSETS, "w:xz", preset=9) as tar:
        for name, data in members:
            info = tarfile.TarInfo(name)          # fixed metadata: the archive is a function of the files alone
            info.size, info.mode, info.mtime = len(data), 0o644, 0
            tar.addfile(info, io.BytesIO(data))
    print("wrote", OUT_ASSETS, len(members) - 1, "robot files,", os.path.getsize(OUT_ASSETS), "bytes")


def record_world():
    for p in (ROOT, os.path.join(HERE, "refstubs"), REF):
        if p not in sys.path:
            sys.path.insert(0, p)
    np.int = int
    import gym
    import metagym.metalocomotion  # noqa: F401
    out = {}
    for env_id, task in (("meta-humanoid-v0", "humanoid.xml"), ("meta-ant-v0", "ant.xml")):
        env = gym.make(env_id, enable_render=False)
        env.set_task(task)
        env.reset()
        w = env._p._world
        out[env_id] = {"task": task, "gravity": w.gravity, "contact_erp": w.contact_erp, "sub_steps": w.sub_steps,
                       "fixed_time_step": w.fixed_time_step, "solver_iterations": w.solver_iterations,
                       "floor_frictions": [b.friction for b in w.bodies if type(b).__name__ == "_Floor"]}
    with open(OUT_WORLD, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", OUT_WORLD)


def main():
    if not os.path.isdir(ASSETS):
        raise SystemExit("no reference tree at %s (set METAGYM_REFERENCE)" % REF)
    record_assets()
    record_world()


if __name__ == "__main__":
    main()
