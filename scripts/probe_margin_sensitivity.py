"""How far ONE sub-step of the CPU oracle (oracle/abd.py) moves when its input state is perturbed by 0 - 2 ulp per entry — the
a1-like robot landing on the `special` stair course of tests/test_a1_physics_gpu.py::test_two_courses_in_one_batch_match_the_oracle,
with Bullet's relative contact margin and without. CPU only. The margin's candidate test (depth > -margin), the per-proxy
deepest-box choice and the PGS clamps are discrete decisions: next to one of them an ulp of input is amplified to 1e-7 in the
output (one sub-step in 220), which bounds what a GPU-vs-oracle comparison of single sub-steps can promise there.

    python scripts/probe_margin_sensitivity.py  >  profiles/r06/walker_margin_sensitivity.txt
"""
import os, sys, numpy as np, copy
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import abd
from urdf_fixture import A1_LIKE_TOES, a1_like_urdf
from metagym_amd.quadrupedal import load_urdf, MOTOR_NAMES
from metagym_amd.quadrupedal.terrain import upstair_terrain, task_terrain
from metagym_amd.metalocomotion.mjcf import contact_margins
m = load_urdf(a1_like_urdf(), foot_links=A1_LIKE_TOES, joint_order=MOTOR_NAMES)
m.sph_friction = np.where(np.asarray(m.sph_foot) >= 0, 1.0, m.sph_friction)
def ob(spec):
    out = []
    for half, pos, (x, y, z, w), mu in spec:
        nq = np.sqrt(x*x+y*y+z*z+w*w); x, y, z, w = x/nq, y/nq, z/nq, w/nq
        R = np.array([[1-2*(y*y+z*z), 2*(x*y-w*z), 2*(x*z+w*y)], [2*(x*y+w*z), 1-2*(x*x+z*z), 2*(y*z-w*x)], [2*(x*z-w*y), 2*(y*z+w*x), 1-2*(x*x+y*y)]])
        out.append((np.array(pos, float), R, np.array(half, float), float(mu)))
    return out
h_b, _, boxes_b = upstair_terrain(stepwidth=0.3, slope=0.34, stepheight=0.07, mode="special",
                                  env_vecs=[[0, 0, 1, 0, 0, 0.08, 0.25], [0, 1, 0, 0, 0.34, 0, 0], [0, 0, 0, 0, 0, 0, 0]] * 3)
for margin_rule in ("relative", 0.0):
    prm = abd.Params(contact_margin=contact_margins(m, margin_rule), dt=0.002, substeps=1, iterations=23, erp=0.2, friction=5.0, sphere_friction=m.sph_friction,
                     self_collision=False, gravity=10.0, terrain=ob(boxes_b), max_velocity=100.0)
    s = abd.State(m)
    s.pos = np.array([2.2, 0.0, 0.28 + h_b + 0.3]) + np.asarray(m.body_pos[0]) * 0
    s.q = np.array([0, 0.9, -1.8] * 4, float)
    target = np.array([0, 0.9, -1.8] * 4, float)
    rs = np.random.RandomState(1); rp = np.random.RandomState(9)
    worst = []
    for t in range(220):
        tau = np.clip(80.0 * (target - s.q) - 1.5 * s.qd + rs.uniform(-2, 2, 12), -33.5, 33.5)
        s2 = s.copy()
        for name in ("pos", "v", "w", "q", "qd"):
            a = getattr(s2, name); setattr(s2, name, a * (1.0 + 2.2e-16 * rp.randint(-2, 3, a.shape)))
        out = {}
        abd.substep(m, s, tau, prm, out=out)
        abd.substep(m, s2, tau, prm)
        d = max(np.abs(s.q - s2.q).max(), np.abs(s.qd - s2.qd).max(), np.abs(s.pos - s2.pos).max(), np.abs(s.v - s2.v).max(), np.abs(s.w - s2.w).max())
        worst.append((d, t, len(out["rows"])))
    worst.sort(reverse=True)
    print(margin_rule, [("%.1e" % a, b, c) for a, b, c in worst[:6]])
