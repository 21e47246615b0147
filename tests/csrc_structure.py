"""How the bandits translation units get their shared code (helper of test_bandits_policy.py and test_bandits_learner.py)."""
import os
import re

from metagym_amd import build


def assert_unit_sits_on_the_bandits_core(unit):
    """The env's device functions come from the family's core header, for the env's own unit and for `unit` alike; no unit is
    cut by a macro; no .hip includes a .hip; the three walker units sit on walker_core.h; LiftSim's two policy units, and
    no other file, sit on liftsim_policy_core.h and keep no PolicyActions, walk or pad helper of their own."""
    text_of = {f: open(os.path.join(build.CSRC, f)).read() for f in sorted(os.listdir(build.CSRC))}
    assert '#include "bandits_core.h"' in text_of["bandits.hip"] and '#include "bandits_core.h"' in text_of[unit]
    assert not [f for f, t in text_of.items() if "MG_BANDITS_CORE_ONLY" in t]
    assert not [f for f, t in text_of.items() if "MG_WALKER_POLICY_ONLY" in t or "MG_WALKER_RPOLICY_ONLY" in t]
    assert all('#include "walker_core.h"' in text_of[f] for f in ("walker.hip", "walker_policy.hip", "walker_rpolicy.hip"))
    assert [(f, m) for f, t in text_of.items() for m in re.findall(r'#include\s+"([^"]*\.hip)"', t)] == []
    policy_units = ["liftsim_policy.hip", "liftsim_rpolicy.hip"]
    assert [f for f, t in text_of.items() if '#include "liftsim_policy_core.h"' in t] == policy_units
    assert not [f for f in policy_units if re.search(r"struct\s+PolicyActions\b|\b\w+_(walk|pad4)\s*\(", text_of[f])]
