"""How the bandits translation units get their shared code (helper of test_bandits_policy.py and test_bandits_learner.py)."""
import os
import re

from metagym_amd import build


def assert_unit_sits_on_the_bandits_core(unit):
    """The env's device functions come from the family's core header, for the env's own unit and for `unit` alike; no unit is
    cut by a macro; no .hip includes a .hip (the walker units, which select instantiations of walker.hip, aside)."""
    text_of = {f: open(os.path.join(build.CSRC, f)).read() for f in sorted(os.listdir(build.CSRC))}
    assert '#include "bandits_core.h"' in text_of["bandits.hip"] and '#include "bandits_core.h"' in text_of[unit]
    assert not [f for f, t in text_of.items() if "MG_BANDITS_CORE_ONLY" in t]
    assert [(f, m) for f, t in text_of.items() for m in re.findall(r'#include\s+"([^"]*\.hip)"', t)] == \
        [("walker_policy.hip", "walker.hip"), ("walker_rpolicy.hip", "walker.hip")]
