"""Solve problems whose sort.Slice calls take the full pdqsort emulation at chosen slice lengths (csrc/kp_gosort.h: short
ranges finished in registers), shared by the CPU (oracle) and GPU (device) tests.

mixed(n): n NodeClaims of one big pod on 8-vCPU types, in creation order n/4 of 7-cpu pods (room for 2 small pods of
400m), n/4 of 6-cpu pods (room for 4; three=False: none of these) and the rest of 5-cpu pods (room for 7).  The small pods
fill the slice level by level.  A NodeClaim that is full keeps its key and stays at the front of the sorted slice, so
from level 3 on the element that gains a pod is the one at n/4 (n/2 with two groups), and from level 5 on the one at n/2,
each time with its run of the old level behind it.  n is chosen with n/2 == (n/4)*2 (and n % 4 == 0 with three groups):
those are centres of choosePivot's sample triples, the triple holds the inversion, the hint is not "increasing" and
every such sort is the full emulation, at slice length n.  13 <= n < 50 has no stable move at all (every inverted sort
is full).  `overflow` more small pods than the NodeClaims hold open one further NodeClaim (an append below the band's
upper end is a full sort too).

(The flagship's pod mix over small instance types, synth.config2 with both NodePools restricted to types of at most
2 vCPU, grows the slice to 277 NodeClaims with 1,500 pods but takes no full sort at all on the parent build, so it is not
a case here.)
"""
from dataclasses import dataclass

from kpsim import abi, model, synth
from kpsim.model import PodClass

import same_shape_cases as SC

SMALL = {"cpu": "400m", "memory": "64Mi"}
MIDDLE = {"cpu": "6", "memory": "1Gi"}


@dataclass
class Case:
    name: str
    problem: model.Problem
    n_nodeclaims: int   # what the oracle must give (asserted by the tests)
    passes: int         # the slice grows past this many NodeClaims (0: it never exceeds 64)
    preference_policy: int = abi.KP_PREFERENCE_RESPECT


def mixed(cat, n, overflow=0, passes=0, three=False):
    assert n // 2 == n // 4 * 2 and (not three or n % 4 == 0)
    g = [n // 4, n // 4, n - n // 2] if three else [n // 2, 0, n - n // 2]
    specs = [(0, SC.BIGGER)] * g[0] + [(0, MIDDLE)] * g[1] + [(0, SC.BIG)] * g[2]
    specs += [(1, SMALL)] * (2 * g[0] + 4 * g[1] + 7 * g[2] + overflow)
    prob = model.Problem(cat, [SC.pool(cat)], [PodClass(), PodClass(labels={"app": "small"})], synth.pods_from_specs(specs))
    return Case("mixed_N%d" % n, prob, n + (1 if overflow else 0), passes)


NAMES = ["mixed_N40", "mixed_N60", "mixed_N68", "mixed_N132", "mixed_N260", "mixed_N448"]  # 448: about where the flagship ends


def build(golden):
    """name -> Case, in a fixed order"""
    cases = [mixed(golden, 40, overflow=5), mixed(golden, 60), mixed(golden, 68, passes=64),
             mixed(golden, 132, passes=128, three=True), mixed(golden, 260, passes=256, three=True),
             mixed(golden, 448, passes=256, three=True)]
    assert [c.name for c in cases] == NAMES
    return {c.name: c for c in cases}
