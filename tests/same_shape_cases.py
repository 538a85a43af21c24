"""Solve problems in which runs of same-shape pods walk the NodeClaim slice level by level (wave 0's same-shape inner
loop), shared by the CPU (oracle) and GPU (device) tests.

Construction: B big pods, each too large to share a NodeClaim of the NodePool's 8-vCPU types, give exactly N = B
NodeClaims of one pod.  M small pods of one shape follow them in the queue (smaller cpu request), of a class without
requirement keys that tolerates the template: each quick-accepts on the first NodeClaim of the slice sorted by
len(Pods), which then moves to the end of its run, so the small pods fill level 1 -> 2 across all N NodeClaims, then
2 -> 3, and so on.  Every case names its N; the tests assert it and that every pod is placed on the oracle's result.
"""
from dataclasses import dataclass

import numpy as np

from kpsim import abi, model, synth
from kpsim.model import INSTANCE_TYPE, PodClass, Requirement

TYPES = ["m5.2xlarge", "c5.2xlarge", "r5.2xlarge"]  # 8 vCPU each: a 5-cpu pod has no room for a second one
BIG = {"cpu": "5", "memory": "1Gi"}
BIGGER = {"cpu": "7", "memory": "1Gi"}             # leaves room for 9 small pods, BIG for 29
SMALL = {"cpu": "100m", "memory": "64Mi"}


@dataclass
class Case:
    name: str
    problem: model.Problem
    n_nodeclaims: int
    preference_policy: int = abi.KP_PREFERENCE_RESPECT


def rows(cat, names=TYPES):
    by = {it.name: i for i, it in enumerate(cat)}
    return [by[n] for n in names]


def pool(cat, capacity_types=("on-demand",)):
    return synth.default_nodepool(capacity_types=capacity_types, instance_types=rows(cat))


def small_levels(n, levels, extra=0):
    """small pods that fill `levels` whole levels of n NodeClaims and `extra` NodeClaims of the next one"""
    return n * levels + extra


def walk(cat, n, m, name=None):
    """n NodeClaims of one big pod, then m small pods of one shape"""
    specs = [(0, BIG)] * n + [(1, SMALL)] * m
    prob = model.Problem(cat, [pool(cat)], [PodClass(), PodClass(labels={"app": "small"})], synth.pods_from_specs(specs))
    return Case(name or "walk_N%d_M%d" % (n, m), prob, n)


def alternating(cat, n):
    """two small shapes of equal cpu and memory (the queue orders them by creation time), in runs of 7 and 5 and, for
    the second half, as a third shape of the first class (another ephemeral-storage request): a shape change falls in
    the middle of a level"""
    specs = [(0, BIG)] * n
    for i in range(3 * n + 7):
        specs.append((1, SMALL) if i % 12 < 7 else (2, SMALL))
    for i in range(2 * n + 3):
        specs.append((1, dict(SMALL, **{"ephemeral-storage": "1Gi"})) if i % 3 else (2, SMALL))
    classes = [PodClass(), PodClass(labels={"app": "a"}), PodClass(labels={"app": "b"})]
    return Case("alternating_shapes_N%d" % n, model.Problem(cat, [pool(cat)], classes, synth.pods_from_specs(specs)), n)


def witness_fails(cat, n, existing=0):
    """half of the NodeClaims hold a 7-cpu pod and stop fitting the small shape after 9 of them, while the others go on
    to 29: from level 10 on the witness fails inside an episode and rejected elements sit inside the runs.
    existing > 0: that many existing nodes with room for 5 small pods each take the first of them (xstart < E)."""
    specs = [(0, BIGGER)] * (n // 2) + [(0, BIG)] * (n - n // 2) + [(1, SMALL)] * (n * 9 + (n - n // 2) * 6 + 3 + 5 * existing)
    nodes = []
    for j in range(existing):
        it = cat[rows(cat)[0]]
        avail = np.zeros(model.R, np.int64)
        avail[model.RIDX["cpu"]] = 550
        avail[model.RIDX["memory"]] = 8 << 40
        avail[model.RIDX["pods"]] = 100_000
        nodes.append(model.ExistingNode("node-%d" % j, synth.node_labels(it, "test-zone-1a", "on-demand", "default"), avail))
    prob = model.Problem(cat, [pool(cat)], [PodClass(), PodClass(labels={"app": "small"})], synth.pods_from_specs(specs),
                         nodes)
    return Case("witness_fails_N%d_E%d" % (n, existing), prob, n)


def requeued(cat, n):
    """PREF: some of the small pods carry a preferred term no type satisfies: each fails once, is relaxed and pushed to
    the back of the queue (Queue.Push(pod, relaxed) clears every lastLen), and walks the slice with the plain small pods
    when its turn comes again"""
    specs = [(0, BIG)] * n
    for i in range(3 * n + 5):
        specs.append((2, SMALL) if i % 9 == 4 else (1, SMALL))
    classes = [PodClass(), PodClass(labels={"app": "small"}),
               PodClass(labels={"app": "small"}, preferred_terms=[(10, [Requirement(INSTANCE_TYPE, "In", ["no-such-type"])])])]
    return Case("pref_requeued_N%d" % n, model.Problem(cat, [pool(cat)], classes, synth.pods_from_specs(specs)), n)


def reserved(cat5, n):
    """RESV: the catalog carries reserved offerings and the NodePool is open to them"""
    specs = [(0, BIG)] * n + [(1, SMALL)] * (4 * n + 5)
    np_ = pool(cat5, ("reserved", "on-demand", "spot"))
    assert any(o.capacity_type == "reserved" for it in cat5 for o in it.offerings)
    prob = model.Problem(cat5, [np_], [PodClass(), PodClass(labels={"app": "small"})], synth.pods_from_specs(specs))
    return Case("reserved_N%d" % n, prob, n)


NS = [1, 12, 13, 49, 50, 64, 65, 130]     # pdqsort's insertion-sort bound, the band without a stable move, the pivot-
                                          # sample rule (n >= 50), the 64-lane slice-window edges, three windows
MS = [1, 2, 63, 64, 65, 129]              # at N = 65: the 64-entry queue window refilled inside an episode
SPECIAL_NS = [12, 56]                     # the other constructions: on both sides of the band without a stable move
NAMES = (["walk_N%d" % n for n in NS] + ["walk_N65_M%d" % m for m in MS] +
         [f % n for n in SPECIAL_NS for f in ("alternating_shapes_N%d", "witness_fails_N%d_E0", "witness_fails_N%d_E3",
                                              "pref_requeued_N%d", "reserved_N%d")])


def build(golden):
    """name -> Case, in a fixed order"""
    cat5 = synth.config5_catalog(golden)
    cases = [walk(golden, n, small_levels(n, 3, (n + 1) // 2) if n > 1 else 20, "walk_N%d" % n) for n in NS]
    cases += [walk(golden, 65, m, "walk_N65_M%d" % m) for m in MS]
    for n in SPECIAL_NS:
        cases += [alternating(golden, n), witness_fails(golden, n), witness_fails(golden, n, existing=3),
                  requeued(golden, n), reserved(cat5, n)]
    assert [c.name for c in cases] == NAMES
    return {c.name: c for c in cases}
