"""Solve problems about the headroom bound's rows and its gather at the hand-off (DESIGN.md §4 "Headroom bound"), shared
by tests/test_bound_rows_cpu.py, tests/test_gpu_bound_rows.py and tests/test_gpu_bound_lazy.py.  They build on
tests/headroom_bound_cases.py (HC) and its NodePools.

Rows.  The NodePool has a cpu-rich and a memory-rich type (HC.LOOSE_TYPES: 16 vCPU / 32 GiB and 8 vCPU / 64 GiB).  G pods
of 5 cpu / 20 GiB open G NodeClaims that keep both options (a second such pod passes each axis but fits no single type,
as HC.loose).  Then G pods of 2 cpu whose class carries an instance-type requirement land one per NodeClaim (the slice is
sorted by len(Pods), so each goes to a NodeClaim that still holds one pod); then M pods of 1.5 cpu without requirements.
* narrowed: the requirement is In [the memory-rich type].  Every accepted Add removes the cpu axis' largest type: the
  row's cpu maximum falls from 16 vCPU's allocatable to 8 vCPU's, and 7 + 1.5 cpu, which passes the old maximum, exceeds
  the new one.  The first 1.5-cpu pod is therefore rejected by all G NodeClaims on the bound alone: G skips exactly (the
  later ones find them marked), and the M pods share one new NodeClaim.
* kept: the requirement is In [both types].  The Add runs in full (the class is not absorbed) and removes nothing: the
  rows stay as they are, 8.5 cpu and 22 GiB fit the cpu-rich type, and nothing is skipped.

Hand-off.  disjoint(F, G): a second NodePool holds the 16-vCPU type alone and a first pod of 13 cpu, whose class requires
that type, opens its NodeClaim R at the head of the slice.  Then HC.not_absorbed's F full and G open NodeClaims and its
2-cpu pods, whose class requires the three 8-vCPU types: R has room for 2 cpu (its witness covers the pod) and rejects
it on requirements, the F NodeClaims behind it are full.  The first 2-cpu pod skips F exactly: for F = 7 they fill R's
round of 8, for F = 8 the last one opens the next round beside the open NodeClaims, for F = 9 and G = 0 the next round
holds full ones alone.

Skips of the pods that open the NodeClaims (as HC.at_bound counts them): a pod whose shape was rejected before finds the
earlier NodeClaims marked in the shape's memo and the newest one not, and the bound rejects that one (7 + 7 or 5 + 5 cpu
exceeds 8 vCPU's allocatable).  So n one-per-NodeClaim pods of a shape skip n - 1, and the first pod of a new shape
skips every NodeClaim it cannot join: the first 7-cpu pod skips R (13 + 7 exceeds 16 vCPU's), the first 5-cpu pod R and
the F full ones.  disjoint(F, G) in all: F (7-cpu pods) + 1 + F + G - 1 (5-cpu pods, G > 0) + F (the first 2-cpu pod);
HC.not_absorbed(0) and HC.absorbed(0): G - 1 = 2.  The openers of the row cases pass the bound on each axis (10 cpu,
40 GiB) and are evaluated: none.
"""
from kpsim import model, synth
from kpsim.model import PodClass, Requirement

import headroom_bound_cases as HC
from headroom_bound_cases import Case

OPENER = {"cpu": "5", "memory": "20Gi"}
NARROW = {"cpu": "2", "memory": "1Gi"}
TAIL = {"cpu": "1500m", "memory": "1Gi"}
CPU_RICH, MEM_RICH = HC.LOOSE_TYPES


def _rows_problem(cat, g, m, types):
    specs = [(0, OPENER)] * g + [(1, NARROW)] * g + [(2, TAIL)] * m
    pool = synth.default_nodepool(instance_types=HC.SC.rows(cat, HC.LOOSE_TYPES))
    classes = [PodClass(), PodClass(labels={"app": "narrow"}, requirements=[Requirement(model.INSTANCE_TYPE, "In", types)]),
               PodClass(labels={"app": "tail"})]
    return model.Problem(cat, [pool], classes, synth.pods_from_specs(specs))


def narrowed(cat, g, m=3):
    return Case("narrowed_G%d" % g, _rows_problem(cat, g, m, [MEM_RICH]), g + 1, g, skips=g)


def kept(cat, g, m=3):
    return Case("kept_G%d" % g, _rows_problem(cat, g, m, [CPU_RICH, MEM_RICH]), g, 0, skips=0)


def disjoint(cat, f, g, m=3):
    specs = [(2, {"cpu": "13", "memory": "1Gi"})] + [(0, HC.FULL)] * f + [(0, HC.OPEN)] * g + [(1, HC.MED)] * m
    first = synth.default_nodepool(name="small", instance_types=HC.SC.rows(cat))
    first.weight = 10
    second = synth.default_nodepool(name="large", instance_types=HC.SC.rows(cat, [CPU_RICH]))
    classes = [PodClass(), PodClass(labels={"app": "med"}, requirements=[Requirement(model.INSTANCE_TYPE, "In", HC.SC.TYPES)]),
               PodClass(labels={"app": "large"}, requirements=[Requirement(model.INSTANCE_TYPE, "In", [CPU_RICH])])]
    prob = model.Problem(cat, [first, second], classes, synth.pods_from_specs(specs))
    return Case("disjoint_F%d_G%d" % (f, g), prob, 1 + f + (g if g else 1), f, skips=2 * f + (f + g if g else 0))


def rank_position(cat, res, pos):
    """the catalog row at position pos of the host's rank table of axis res: the types by allocatable, largest first,
    equal values in type order (std::stable_sort in the prepare's rank-table stage; Python's sort is stable too)"""
    a = [int(it.allocatable[model.RIDX[res]]) for it in cat]
    return sorted(range(len(cat)), key=lambda t: -a[t])[pos]


# rank positions on both sides of the walk's first step edge (64 ranks per step) and the first of the last step of the
# 918-type catalog (padded to 960: ranks 896 ..)
EDGES = {"r63": 63, "r64": 64, "last": 896}


def rank_edge(cat, res, edge, above, f=3, m=2):
    """A NodePool of the one type at rank position EDGES[edge] of axis res: a NodeClaim being created finds its option
    on that axis in the last lane of the first rank step, the first lane of the second, or only in the last step (the
    other axes wherever the type ranks there), and the row must hold that type's allocatable exactly.  HC.at_bound's
    construction on it: F pods leave exactly X on res, the small pods request X (each fits: nothing may be rejected for
    it, F - 1 skips among the big pods themselves) or one milli-unit more (2 F - 1 skips, one new NodeClaim)."""
    t = rank_position(cat, res, EDGES[edge])
    alloc = int(cat[t].allocatable[model.RIDX[res]])
    x = 100 if res == "cpu" else (64 << 20) * 1000
    big = {"cpu": "100m", "memory": "64Mi"}
    small = {"cpu": "10m", "memory": "16Mi"}
    pods = synth.pods_from_specs([(0, big)] * f + [(1, small)] * m)
    HC._set(pods, pods.class_id == 0, res, alloc - x)
    HC._set(pods, pods.class_id == 1, res, x + (1 if above else 0))
    pool = synth.default_nodepool(instance_types=[t])
    prob = model.Problem(cat, [pool], [PodClass(), PodClass(labels={"app": "small"})], pods)
    return Case("%s_%s_%s" % (res, edge, "above" if above else "at"), prob, f + (1 if above else 0), f - 1,
                skips=2 * f - 1 if above else f - 1)


STAT_FIELDS = ("pods_popped", "nodeclaim_evals", "nodeclaim_candidates_scanned", "template_evals",
                                "existing_evals", "sorts_fast", "sorts_full")
# kp_last_kernel_times: the counters that are always exact (kpsim.h): evaluation calls, quick accepts, slow-path pods,
# witness misses, topology quick accepts, failed evaluations by stage (merge, topology, no type left, minValues), bound skips
EXACT = (16, 17, 18, 19, 35, 38, 39, 40, 41, 49)


def observe(ctx, result):
    """the always-on statistics of the last solve on ctx: STAT_FIELDS of kp_solve_stats, then EXACT"""
    import ctypes as C
    a = (C.c_double * 52)()
    ctx.check(ctx.L.kp_last_kernel_times(ctx.h, a, len(a)), "kp_last_kernel_times")
    return tuple(int(result.stats[f]) for f in STAT_FIELDS) + tuple(int(a[i]) for i in EXACT)


# case -> observe() of a build of the parent commit (PARENT_COMMIT; tools/build_commit.sh builds it, KPSIM_LIB selects
# it) on these same inputs, never of the build under test.  "narrowed_then_kept": kept_G3 solved on the context that
# has just solved narrowed_G3.
PARENT_COMMIT = "cdbf214"
PARENT = {
    "narrowed_G3": (9, 8, 23, 4, 0, 1, 0, 3, 2, 7, 2, 0, 0, 0, 0, 0, 3),
    "narrowed_then_kept": (9, 5, 21, 3, 0, 2, 0, 3, 3, 6, 2, 0, 0, 0, 0, 0, 0),
    "narrowed_G9": (21, 26, 146, 10, 0, 1, 0, 9, 2, 19, 8, 0, 0, 0, 0, 0, 9),
    "kept_G3": (9, 5, 21, 3, 0, 2, 0, 3, 3, 6, 2, 0, 0, 0, 0, 0, 0),
    "kept_G9": (21, 17, 144, 9, 0, 2, 0, 9, 3, 18, 8, 0, 0, 0, 0, 0, 0),
    "not_absorbed_F0": (6, 5, 12, 3, 0, 0, 0, 3, 0, 6, 0, 0, 0, 0, 0, 0, 2),
    "disjoint_F7_G3": (14, 30, 88, 12, 0, 0, 0, 6, 0, 14, 0, 0, 1, 0, 0, 0, 24),
    "disjoint_F8_G3": (15, 33, 102, 13, 0, 0, 0, 6, 0, 15, 0, 0, 1, 0, 0, 0, 27),
    "disjoint_F9_G0": (13, 19, 77, 12, 0, 0, 0, 1, 2, 11, 0, 0, 1, 0, 0, 0, 18),
    "absorbed_F0": (6, 2, 12, 3, 0, 2, 0, 0, 3, 3, 0, 0, 0, 0, 0, 0, 2),
    "cpu_r63_above": (5, 5, 10, 4, 0, 0, 0, 0, 1, 4, 0, 0, 0, 0, 0, 0, 5),
    "cpu_r64_above": (5, 5, 10, 4, 0, 0, 0, 0, 1, 4, 0, 0, 0, 0, 0, 0, 5),
    "cpu_last_above": (5, 5, 10, 4, 0, 0, 0, 0, 1, 4, 0, 0, 0, 0, 0, 0, 5),
    "memory_r63_above": (5, 5, 10, 4, 0, 0, 0, 0, 1, 4, 0, 0, 0, 0, 0, 0, 5),
    "memory_r64_above": (5, 5, 10, 4, 0, 0, 0, 0, 1, 4, 0, 0, 0, 0, 0, 0, 5),
    "memory_last_above": (5, 5, 10, 4, 0, 0, 0, 0, 1, 4, 0, 0, 0, 0, 0, 0, 5),
    "cpu_r64_at": (5, 2, 9, 3, 0, 1, 0, 0, 2, 3, 0, 0, 0, 0, 0, 0, 2),
    "memory_r64_at": (5, 2, 9, 3, 0, 1, 0, 0, 2, 3, 0, 0, 0, 0, 0, 0, 2),
    # the same inputs with KPSIM_NO_TEAM_FIRST=1 (no first candidate is evaluated by the block)
    "not_absorbed_F0@no_team_first": (6, 10, 12, 3, 0, 0, 0, 6, 0, 6, 0, 0, 0, 0, 0, 0, 4),
    "disjoint_F7_G3@no_team_first": (14, 33, 88, 22, 0, 0, 0, 7, 0, 14, 0, 0, 1, 0, 0, 0, 26),
    "disjoint_F9_G0@no_team_first": (13, 19, 77, 22, 0, 0, 0, 1, 2, 11, 0, 0, 1, 0, 0, 0, 18),
}

ROWS = ["narrowed_G3", "narrowed_G9", "kept_G3", "kept_G9"]
LAZY = ["not_absorbed_F0", "disjoint_F7_G3", "disjoint_F8_G3", "disjoint_F9_G0", "absorbed_F0"]
RANKS = (["%s_%s_above" % (res, e) for res in ("cpu", "memory") for e in EDGES] + ["cpu_r64_at", "memory_r64_at"])
NO_TEAM_FIRST = ["not_absorbed_F0", "disjoint_F7_G3", "disjoint_F9_G0"]  # also solved with the block's first evaluation off
NAMES = ROWS + LAZY + RANKS


def build(golden):
    """name -> Case, in a fixed order"""
    cases = [narrowed(golden, 3), narrowed(golden, 9), kept(golden, 3), kept(golden, 9)]
    first = HC.not_absorbed(golden, 0)   # the first candidate has room, is not absorbed and accepts
    first.skips = 2
    fits = HC.absorbed(golden, 0)        # an absorbed first candidate: fits-only, not evaluated by the block
    fits.skips = 2
    cases += [first, disjoint(golden, 7, 3), disjoint(golden, 8, 3), disjoint(golden, 9, 0), fits]
    cases += [rank_edge(golden, res, e, True) for res in ("cpu", "memory") for e in EDGES]
    cases += [rank_edge(golden, "cpu", "r64", False), rank_edge(golden, "memory", "r64", False)]
    assert [c.name for c in cases] == NAMES
    return {c.name: c for c in cases}
