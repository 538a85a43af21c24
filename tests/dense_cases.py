"""Node-dense Solve problems with unequal slice keys: more than KP_NC_FIRST = 4,096 in-flight NodeClaims whose pod counts
differ, so that sort.Slice finds an inversion after almost every commit and resolves it over thousands of positions.
Shared by the CPU (oracle) and GPU (device) tests; a generalisation of sort_ranges_cases.mixed.

Base shape: n = 4,100 big pods on the 8-vCPU NodePool of same_shape_cases.pool, one per NodeClaim, in three groups by
the room they leave for small pods of 400m; then m small pods of a second class, which fill the NodeClaims level by
level.  A NodeClaim that is full stays at the front of the sorted slice, so from the level at which the first group is
full the element that gains a pod sits at n/4 or n/2 — centres of choosePivot's sample triples — and those sorts are the
full pdqsort emulation at slice length n; the commits of the first level are stable moves over up to n positions.

Two sizes.  No first plan holds 4,100 NodeClaims, so kp_solve re-plans for every pod (NCcap = P):
  hbm  n/4 BIGGER (room 2), n/4 MIDDLE (room 4), n/2 BIG (room 7); m = 14,000, P = 18,100: the slice arrays of a plan
       for 18,100 NodeClaims do not fit LDS beside the fixed tables (9 B each) and live in HBM;
       4,100 NodeClaims of 3 / 4 / 5 pods (1,025 / 350 / 2,725).
  mid  n/4 TIGHT (room 1), n/2 BIGGER, n/4 MIDDLE; m = 7,400, P = 11,500: slices in LDS, allocatable table in HBM, quick-
       accept rows for the first lds_nq < n NodeClaims only; NodeClaims of 2 / 3 / 4 pods (1,025 / 2,850 / 225).
       (The hbm groups with about 5,900 small pods would give two levels only, 2 and 3 pods; three need m > 8,200 there,
       which is past the 12,000 pods the size allows.  Hence the group with room for one.  It is kept below every
       family's lds_nq (1,281 at the least among the topology families), so that NodeClaims with a quick-accept row
       take a second small pod: a topology pod is quick-accepted only on a NodeClaim whose zone an earlier small pod
       narrowed to one domain.)

Families: each layers one feature, so that the launcher selects the named instantiation (PORTS, PREF, RESV, TOPO bits):
  base             nothing
  pref             2,000 of the small pods (one run in creation order) prefer zone 1a.  The NodePool's cpu limit is what
                   the n NodeClaims take, so no small pod opens another; the big pods of the second and third group
                   require zone 1b.  The run starts 1,000 pods before the first group is full: 1,000 land there and
                   narrow their NodeClaim to 1a, 1,000 fail everywhere, are relaxed (Respect) and requeued at the back.
                   (hbm: the first group is TIGHT here too, so that it is full after one level.)
  resv             the catalog is synth.config5_catalog over the pool's three types (every one carries a reservation of
                   at most 20 instances) and the pool is open to reserved.  A NodeClaim open to reserved holds an
                   instance of every reservation that has one left; once all have run out no such NodeClaim can be
                   created (ReservedOfferingModeStrict), so only the first big pods, as many as the largest reservation
                   holds, are open to reserved and the others require on-demand.  The reservations run out one by one.
  topo             a self-selecting zonal spread (maxSkew 1, DoNotSchedule) on every small pod
  ports            2,000 of the small pods (every 3rd from the first) carry HostPort 80: one per NodeClaim.  Fewer than
                   the 3,584 at which the prepare's own node-dense estimate would plan past 4,096 without a re-plan.
  pref_resv_topo   resv + topo, and 200 of the small pods (every 20th) also prefer zone 1a: those whose spread admits
                   another zone only fail everywhere and are relaxed
  ports_resv_topo  resv + topo + the 2,000 port pods
Host ports reach the oracle as spare resource axes (hostport_cases.transform); the device solves the problem over the
catalog with those axes zeroed.

Oracle time of each case as it stands, one at a time on an otherwise idle 8-core development machine (s), hbm / mid:
base 6.4 / 4.4, pref 13.8 / 9.1, resv 8.8 / 6.0, topo 12.5 / 5.1, ports 6.7 / 4.5, pref_resv_topo 13.7 / 6.7,
ports_resv_topo 13.2 / 6.6.  (With compiles running beside them the same runs took up to 1.6 times as long.)
"""
from dataclasses import dataclass, field

import numpy as np

from kpsim import abi, model, synth
from kpsim.model import HostPort, PodClass, Requirement, TopologyTerm

import hostport_cases as HP
import same_shape_cases as SC
import sort_ranges_cases as SR

N = 4100
TIGHT = {"cpu": "7400m", "memory": "1Gi"}     # room for one small pod of 400m on 7,910m allocatable
SMALL = SR.SMALL
Z1A, Z1B = "test-zone-1a", "test-zone-1b"
GROUPS = {"hbm": [(SC.BIGGER, N // 4), (SR.MIDDLE, N // 4), (SC.BIG, N // 2)],
          "mid": [(TIGHT, N // 4), (SC.BIGGER, N // 2), (SR.MIDDLE, N // 4)]}
PREF_GROUPS = {"hbm": [(TIGHT, N // 4), (SR.MIDDLE, N // 4), (SC.BIG, N // 2)], "mid": GROUPS["mid"]}
M_SMALL = {"hbm": 14_000, "mid": 7_400}
P_RANGE = {"hbm": (18_000, 65_535), "mid": (4_097, 12_000)}
# The preference sub-classes.  pref: the 2,000 pods the design asks for (oracle 13.8 s, Solve kernel 566 ms at hbm).
# pref_resv_topo: 200, every 20th small pod.  Under the spread every relaxed pod first fails on all 4,100 NodeClaims
# through the topology path: with 2,000 (every 7th) the oracle takes 17.4 s but the Solve kernel 17.9 s on an MI355X
# (4.7 M evaluations), against 1.4 s with 200; a case is to stay below about 5 s of device time.
PREF_RUN, PREF_SPREAD, PREF_EVERY = 2000, 200, 20
PORT_PODS, PORT_EVERY = 2000, 3

# family -> the selection bits of kp_launch_ffd (Context.solve_plan): ports, pref, resv, topo.  The PORTS instantiations
# carry PREF themselves: their pref bit reads 0 unless a class has a preference.
FAMILIES = {
    "base": dict(ports=0, pref=0, resv=0, topo=0),
    "pref": dict(ports=0, pref=1, resv=0, topo=0),
    "resv": dict(ports=0, pref=0, resv=1, topo=0),
    "topo": dict(ports=0, pref=0, resv=0, topo=1),
    "ports": dict(ports=1, pref=0, resv=0, topo=0),
    "pref_resv_topo": dict(ports=0, pref=1, resv=1, topo=1),
    "ports_resv_topo": dict(ports=1, pref=0, resv=1, topo=1),
}
SIZES = ["hbm", "mid"]
NAMES = ["%s-%s" % (f, s) for f in FAMILIES for s in SIZES]


@dataclass
class Case:
    name: str
    family: str
    size: str
    problem: model.Problem           # what the device solves
    oracle_problem: model.Problem    # what the oracle solves (host ports: the transformed problem)
    n_nodeclaims: int
    bits: dict
    small: np.ndarray                # pod indices of the small pods
    sub: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int64))  # ... of the feature's sub-class
    preference_policy: int = abi.KP_PREFERENCE_RESPECT


class Catalogs:
    """The catalogs of the families, built once: golden; the pool's three types with reservations; each derived for
    host ports (device, oracle)."""

    def __init__(self, golden):
        self.golden = golden
        self.resv = synth.config5_catalog([golden[i] for i in SC.rows(golden)], n_default=2, n_block=1)
        assert all(any(o.capacity_type == "reserved" for o in it.offerings) for it in self.resv)
        # every NodeClaim open to reserved takes one instance of each reservation that has one left, and none can be
        # created once all are used up (ReservedOfferingModeStrict): as many big pods stay open to reserved
        self.resv_nodeclaims = max(o.reservation_capacity for it in self.resv for o in it.offerings
                                   if o.capacity_type == "reserved" and o.available)
        self._ports = {}

    def get(self, resv, ports):
        cat = self.resv if resv else self.golden
        if not ports:
            return cat, cat
        if resv not in self._ports:
            self._ports[resv] = HP.derive_catalogs(cat)
        return self._ports[resv]


def build(cats, family, size):
    bits = FAMILIES[family]
    limited = family == "pref"       # the cpu limit and the zone-1b big pods (see the module docstring)
    groups = (PREF_GROUPS if limited else GROUPS)[size]
    m = M_SMALL[size]
    dcat, ocat = cats.get(bits["resv"], bits["ports"])
    pool = SC.pool(dcat, ("reserved", "on-demand") if bits["resv"] else ("on-demand",))
    if limited:
        pool.limits_remaining = {"cpu": N * 8000}
    spread = [TopologyTerm("spread", model.ZONE, [Requirement("app", "In", ["small"])], max_skew=1)] if bits["topo"] else []
    lab = {"app": "small"}
    classes = [PodClass()]
    big_b = big_od = small = sub = 0
    if limited:
        big_b = len(classes)
        classes.append(PodClass(requirements=[Requirement(model.ZONE, "In", [Z1B])]))
    if bits["resv"]:
        big_od = len(classes)
        classes.append(PodClass(requirements=[Requirement(model.CAPACITY_TYPE, "In", ["on-demand"])]))
    small = len(classes)
    classes.append(PodClass(labels=lab, topology=spread))
    is_sub = np.zeros(m, bool)
    if bits["pref"]:
        sub = len(classes)
        classes.append(PodClass(labels=lab, topology=spread, preferred_terms=[(10, [Requirement(model.ZONE, "In", [Z1A])])]))
        if limited:
            is_sub[groups[0][1] - PREF_RUN // 2:groups[0][1] + PREF_RUN // 2] = True
        else:
            is_sub[::PREF_EVERY][:PREF_SPREAD] = True
    elif bits["ports"]:
        sub = len(classes)
        classes.append(PodClass(labels=lab, topology=spread, host_ports=[HostPort(80)]))
        is_sub[::PORT_EVERY][:PORT_PODS] = True
    specs = []
    for gi, (req, cnt) in enumerate(groups):
        specs += [(big_b if gi > 0 else 0, req)] * cnt
    if bits["resv"]:
        specs = [(0 if i < cats.resv_nodeclaims else big_od, req) for i, (_, req) in enumerate(specs)]
    specs += [(sub if s else small, SMALL) for s in is_sub]
    prob = model.Problem(dcat, [pool], classes, synth.pods_from_specs(specs))
    oprob = prob
    if bits["ports"]:
        prob = HP.device_problem(prob, dcat)
        oprob = HP.transform(prob, ocat)
    return Case("%s-%s" % (family, size), family, size, prob, oprob, N, bits, N + np.arange(m), N + np.flatnonzero(is_sub))


_ORACLE = {}


def run_oracle(case):
    """(Results, requirements) of the oracle, as parity.run_oracle gives them.  Computed once per case and process;
    nobody changes it."""
    if case.name not in _ORACLE:
        _ORACLE[case.name] = HP.run_oracle(case.oracle_problem, case.preference_policy)
    return _ORACLE[case.name]


def _zones(reqs):
    """per NodeClaim the zones its requirements admit (None: no zone requirement)"""
    return [q[model.ZONE][4] if model.ZONE in q and not q[model.ZONE][0] else None for q in reqs]


def check(case, res):
    """What the GPU tests rest on, from the oracle's result alone (test_dense_plans_cpu)."""
    r, reqs = res
    P = case.problem.pods.n
    lo, hi = P_RANGE[case.size]
    assert lo <= P <= hi, P
    assert r.n_nodeclaims == case.n_nodeclaims and r.n_nodeclaims > 4096
    assert not (r.pod_result == -1).any()
    vals, cnt = np.unique(r.nodeclaim_n_pods, return_counts=True)
    levels = [int(v) for v, c in zip(vals, cnt) if c * 20 >= r.n_nodeclaims]
    assert len(levels) >= 3, dict(zip(vals.tolist(), cnt.tolist()))   # unequal slice keys, each level on >= 5 %
    zones = _zones(reqs)
    if case.bits["pref"]:
        kept = np.array([zones[int(r.pod_result[p])] == (Z1A,) for p in case.sub])
        assert kept.any() and not kept.all(), int(kept.sum())
        assert int(r.stats["pods_popped"]) > P  # a relaxed pod is popped again
    if case.bits["resv"]:
        held = [model.RESERVATION_ID in q for q in reqs]
        assert any(held) and not all(held), sum(held)
    if case.bits["topo"]:
        z = [zones[int(r.pod_result[p])] for p in case.small]
        assert all(x is not None and len(x) == 1 for x in z)
        per = np.unique([x[0] for x in z], return_counts=True)[1]
        assert len(per) == 3 and per.max() - per.min() <= 1, per
    if case.bits["ports"]:
        on = np.bincount(r.pod_result[case.sub], minlength=r.n_nodeclaims)
        assert on.max() == 1 and len(case.sub) > 0
        HP.assert_no_conflict(case.problem, r)
