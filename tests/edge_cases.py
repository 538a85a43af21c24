"""Inputs at the edges of the 64-bit mask words (tests/test_gpu_word_edges.py, tests/test_word_edges_cpu.py): catalogs
with 32 x 2, 64 x 1 and 63 x 1 (zone, capacity-type) slots, problems rewritten into the upper half of the zone list,
catalogs of 1..129 types, launch requests whose draws clamp to the catalog, and the hand KATs whose expectations are
computed here in plain Python / numpy from the InstanceType / Offering objects (never from the oracle)."""
import copy
import hashlib

import numpy as np

import fuzzgen
import parity
from kpsim import catalog as kcat
from kpsim import model, synth
from kpsim.model import CAPACITY_TYPE, INSTANCE_TYPE, ZONE, Requirement

FOREIGN_ZONE = "us-west-2z"   # the zone value no catalog has (fuzzgen's)
FAMILY = "karpenter.k8s.aws/instance-family"


def sample(golden, n_types, seed):
    """a seeded subsample of n_types catalog rows, in catalog order (as the fuzz tests of the suite draw theirs)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    return [golden[int(i)] for i in sorted(rng.choice(len(golden), size=n_types, replace=False))]


def fuzz_default_digests(golden):
    """{family: [digest per seed 0-3]} of the fuzz generators' default (three-zone) path, through the oracle."""
    out = {}
    sub = sample(golden, 160, 4242)
    fams = {
        "fuzz_problem": lambda s: fuzzgen.fuzz_problem(sub, s, n_pods=200),
        "fuzz_topology_problem": lambda s: fuzzgen.fuzz_topology_problem(sub, s, n_pods=150),
        "fuzz_topology_existing_problem": lambda s: fuzzgen.fuzz_topology_existing_problem(sub, s, n_pods=150),
    }
    for name, gen in fams.items():
        out[name] = [parity.result_digest(parity.run_oracle(gen(s))) for s in range(4)]
    out["fuzz_consolidation"] = []
    for s in range(4):
        cp = fuzzgen.fuzz_consolidation(sub, s, n_nodes=30, n_pods=150)
        d = parity.result_digest(parity.run_oracle(cp.cluster))
        h = hashlib.sha256()
        for c in cp.candidates:
            h.update(repr((c.node, [int(p) for p in c.pods], float(c.price), int(c.capacity_type), int(c.instance_type),
                           int(c.nodepool))).encode())
        h.update(np.ascontiguousarray(cp.pending, np.int64).tobytes())
        h.update(repr([sorted(n.labels.items()) for n in cp.cluster.existing]).encode())
        d["candidates"] = h.hexdigest()
        out["fuzz_consolidation"].append(d)
    return out


# ------------------------------------------------------------------------------------------------
# catalogs
# ------------------------------------------------------------------------------------------------
def zone_names(n):
    """test-zone-1a, 1b, 1c (the suite's three), then 2a, 2b, ... : n distinct zones"""
    return ["test-zone-%d%s" % (1 + i // 3, "abc"[i % 3]) for i in range(n)]


def zone_ids(n):
    return ["use1-az1", "use1-az2", "use1-az4"][:n] + ["use1-az%d" % (i + 2) for i in range(3, n)]


def zoned_catalog(fx, n_zones, capacity_types=("on-demand", "spot"), n_types=160, seed=0):
    """The golden catalog over n_zones zones, a seeded subsample of n_types rows.  One capacity type: the other type's
    offerings are dropped and the capacity-type label lists that type alone, so the catalog has n_zones x 1 slots."""
    cat = sample(kcat.golden_catalog(zones=tuple(zone_names(n_zones)), zone_ids=tuple(zone_ids(n_zones)), fx=fx),
                 n_types, seed)
    cts = list(capacity_types)
    if len(cts) == 1:
        for it in cat:
            it.offerings = [o for o in it.offerings if o.capacity_type == cts[0]]
            it.labels[CAPACITY_TYPE] = list(cts)
    return cat


CATALOGS = {"Z32x2": (32, ("on-demand", "spot")),   # 64 slots, zone bits 0..31
            "Z64x1": (64, ("on-demand",)),          # 64 slots, zone bit 63
            "Z63x1": (63, ("on-demand",))}          # 63 zones: one foreign pod zone value fills the dictionary to 64
NAMES = list(CATALOGS)


def named_catalog(fx, name):
    nz, cts = CATALOGS[name]
    return zoned_catalog(fx, nz, cts, 160, seed=sum(map(ord, name)))


def slots(cat):
    """(zone, capacity type) of every offering slot in the device's order: zones, then capacity types, each in order
    of first appearance over the catalog's offerings; slot = zone index x number of capacity types + type index."""
    zs, cs = [], []
    for it in cat:
        for o in it.offerings:
            if o.capacity_type == "reserved":
                continue
            if o.zone not in zs:
                zs.append(o.zone)
            if o.capacity_type not in cs:
                cs.append(o.capacity_type)
    return [(z, c) for z in zs for c in cs]


def zones_of(cat):
    out = []
    for z, _ in slots(cat):
        if z not in out:
            out.append(z)
    return out


def offering_row(cat, t, zone, ct):
    """flat offering index (kp_catalog_patch_* numbering) of type t's (zone, capacity type) offering"""
    row = 0
    for u, it in enumerate(cat):
        for o in it.offerings:
            if u == t and o.zone == zone and o.capacity_type == ct:
                return row
            row += 1
    raise KeyError((t, zone, ct))


def tail_catalog(golden, n_types):
    """n_types random golden types, seeded by n_types (the type-word tails: T = 1, 2, 63, 64, 65, 127, 128, 129)"""
    return sample(golden, n_types, n_types)


# ------------------------------------------------------------------------------------------------
# generator rewrites
# ------------------------------------------------------------------------------------------------
def high_zones(prob, zones, seed):
    """Moves a fuzzed Problem (or a ConsolidationProblem's cluster) into the upper half of `zones`: every NodePool's
    zone requirement becomes In [5 random zones of the upper half + the last zone], the classes' own zone requirements
    are dropped (they would rarely meet a pool's six zones), existing nodes are relabelled into the upper half.  Below 64
    zones class 0 says zone NotIn [a zone no catalog has], so the zone dictionary gains a pod value (63 zones: exactly
    64 values)."""
    p = prob.cluster if isinstance(prob, model.ConsolidationProblem) else prob
    rng = np.random.Generator(np.random.PCG64(seed + 31))
    upper = list(zones[len(zones) // 2:])
    for np_ in p.nodepools:
        sub = sorted(set(str(z) for z in rng.choice(upper[:-1], size=5, replace=False)) | {zones[-1]})
        np_.requirements = [r for r in np_.requirements if r.key != ZONE] + [Requirement(ZONE, "In", sub)]
    for pc in p.classes:
        pc.requirements = [r for r in pc.requirements if r.key != ZONE]
    if len(zones) < 64 and p.classes:
        p.classes[0].requirements = list(p.classes[0].requirements) + [Requirement(ZONE, "NotIn", [FOREIGN_ZONE])]
    for n in p.existing:
        n.labels[ZONE] = str(rng.choice(upper))
    return prob


def launch_requests(cat, n, seed, source=None):
    """synth.launch_requests with its draws fitted to `cat`: the requests are drawn over `source` (a catalog wide enough
    for the generator's In-list sizes; cat itself by default), then every instance-type / instance-family In list is
    redrawn from cat's own names and families with its length clamped to what cat has, and every zone In list from cat's
    own zones, three in four from the upper half."""
    reqs = synth.launch_requests(source if source is not None else cat, n=n, seed=seed)
    rng = np.random.Generator(np.random.PCG64(seed + 606))
    names = [it.name for it in cat]
    fams = sorted({(it.labels.get(FAMILY) or [""])[0] for it in cat} - {""})
    zs = zones_of(cat)
    upper = zs[len(zs) // 2:]
    for lr in reqs:
        for r in lr.requirements:
            if r.op != "In":
                continue
            if r.key == INSTANCE_TYPE:
                r.values = [names[int(x)] for x in rng.choice(len(names), size=min(len(r.values), len(names)),
                                                              replace=False)]
            elif r.key == FAMILY and fams:
                r.values = [fams[int(x)] for x in rng.choice(len(fams), size=min(len(r.values), len(fams)),
                                                             replace=False)]
            elif r.key == ZONE:
                r.values = sorted({str(rng.choice(upper if rng.random() < 0.75 else zs)) for _ in r.values})
    return reqs


# ------------------------------------------------------------------------------------------------
# hand KATs: inputs and plain expectations
# ------------------------------------------------------------------------------------------------
def kat_daemon():
    d = np.zeros(model.R, np.int64)
    d[model.RIDX["cpu"]] = 250
    d[model.RIDX["memory"]] = 512 * 2 ** 20 * 1000
    d[model.RIDX["pods"]] = 2000
    return d


def kat_pool(cat):
    cts = []
    for _, c in slots(cat):
        if c not in cts:
            cts.append(c)
    return synth.default_nodepool(capacity_types=tuple(cts), daemon_overhead=kat_daemon())


def expected_options(cat, need, zone, cts, M=60):
    """A NodeClaim's Truncate(60) list for requirements zone In [zone], capacity-type In cts and total requests `need`
    (daemon overhead included): the types whose allocatable holds `need` and that have an available offering in the zone,
    ordered by their cheapest such price, then by name.  -> (type rows, number of options before truncation)"""
    rows = []
    for t, it in enumerate(cat):
        if any(need[r] > 0 and need[r] > it.allocatable[r] for r in range(model.R)):
            continue
        prices = [o.price for o in it.offerings if o.available and o.zone == zone and o.capacity_type in cts]
        if prices:
            rows.append((min(prices), it.name, t))
    rows.sort()
    return [t for _, _, t in rows[:M]], len(rows)


def kat_every_zone(cat):
    """One class per zone (zone In [z]) with one small pod each, in zone order.  -> (Problem, per pod: (type rows,
    n_options)).  Identical requests, creation order decides: pod i opens NodeClaim i, alone."""
    zs = zones_of(cat)
    pool = kat_pool(cat)
    classes = [model.PodClass([Requirement(ZONE, "In", [z])]) for z in zs]
    pods = synth._pods_from_milli([(i, {"cpu": 500, "memory": 2 ** 30 * 1000}) for i in range(len(zs))])
    prob = model.Problem(cat, [pool], classes, pods)
    cts = pool.requirements[0].values
    expect = [expected_options(cat, pods.requests[i] + pool.daemon_overhead, z, cts) for i, z in enumerate(zs)]
    return prob, expect


def check_every_zone(prob, res, expect):
    r, reqs = res
    n = len(expect)
    assert r.n_nodeclaims == n
    assert sorted(r.pod_result.tolist()) == list(range(n))
    zs = zones_of(prob.catalog)
    for i, (types, n_opt) in enumerate(expect):
        nc = int(r.pod_result[i])
        assert r.nodeclaim_types[nc] == types, (i, zs[i], r.nodeclaim_types[nc][:8], types[:8])
        assert int(r.nodeclaim_n_options[nc]) == n_opt, (i, zs[i])
        assert int(r.nodeclaim_n_pods[nc]) == 1
        comp, _, _, _, vals = reqs[nc][ZONE]
        assert not comp and vals == (zs[i],), (i, reqs[nc][ZONE])


def kat_spread(cat, min_domains=False):
    """A Deployment with a zonal spread of maxSkew 1 over every zone of the catalog: 130 pods, or (min_domains) one pod
    fewer than zones with minDomains = the zone count."""
    nz = len(zones_of(cat))
    sel = [Requirement("app", "In", ["web"])]
    term = model.TopologyTerm("spread", ZONE, sel, max_skew=1, min_domains=nz if min_domains else None)
    pc = model.PodClass(labels={"app": "web"}, topology=[term])
    n = nz - 1 if min_domains else 130
    pods = synth._pods_from_milli([(0, {"cpu": 100, "memory": 128 * 2 ** 20 * 1000})] * n)
    return model.Problem(cat, [kat_pool(cat)], [pc], pods)


def check_spread(prob, res):
    """every pod scheduled, every NodeClaim in one zone, one NodeClaim per used zone, as many zones as pods allow, and
    the zones' pod counts within maxSkew 1 of each other"""
    r, reqs = res
    zs = zones_of(prob.catalog)
    P = prob.pods.n
    assert (r.pod_result >= 0).all()
    per_zone = {}
    for nc in range(r.n_nodeclaims):
        comp, _, _, _, vals = reqs[nc][ZONE]
        assert not comp and len(vals) == 1 and vals[0] in zs, (nc, reqs[nc][ZONE])
        assert vals[0] not in per_zone, "two NodeClaims in %s" % vals[0]
        per_zone[vals[0]] = int(r.nodeclaim_n_pods[nc])
    assert r.n_nodeclaims == min(P, len(zs))
    counts = [per_zone.get(z, 0) for z in zs]
    assert sum(counts) == P and max(counts) - min(counts) <= 1, counts


def kat_two_types(cat, slot, a_available=True, b_available=True):
    """Types A and B (rows in two different 64-type words) and one pod with instance-type In [A, B], zone In [the slot's
    zone], capacity-type In [the slot's type].  Returns (Problem over a copy of the catalog, A, B, zone, capacity type,
    A's and B's offering rows at the slot); both types are available everywhere except as the flags say at the slot."""
    cat = copy.deepcopy(cat)
    zone, ct = slots(cat)[slot]
    need = synth._pods_from_milli([(0, {"cpu": 500, "memory": 2 ** 30 * 1000})]).requests[0] + kat_daemon()
    aws = "karpenter.k8s.aws/instance-"
    # plain types only: the launch path drops metal / accelerator types while others remain (filterExoticInstanceTypes)
    fits = [t for t, it in enumerate(cat) if all(need[r] <= it.allocatable[r] for r in range(model.R) if need[r] > 0)
            and any(o.zone == zone and o.capacity_type == ct for o in it.offerings)
            and (it.labels.get(aws + "size") or [""])[0] != "metal"
            and not it.labels.get(aws + "gpu-count") and not it.labels.get(aws + "accelerator-count")]
    A = fits[0]
    B = next(t for t in reversed(fits) if t // 64 != A // 64) if len(cat) > 64 else fits[-1]
    for t, av in ((A, a_available), (B, b_available)):
        for o in cat[t].offerings:
            o.available = True if (o.zone, o.capacity_type) != (zone, ct) else av
    pc = model.PodClass([Requirement(INSTANCE_TYPE, "In", [cat[A].name, cat[B].name]), Requirement(ZONE, "In", [zone]),
                         Requirement(CAPACITY_TYPE, "In", [ct])])
    pods = synth._pods_from_milli([(0, {"cpu": 500, "memory": 2 ** 30 * 1000})])
    prob = model.Problem(cat, [kat_pool(cat)], [pc], pods)
    return prob, A, B, zone, ct, offering_row(cat, A, zone, ct), offering_row(cat, B, zone, ct)


def availability(cat):
    return np.array([1 if o.available else 0 for it in cat for o in it.offerings], np.uint8)


def by_price_then_name(cat, rows, zone, ct):
    """the order OrderByPrice gives types `rows` whose only admitted offering is (zone, ct)"""
    def price(t):
        return min(o.price for o in cat[t].offerings if o.available and o.zone == zone and o.capacity_type == ct)
    return sorted(rows, key=lambda t: (price(t), cat[t].name))


def price_steps(cat):
    """(Problem, launch request, steps) of the price KAT at the catalog's last slot; steps: (patches, expected type
    order, expected override rows)"""
    slot = len(slots(cat)) - 1
    prob, A, B, zone, ct, ra, rb = kat_two_types(cat, slot)
    pb = next(o.price for o in prob.catalog[B].offerings if (o.zone, o.capacity_type) == (zone, ct))
    lr = model.LaunchRequest(list(prob.classes[0].requirements), prob.pods.requests[0] + kat_daemon())
    return prob, lr, [([(ra, pb / 2)], [A, B], [ra, rb]), ([(ra, pb * 2)], [B, A], [rb, ra])]


def top_slots(cat):
    """the last slot, and the two around the 32-bit edge"""
    n = len(slots(cat))
    return sorted({n - 1, 31, 32})


def single_zone(reqs_i, zones):
    comp, _, _, _, vals = reqs_i.get(ZONE, (True, "", "", "", ()))
    return vals[0] if (not comp and len(vals) == 1 and vals[0] in zones) else None


# ------------------------------------------------------------------------------------------------
# the fuzz families over a zoned catalog (device parity in test_gpu_word_edges.py, non-vacuity in test_word_edges_cpu.py)
# ------------------------------------------------------------------------------------------------
FAMILY_SEEDS = {"requirements": 6, "topology": 6, "topology_existing": 4, "consolidation": 4, "topology_consolidation": 4}


def family_problem(cat, family, seed):
    """seed-th problem of a fuzz family over a zoned catalog: the generator draws over the catalog's own zones, then
    high_zones moves pools and nodes into the upper half"""
    zs = zones_of(cat)
    if family == "requirements":
        prob = fuzzgen.fuzz_problem(cat, 7000 + seed, n_pods=200, zones=zs)
    elif family == "topology":
        prob = fuzzgen.fuzz_topology_problem(cat, 7100 + seed, n_pods=200, zones=zs)
    elif family == "topology_existing":
        prob = fuzzgen.fuzz_topology_existing_problem(cat, 7200 + seed, n_pods=200, zones=zs)
    elif family == "consolidation":
        # no pending pods and every node a candidate: few pods per probe, so probes whose pods all reschedule occur
        prob = fuzzgen.fuzz_consolidation(cat, 7300 + seed, n_nodes=40, n_pods=200, zones=zs, n_candidates=40,
                                          pending_frac=0.0)
    elif family == "topology_consolidation":
        prob = fuzzgen.fuzz_topology_consolidation(cat, 7300 + seed, n_nodes=40, n_pods=200, zones=zs, n_candidates=40,
                                                   pending_frac=0.0)
    else:
        raise KeyError(family)
    return high_zones(prob, zs, seed)


def apply_patches(cat, available=None, prices=()):
    """the catalog a re-List would give after kp_catalog_patch_avail(available) and kp_catalog_patch_price(prices):
    a copy with the flat offering rows' flags and prices changed (prices: (row, price) pairs)"""
    cat = copy.deepcopy(cat)
    flat = [o for it in cat for o in it.offerings]
    if available is not None:
        for o, a in zip(flat, available):
            o.available = bool(a)
    for row, p in prices:
        flat[int(row)].price = float(p)
    return cat


def min_values_problem(golden, M):
    """a fuzzed Solve whose NodePools carry minValues on instance-family: with the option list cut to M = 1 a NodeClaim
    misses SatisfiesMinValues that meets it at 60 (test_word_edges_cpu.test_min_values_fail_at_one)"""
    prob = fuzzgen.fuzz_problem(sample(golden, 200, 77), 9303, n_pods=200, with_min=True)
    prob.max_instance_types = M
    return prob


def replace_cluster(golden, M):
    """Two full nodes of the catalog's dearest on-demand type, each a candidate holding one small pod, one on-demand
    NodePool: every single-node probe and the two-node probe reschedule onto one new NodeClaim that any small type holds,
    so the command is a REPLACE whose option list is the M cheapest types (M = 64: a full 64-entry replacement list).
    -> (ConsolidationProblem, the plain expectation of the BOTH command's type rows); capacity_type 0 = on-demand"""
    za = "test-zone-1a"

    def od_price(it, zone=None):
        ps = [o.price for o in it.offerings if o.available and o.capacity_type == "on-demand" and zone in (None, o.zone)]
        return min(ps) if ps else None
    dear = max((t for t, it in enumerate(golden) if od_price(it, za) is not None), key=lambda t: od_price(golden[t], za))
    it = golden[dear]
    pods = synth._pods_from_milli([(0, {"cpu": 100, "memory": 128 * 2 ** 20 * 1000})] * 2)
    nodes, cands = [], []
    for j in range(2):
        labels = synth.node_labels(it, za, "on-demand", "default")
        nodes.append(model.ExistingNode("node-%d" % j, labels, np.zeros(model.R, np.int64), np.zeros(model.R, np.int64)))
        cands.append(model.Candidate(node=j, pods=np.array([j], np.int32), price=synth.candidate_price(it, labels),
                                     capacity_type=0, instance_type=dear, nodepool=0,
                                     capacity=np.array(it.capacity, np.int64)))
    cluster = model.Problem(golden, [synth.default_nodepool()], [model.PodClass()], pods, nodes, max_instance_types=M)
    cp = model.ConsolidationProblem(cluster, cands, np.zeros(0, np.int32), np.ones(2, np.uint8))
    need = pods.requests.sum(axis=0)  # the two-node probe comes first in a BOTH pass: both pods on one NodeClaim
    rows = sorted((od_price(t_), t_.name, t) for t, t_ in enumerate(golden)
                  if od_price(t_) is not None and all(need[r] <= t_.allocatable[r] for r in range(model.R) if need[r] > 0))
    return cp, [t for _, _, t in rows[:M]]
