"""Reference for kp_consolidate_explain: computeConsolidation's tail restated in Python over the CPU oracle's outputs.

The oracle reports no reasons, so the expectation for the device's rows comes from here; tests/test_cons_explain_cpu.py
pins this file to the unmodified oracle (the restated decision, validity, option count and replacement price of every
probe equal pyoracle.consolidate's row).

A probe's SimulateScheduling is an oracle Solve of its reduced cluster: the state nodes minus the candidates, the
pending pods plus the candidates' pods, the candidates' capacity back in their NodePools' limits.  That Solve returns
the NodeClaim before computeConsolidation touches it, and the placeless pods with it.  (pyoracle.consolidate_replacement
over raised candidate prices cannot serve: it narrows the requirements text to spot and, for multi-node probes, runs
filterOutSameInstanceType under the narrowed requirements, which drops on-demand-only options from the list.)  From
its one NodeClaim (options after TruncateInstanceTypes in OrderByPrice order, requirements text) the tail is restated:
WorstLaunchPrice (reserved, spot, on-demand; the most expensive compatible available offering of the first capacity
type present), the price filter, the minValues check, the 15-option rule of single-node spot-to-spot,
filterOutSameInstanceType.

Scope: catalogs without reserved offerings, clusters without topology terms or preferences.
"""
import dataclasses

import numpy as np

import explain_ref
from kpsim import abi, model
from kpsim.model import CAPACITY_TYPE, ZONE

ZONE_ID = "topology.k8s.aws/zone-id"
DBL_MAX = float(np.finfo(np.float64).max)


# ---- the corpus shared by tests/test_cons_explain_cpu.py and tests/test_gpu_cons_explain.py ----
def fuzz_case(golden, seed):
    """test_gpu_consolidation.py::test_fuzz_consolidation's inputs: (ConsolidationProblem, spot_to_spot)"""
    import fuzzgen
    rng = np.random.Generator(np.random.PCG64(500 + seed))
    sub = [golden[int(i)] for i in sorted(rng.choice(len(golden), size=int(rng.integers(60, 300)), replace=False))]
    cp = fuzzgen.fuzz_consolidation(sub, 500 + seed, n_nodes=int(rng.integers(4, 80)),
                                    n_pods=int(rng.integers(20, 300)), all_spot=seed % 4 == 0)
    return cp, seed % 2 == 0


def min_values_case(golden, seed):
    """test_gpu_consolidation.py::test_fuzz_consolidation_min_values's inputs"""
    import fuzzgen
    rng = np.random.Generator(np.random.PCG64(900 + seed))
    sub = [golden[int(i)] for i in sorted(rng.choice(len(golden), size=int(rng.integers(60, 300)), replace=False))]
    cp = fuzzgen.fuzz_consolidation(sub, 900 + seed, n_nodes=int(rng.integers(4, 80)),
                                    n_pods=int(rng.integers(20, 300)), all_spot=seed % 3 == 0, with_min=True)
    for np_ in cp.cluster.nodepools:
        if not any(r.min_values for r in np_.requirements):
            np_.requirements.append(model.Requirement("karpenter.k8s.aws/instance-family", "Exists", [],
                                                      int(rng.choice([1, 2, 5, 20, 40]))))
    return cp, seed % 2 == 0


def probe_candidates(cp, mode, probe):
    return [probe] if mode == abi.KP_CONSOLIDATE_SINGLE else list(range(probe + 2))


def queue_key(prob, p):
    """NewQueue's byCPUAndMemoryDescending, then creation time and UID"""
    rq = prob.pods.requests[p]
    return (-int(rq[model.RIDX["cpu"]]), -int(rq[model.RIDX["memory"]]), int(prob.pods.creation_ns[p]), prob.pods.uids[p])


def reduced_problem(cp, cands):
    """(Problem, pods, nodes) of the probe over candidates `cands`: its pods (pending first) and state nodes as indices
    into cp.cluster's."""
    prob = cp.cluster
    gone = {int(cp.candidates[c].node) for c in cands}
    nodes = [j for j in range(len(prob.existing)) if j not in gone]
    pods = [int(p) for p in cp.pending] + [int(p) for c in cands for p in cp.candidates[c].pods]
    pools = []
    for i, pool in enumerate(prob.nodepools):
        lim = dict(pool.limits_remaining) if pool.limits_remaining else pool.limits_remaining
        if lim:
            for c in cands:
                cd = cp.candidates[c]
                if cd.nodepool == i and cd.capacity is not None:
                    for r in lim:
                        lim[r] += int(cd.capacity[model.RIDX[r]])
        pools.append(dataclasses.replace(pool, limits_remaining=lim))
    idx = np.array(pods, np.int64)
    pv = model.Pods(prob.pods.class_id[idx], prob.pods.requests[idx], prob.pods.creation_ns[idx],
                    [prob.pods.uids[p] for p in pods],
                    None if prob.pods.volumes is None else [prob.pods.volumes[p] for p in pods])
    pos = {j: i for i, j in enumerate(nodes)}
    red = dataclasses.replace(prob, nodepools=pools, pods=pv, existing=[prob.existing[j] for j in nodes],
                              bound=[(pos[j], c) for j, c in prob.bound if j in pos])
    return red, pods, nodes


def _admits(reqs, key, value):
    r = reqs.get(key)
    if r is None:
        return True
    comp, gt, lt, _mn, vals = r
    assert gt == "-" and lt == "-", "bounds on an offering key"
    return (value not in vals) if comp else (value in vals)


def worst_launch_price(it, reqs):
    """Offerings.Available().WorstLaunchPrice(reqs)"""
    for ct in ("reserved", "spot", "on-demand"):
        ps = [o.price for o in it.offerings
              if o.available and o.capacity_type == ct and _admits(reqs, CAPACITY_TYPE, ct) and
              _admits(reqs, ZONE, o.zone) and (o.zone_id is None or _admits(reqs, ZONE_ID, o.zone_id))]
        if ps:
            return max(ps)
    return DBL_MAX


def _spot(reqs):
    out = dict(reqs)
    mn = reqs[CAPACITY_TYPE][3] if CAPACITY_TYPE in reqs else "-"
    out[CAPACITY_TYPE] = (False, "-", "-", mn, ("spot",))
    return out


def satisfies_min_values(ref, opts, reqs):
    """InstanceTypes.SatisfiesMinValues -> (ok, minNeeded)"""
    mins = {k: int(q[3]) for k, q in reqs.items() if q[3] != "-"}
    if not mins:
        return True, 0
    seen = {k: set() for k in mins}
    for i, t in enumerate(opts):
        for k in mins:
            seen[k] |= set(ref.types[t][0].get_req(k).values)
        if all(len(seen[k]) >= mins[k] for k in mins):
            return True, i + 1
    return all(len(seen[k]) >= mins[k] for k in mins), len(opts)


class ConsRef:
    def __init__(self, cp, spot_to_spot):
        for it in cp.cluster.catalog:
            assert not any(o.reservation_id for o in it.offerings), "the restatement does not cover reserved offerings"
        self.cp, self.s2s = cp, spot_to_spot
        self.ref = explain_ref.Ref(cp.cluster)

    def simulate(self, mode, probe):
        """The probe's SimulateScheduling: dict with the reduced Problem, its oracle Results and requirement texts, the
        probe's pods / nodes, its placeless non-pending pods in queue order, whether a non-pending pod landed on an
        uninitialized node, its valid NodeClaims and the non-pending pods on dropped ones."""
        import pyoracle
        cp = self.cp
        cands = probe_candidates(cp, mode, probe)
        red, pods, nodes = reduced_problem(cp, cands)
        o = pyoracle.solve(red)
        r = o.results
        n_pend = len(cp.pending)
        valid = [n for n in range(r.n_nodeclaims) if int(r.nodeclaim_nodepool[n]) >= 0]
        placeless, dropped, uninit = [], 0, False
        for li in range(n_pend, len(pods)):
            res = int(r.pod_result[li])
            if res == -1:
                placeless.append(pods[li])
            elif res <= -2:
                if cp.initialized is not None and not cp.initialized[nodes[-2 - res]]:
                    uninit = True
            elif res not in valid:
                dropped += 1
        placeless.sort(key=lambda p: queue_key(cp.cluster, p))
        return dict(red=red, results=r, oracle=o, pods=pods, nodes=nodes, cands=cands, placeless=placeless,
                    dropped=dropped, uninit=uninit, valid=valid,
                    truncated=any(int(x) < 0 for x in r.nodeclaim_nodepool[:r.n_nodeclaims]))

    def explain(self, mode, probe, sim=None):
        """(kp_probe_explanation as a dict, restated (decision, valid, n_replacement_types, replacement_price))"""
        cp = self.cp
        sim = sim or self.simulate(mode, probe)
        cands, r = sim["cands"], sim["results"]
        cprice = 0.0
        for c in cands:
            cprice += float(cp.candidates[c].price)
        all_spot = all(cp.candidates[c].capacity_type == abi.KP_CT_SPOT for c in cands)
        row = dict(reason=abi.KP_UNCONS_NONE, flags=0, n_unscheduled=0, first_unscheduled=-1, n_options=0, n_cheaper=0,
                   min_needed=0, pad=0, candidate_price=cprice, cheapest_price=0.0)
        none = (abi.KP_DECISION_NONE, 0, 0, 0.0)
        valid = sim["valid"]
        if len(valid) >= 2:  # the device stops at the second NodeClaim: this wins over an unschedulable pod
            row["reason"] = abi.KP_UNCONS_MULTIPLE_NODECLAIMS
            return row, none
        if sim["placeless"] or sim["uninit"] or sim["dropped"]:
            row["reason"] = abi.KP_UNCONS_PODS_UNSCHEDULABLE
            row["n_unscheduled"] = len(sim["placeless"]) + sim["dropped"]
            row["first_unscheduled"] = sim["placeless"][0] if sim["placeless"] else -1
            if sim["uninit"]:
                row["flags"] |= abi.KP_UNCONS_F_UNINITIALIZED_NODE
            if sim["truncated"]:
                row["flags"] |= abi.KP_UNCONS_F_TRUNCATED
            return row, none
        if not valid:
            if sim["truncated"]:
                row["flags"] |= abi.KP_UNCONS_F_TRUNCATED
            return row, (abi.KP_DECISION_DELETE, 1, 0, 0.0)
        nc = valid[0]
        opts = [int(t) for t in r.nodeclaim_types[nc]]
        reqs = model.parse_requirements_blob(sim["oracle"].requirements(nc))
        cat = cp.cluster.catalog
        has_spot, has_od = _admits(reqs, CAPACITY_TYPE, "spot"), _admits(reqs, CAPACITY_TYPE, "on-demand")
        has_min = any(q[3] != "-" for q in reqs.values())
        row["n_options"] = len(opts)
        if all_spot and has_spot:
            row["flags"] |= abi.KP_UNCONS_F_SPOT_TO_SPOT
            reqs = _spot(reqs)
        wl = [worst_launch_price(cat[t], reqs) for t in opts]
        keep = [t for t, w in zip(opts, wl) if w < cprice]
        row["n_cheaper"] = len(keep)
        row["cheapest_price"] = min(wl) if wl else 0.0
        ok, need = satisfies_min_values(self.ref, keep, reqs)
        if all_spot and has_spot:
            if not self.s2s:
                row["reason"] = abi.KP_UNCONS_SPOT_TO_SPOT_DISABLED
                return row, none
            if not ok:
                row["reason"] = abi.KP_UNCONS_MIN_VALUES
                return row, none
            row["min_needed"] = need if has_min else 0
            if not keep:
                row["reason"] = abi.KP_UNCONS_NOT_CHEAPER
                return row, none
            if len(cands) == 1:
                if len(keep) < 15:
                    row["reason"] = abi.KP_UNCONS_SPOT_TO_SPOT_TOO_FEW
                    return row, none
                keep = keep[:max(15, need) if has_min else 15]
        else:
            if not ok:
                row["reason"] = abi.KP_UNCONS_MIN_VALUES
                return row, none
            if not keep:
                row["reason"] = abi.KP_UNCONS_NOT_CHEAPER
                return row, none
            if has_spot and has_od:
                reqs = _spot(reqs)
        if mode == abi.KP_CONSOLIDATE_MULTI:  # filterOutSameInstanceType
            ps = [float(cp.candidates[c].price) for c in cands if cp.candidates[c].instance_type in keep]
            maxp = min(ps) if ps else DBL_MAX
            keep = [t for t in keep if worst_launch_price(cat[t], reqs) < maxp]
            if not keep:
                row["reason"] = abi.KP_UNCONS_SAME_INSTANCE_TYPE
        price = min(worst_launch_price(cat[t], reqs) for t in keep) if keep else 0.0
        return row, (abi.KP_DECISION_REPLACE, 1 if keep else 0, len(keep), price)

    def remaining(self, sim):
        """The probe's remaining NodePool limits at its end, as explain_ref.Ref.final_remaining computes them over the
        reduced cluster's Solve: {nodepool index: {resource: milli}}."""
        return explain_ref.Ref(sim["red"]).final_remaining(sim["results"])

    def rows(self, mode):
        n = model.consolidation_probe_count(len(self.cp.candidates), mode)
        out = np.zeros(n, abi.PROBE_EXPLANATION_DTYPE)
        dec = []
        for i in range(n):
            row, d = self.explain(mode, i)
            for k, v in row.items():
                out[i][k] = v
            dec.append(d)
        return out, dec
