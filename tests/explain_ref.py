"""Reference for kp_solve_explain: a small requirement algebra over kpsim.model objects and the stage ladder of
scheduler.add / NodeClaim.Add for one (pod class, requests, NodePool), as plain Python.

The CPU oracle reports no reasons, so the expectation for the device's rows comes from here; tests/test_explain_cpu.py
pins this file to the unmodified oracle (a one-pod, one-NodePool oracle Solve makes a NodeClaim iff the ladder finds no
failing stage).  Covered: In / NotIn / Exists / DoesNotExist / Gt / Lt, Intersects with the NotIn / DoesNotExist
exception, Compatible with the well-known-label allowance, NodePool limits, taints, daemonset host ports, the
instance-type filter with filterResults' criteria, minValues.  Not covered: topology (rows of topology classes are
compared stage-wise by the GPU test) and the reservation residual.
"""
import numpy as np

from kpsim import abi, model

INT64_MAX = (1 << 63) - 1

WELL_KNOWN = {
    "karpenter.sh/nodepool", "topology.kubernetes.io/zone", "topology.kubernetes.io/region",
    "node.kubernetes.io/instance-type", "kubernetes.io/arch", "kubernetes.io/os", "karpenter.sh/capacity-type",
    "node.kubernetes.io/windows-build", "karpenter.k8s.aws/capacity-reservation-id",
    "karpenter.k8s.aws/capacity-reservation-type", "karpenter.k8s.aws/instance-hypervisor",
    "karpenter.k8s.aws/instance-encryption-in-transit-supported", "karpenter.k8s.aws/instance-category",
    "karpenter.k8s.aws/instance-capacity-flex", "karpenter.k8s.aws/instance-family",
    "karpenter.k8s.aws/instance-generation", "karpenter.k8s.aws/instance-size", "karpenter.k8s.aws/instance-local-nvme",
    "karpenter.k8s.aws/instance-cpu", "karpenter.k8s.aws/instance-cpu-manufacturer",
    "karpenter.k8s.aws/instance-cpu-sustained-clock-speed-mhz", "karpenter.k8s.aws/instance-memory",
    "karpenter.k8s.aws/instance-ebs-bandwidth", "karpenter.k8s.aws/instance-network-bandwidth",
    "karpenter.k8s.aws/instance-gpu-name", "karpenter.k8s.aws/instance-gpu-manufacturer",
    "karpenter.k8s.aws/instance-gpu-count", "karpenter.k8s.aws/instance-gpu-memory",
    "karpenter.k8s.aws/instance-accelerator-name", "karpenter.k8s.aws/instance-accelerator-manufacturer",
    "karpenter.k8s.aws/instance-accelerator-count", "topology.k8s.aws/zone-id",
}
NORMALIZED = {
    "failure-domain.beta.kubernetes.io/zone": "topology.kubernetes.io/zone",
    "failure-domain.beta.kubernetes.io/region": "topology.kubernetes.io/region",
    "beta.kubernetes.io/arch": "kubernetes.io/arch", "beta.kubernetes.io/os": "kubernetes.io/os",
    "beta.kubernetes.io/instance-type": "node.kubernetes.io/instance-type",
    "topology.ebs.csi.aws.com/zone": "topology.kubernetes.io/zone",
}


# The fuzz corpus shared by tests/test_explain_cpu.py and tests/test_gpu_explain.py:
# fuzzgen.fuzz_problem(sample(golden, 160, 4242), seed, n_pods=150), the first 12 seeds from 0 on whose oracle Solve
# leaves a pod unschedulable (1 leaves none)
SEEDS = [0, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12]
N_PODS = 150
HOSTNAME = "kubernetes.io/hostname"
PLACEHOLDER = "hostname-placeholder-0001"   # NewNodeClaim: hostname In [a fresh placeholder no pod can name]


def catalog_of(golden):
    import edge_cases
    return edge_cases.sample(golden, 160, 4242)


def problem(sub, seed):
    import fuzzgen
    return fuzzgen.fuzz_problem(sub, seed, n_pods=N_PODS)


def shapes_of(prob, pods):
    """distinct (class, requests) among `pods`, in first-seen order"""
    seen = {}
    for p in pods:
        seen.setdefault((int(prob.pods.class_id[p]), tuple(int(x) for x in prob.pods.requests[p])), int(p))
    return list(seen)


def go_atoi(s):
    """strconv.Atoi: optional sign, decimal digits only, within int64; None when it fails."""
    body = s[1:] if s[:1] in ("+", "-") else s
    if not body or not all("0" <= ch <= "9" for ch in body):
        return None
    v = int(s)
    return v if -(1 << 63) <= v <= INT64_MAX else None


class Req:
    """scheduling.Requirement: a value set or its complement, integer bounds, minValues."""

    def __init__(self, key, complement=False, values=(), gt=None, lt=None, min_values=None):
        self.key, self.complement, self.values = key, complement, frozenset(values)
        self.gt, self.lt, self.min_values = gt, lt, min_values

    @staticmethod
    def new(key, op, values=(), min_values=None):
        if op == "In":
            return Req(key, False, values, min_values=min_values)
        if op == "NotIn":
            return Req(key, True, values, min_values=min_values)
        if op == "Exists":
            return Req(key, True, min_values=min_values)
        if op == "DoesNotExist":
            return Req(key, False, min_values=min_values)
        bound = go_atoi(values[0]) if values else 0
        return Req(key, True, gt=bound if op == "Gt" else None, lt=bound if op == "Lt" else None, min_values=min_values)

    def length(self):
        return INT64_MAX - len(self.values) if self.complement else len(self.values)

    def operator(self):
        if self.complement:
            return "NotIn" if self.values else "Exists"
        return "In" if self.values else "DoesNotExist"

    def negative(self):
        return self.operator() in ("NotIn", "DoesNotExist")

    def within(self, v):
        if self.gt is None and self.lt is None:
            return True
        x = go_atoi(v)
        return x is not None and not (self.gt is not None and self.gt >= x) and not (self.lt is not None and self.lt <= x)

    def has(self, v):
        return ((v not in self.values) if self.complement else (v in self.values)) and self.within(v)

    def intersection(self, q):
        gts = [b for b in (self.gt, q.gt) if b is not None]
        lts = [b for b in (self.lt, q.lt) if b is not None]
        mins = [m for m in (self.min_values, q.min_values) if m is not None]
        gt, lt, mn = (max(gts) if gts else None), (min(lts) if lts else None), (max(mins) if mins else None)
        if gt is not None and lt is not None and gt >= lt:
            return Req(self.key, False, min_values=mn)  # DoesNotExist
        if self.complement and q.complement:
            vals = self.values | q.values
        elif self.complement:
            vals = q.values - self.values
        elif q.complement:
            vals = self.values - q.values
        else:
            vals = self.values & q.values
        bounds = Req(self.key, True, gt=gt, lt=lt)
        vals = [v for v in vals if bounds.within(v)]
        if self.complement and q.complement:
            return Req(self.key, True, vals, gt, lt, mn)
        return Req(self.key, False, vals, min_values=mn)  # a concrete set carries no bounds


class Reqs(dict):
    """scheduling.Requirements: key -> Req; add() intersects with what is there."""

    def add(self, q):
        self[q.key] = q.intersection(self[q.key]) if q.key in self else q

    def merged(self, other):
        out = Reqs(self)
        for q in other.values():
            out.add(q)
        return out

    def get_req(self, key):
        return self[key] if key in self else Req(key, True)  # undefined: Exists


def build_reqs(requirements):
    out = Reqs()
    for r in requirements:
        out.add(Req.new(NORMALIZED.get(r.key, r.key), r.op, list(r.values), r.min_values))
    return out


def intersect_failures(r, q):
    """Keys on which Requirements.Intersects(r, q) fails."""
    bad = []
    for k in r.keys() & q.keys():
        if r[k].intersection(q[k]).length() == 0 and not (q[k].negative() and r[k].negative()):
            bad.append(k)
    return bad


def compatible_failures(r, q, allow_well_known):
    """Keys on which r.Compatible(q) fails: undefined in r (unless NotIn / DoesNotExist or, with the option, a
    well-known label), or an empty intersection."""
    bad = [k for k in q if k not in r and not q[k].negative() and not (allow_well_known and k in WELL_KNOWN)]
    return bad + intersect_failures(r, q)


def tolerates(taints, tolerations):
    def one(t, taint):
        if t.effect and t.effect != taint.effect:
            return False
        if t.key and t.key != taint.key:
            return False
        return t.operator == "Exists" or t.value == taint.value
    return all(any(one(t, taint) for t in tolerations) for taint in taints)


def ports_conflict(a, b):
    """HostPortUsage: same port and protocol, and the IPs are equal or one of them is unspecified."""
    unspec = ("", "0.0.0.0", "::")
    return any(x.port == y.port and x.protocol == y.protocol and (x.ip == y.ip or x.ip in unspec or y.ip in unspec)
               for x in a for y in b)


def template_order(prob):
    """NodePool indices in NodeClaimTemplate order: weight descending, name ascending."""
    return sorted(range(len(prob.nodepools)), key=lambda i: (-prob.nodepools[i].weight, prob.nodepools[i].name))


class Ref:
    def __init__(self, prob):
        self.prob = prob
        self.best_effort = prob.min_values_policy != 0
        self.types = []
        for it in prob.catalog:
            rq = Reqs()
            for k, v in it.labels.items():
                rq.add(Req.new(NORMALIZED.get(k, k), "DoesNotExist" if v is None else "In", list(v or [])))
            offs = []
            for o in it.offerings:
                oq = Reqs()
                for k in model.OFFERING_KEYS:
                    st, v = o.label(k)
                    if st == abi.KP_LABEL_IN:
                        oq.add(Req.new(k, "In", [v]))
                    elif st == abi.KP_LABEL_DOES_NOT_EXIST:
                        oq.add(Req.new(k, "DoesNotExist"))
                offs.append((bool(o.available), oq))
            self.types.append((rq, np.asarray(it.allocatable, np.int64), np.asarray(it.capacity, np.int64), offs))
        self._tmpl = {}

    # ---- the three criteria of filterInstanceTypesByRequirements ----
    def _req_met(self, t, reqs):
        return not intersect_failures(self.types[t][0], reqs)

    def _fits(self, t, total):
        alloc = self.types[t][1]
        return bool((alloc >= 0).all() and (total <= alloc).all())

    def _has_offering(self, t, reqs):
        return any(av and not compatible_failures(reqs, oq, True) for av, oq in self.types[t][3])

    def _min_unmet(self, its, reqs):
        bad = []
        for k, q in reqs.items():
            if q.min_values is None:
                continue
            vals = set()
            for t in its:
                vals |= self.types[t][0].get_req(k).values
            if len(vals) < q.min_values:
                bad.append(k)
        return bad

    def template(self, npi):
        """(requirements, InstanceTypeOptions) of NodePool npi as NewScheduler builds them."""
        if npi not in self._tmpl:
            pool = self.prob.nodepools[npi]
            reqs = build_reqs(pool.template_requirements())
            rows = range(len(self.types)) if pool.instance_types is None else pool.instance_types
            zero = np.zeros(model.R, np.int64)
            opts = [t for t in rows if self._req_met(t, reqs) and self._fits(t, zero) and self._has_offering(t, reqs)]
            if not self.best_effort and self._min_unmet(opts, reqs):
                opts = []
            self._tmpl[npi] = (reqs, opts)
        return self._tmpl[npi]

    def class_reqs(self, c):
        pc = self.prob.classes[c]
        return build_reqs(list(pc.requirements) + (list(pc.required_terms[0]) if pc.required_terms else []))

    def explain(self, c, requests, npi, remaining=None):
        """The row of kp_solve_explain for a pod of class c with `requests` against NodePool npi whose remaining limits
        are `remaining` (resource -> milli; None: the NodePool's own).  reason None: no stage fails; then `options`
        holds the instance types the new NodeClaim would keep."""
        pool, pc = self.prob.nodepools[npi], self.prob.classes[c]
        treqs, topts = self.template(npi)
        row = dict(nodepool=npi, reason=None, key=None, criteria=0, n_options=0, n_requirements=0, n_fits=0,
                   n_offering=0, options=[])
        limits = pool.limits_remaining if remaining is None else remaining
        opts = [t for t in topts
                if all(self.types[t][2][model.RIDX[r]] <= q for r, q in (limits or {}).items())]
        row["n_options"] = len(opts)
        if topts and not opts:
            row["reason"] = abi.KP_WHY_LIMITS
            return row
        if not tolerates(pool.taints, pc.tolerations):
            row["reason"] = abi.KP_WHY_TAINTS
            return row
        if ports_conflict(pool.daemon_host_ports, pc.host_ports):
            row["reason"] = abi.KP_WHY_HOST_PORTS
            return row
        preqs = self.class_reqs(c)
        claim = Reqs(treqs)                      # NewNodeClaim: the template's requirements + its own hostname
        claim.add(Req.new(HOSTNAME, "In", [PLACEHOLDER]))
        bad = compatible_failures(claim, preqs, True)
        if bad:
            row["reason"], row["key"] = abi.KP_WHY_REQUIREMENTS, min(bad)
            return row
        reqs = treqs.merged(preqs)
        daemon = np.zeros(model.R, np.int64) if pool.daemon_overhead is None else np.asarray(pool.daemon_overhead, np.int64)
        total = daemon + np.asarray(requests, np.int64)
        rq = [self._req_met(t, reqs) for t in opts]
        ft = [self._fits(t, total) for t in opts]
        of = [self._has_offering(t, reqs) for t in opts]
        row["n_requirements"], row["n_fits"], row["n_offering"] = sum(rq), sum(ft), sum(of)
        keep = [t for t, a, b, d in zip(opts, rq, ft, of) if a and b and d]
        if not keep:
            pairs = list(zip(rq, ft, of))
            row["reason"] = abi.KP_WHY_INSTANCE_TYPES
            row["criteria"] = ((abi.KP_CRIT_REQUIREMENTS if any(rq) else 0) | (abi.KP_CRIT_FITS if any(ft) else 0) |
                               (abi.KP_CRIT_OFFERING if any(of) else 0) |
                               (abi.KP_CRIT_REQUIREMENTS_AND_FITS if any(a and b for a, b, _ in pairs) else 0) |
                               (abi.KP_CRIT_REQUIREMENTS_AND_OFFERING if any(a and d for a, _, d in pairs) else 0) |
                               (abi.KP_CRIT_FITS_AND_OFFERING if any(b and d for _, b, d in pairs) else 0))
            return row
        if not self.best_effort:
            bad = self._min_unmet(keep, reqs)
            if bad:
                row["reason"], row["key"] = abi.KP_WHY_MIN_VALUES, min(bad)
                return row
        row["options"] = keep
        return row

    def final_remaining(self, results):
        """The NodePools' remaining limits after a Solve with `results` (model.Results of a problem without topology,
        preferences or reservations): every NodeClaim, in creation order, took subtractMax over the options its first
        pod left it.  Returns {nodepool index: {resource: milli}} for the NodePools with limits."""
        prob = self.prob
        rem = {i: dict(p.limits_remaining) for i, p in enumerate(prob.nodepools) if p.limits_remaining}
        res = np.asarray(results.pod_result)
        order = np.asarray(results.pod_order)
        for n in range(results.n_nodeclaims):
            npi = int(results.nodeclaim_nodepool[n])
            assert npi >= 0, "a NodeClaim FinalizeScheduling dropped: the replay does not cover it"
            if npi not in rem:
                continue
            pods = np.nonzero(res == n)[0]
            first = int(pods[np.argmin(order[pods])])
            row = self.explain(int(prob.pods.class_id[first]), prob.pods.requests[first], npi, rem[npi])
            assert row["reason"] is None, (n, first, row)
            for r in rem[npi]:
                rem[npi][r] -= max(int(self.types[t][2][model.RIDX[r]]) for t in row["options"])
        return rem

    def rows(self, c, requests, remaining=None):
        """A pod's rows in template order (remaining: {nodepool index: limits} as final_remaining returns)."""
        return [self.explain(c, requests, i, (remaining or {}).get(i)) for i in template_order(self.prob)]
