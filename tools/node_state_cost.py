"""Cost figures of the node-side-state (PORTS) Solve entry points (DESIGN.md §6 "Volume limits").

  volumes  the volume test in wave 0's existing-node scan: config 2 (50k pods) over a 2,000-node cluster whose nodes
           carry one mounted claim and an attach limit of 12 on one driver (so both runs launch the PORTS entry point),
           with and without one private claim per pod
  ports    a port-only solve, for A/B against another build of the library: a seeded 5,000-pod sample of config 2, every
           fifth class binding hostPort 80 (its pods take a NodeClaim each)

Prints one JSON line with the FFD kernel's milliseconds over 4 executes of one prepare.  KPSIM_ROOT selects the tree
whose package and library are measured (default: this one).
"""
import json
import os
import sys

ROOT = os.environ.get("KPSIM_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "karpenter-provider-aws_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402

import fuzzgen  # noqa: E402
from kpsim import catalog, model, native, synth  # noqa: E402

DRIVER = "ebs.csi.aws.com"


def measure(ctx, prob):
    ctx.prepare(model.SolveInputView(prob))
    ms = []
    for _ in range(4):
        ctx.execute()
        ms.append(float(ctx.kernel_times_ms()[3]))
    o = model.OutputBuffers(prob.pods.n, prob.pods.n + 1, (prob.pods.n + 1) * 60)
    ctx.fetch(o)
    r = o.results()
    return {"ffd_ms": ms, "ffd_ms_median_warm": float(np.median(ms[1:])), "on_existing": int((r.pod_result <= -2).sum()),
            "nodeclaims": int(r.n_nodeclaims)}


def main(mode):
    cat = catalog.golden_catalog(fx=catalog.load_fixtures())
    ctx = native.Context(0)
    ctx.upload_catalog(model.CatalogView(cat))
    if mode == "volumes":
        prob = synth.config2(n_pods=50_000, catalog=cat)
        nodes = fuzzgen.existing_nodes(np.random.Generator(np.random.PCG64(7)), cat, 2000)
        for e in nodes:
            e.taints = []
            e.available = np.array(e.available, np.int64)
            e.available[model.RIDX["cpu"]] = 16000
            e.available[model.RIDX["memory"]] = 64 * 2 ** 30 * 1000
            e.available[model.RIDX["pods"]] = 30000
            e.volumes = [(DRIVER, "bound/%s" % e.name)]
            e.volume_limits = {DRIVER: 12}
        prob.existing = nodes
        out = {"metric": "volume test cost, config 2 over 2,000 nodes, PORTS entry points"}
        for tag in ("no_claims", "one_claim_per_pod"):
            prob.pods.volumes = None if tag == "no_claims" else [[(DRIVER, "default/data-%d" % p)] for p in range(prob.pods.n)]
            out[tag] = measure(ctx, prob)
    else:
        prob = synth.subsample(synth.config2(n_pods=50_000, catalog=cat), 5000)
        for c in range(0, len(prob.classes), 5):
            prob.classes[c].host_ports = [model.HostPort(80)]
        out = {"metric": "port-only solve, 5,000 pods of config 2, every fifth class on hostPort 80", "ports": measure(ctx, prob)}
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "volumes")
