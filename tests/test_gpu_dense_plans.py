"""GPU: Solve parity on node-dense plans whose slice keys differ (tests/dense_cases.py): the *_hbm_kernel instantiations
of every family, with the slice arrays in HBM, and the mid plan (slices in LDS, allocatable table in HBM, quick-accept
rows for the first lds_nq NodeClaims only).  Every case has 4,100 NodeClaims of three pod counts, so each commit leaves an
inversion that sort.Slice resolves over thousands of positions: block-wide stable moves and full pdqsort emulations at
slice length 4,100, through the d.g_* pointers at the hbm size.

test_dense_parity: device == oracle on every output field, requirements included; the plan of the solve
(Context.solve_plan) names the entry point the family claims and the plan of its size; the device counters show that
full sorts, stable moves, quick accepts and the slow path all ran.
test_dense_twin: the production *_hbm_kernel against its diagnostic twin (KPSIM_PROFILE), base and topology.
test_dense_split_calls_and_plan_reset: the overflow seen through prepare / execute / fetch, the one re-plan for every
pod, and a small solve afterwards that starts from the first plan again.

Device time of the Solve kernel (kernel_times_ms()[3] of the re-planned attempt, one run each on an MI355X), ms,
hbm / mid: base 321 / 224, pref 566 / 306, resv 334 / 219, topo 538 / 365, ports 475 / 273, pref_resv_topo 1,379 -
1,420 / 1,222, ports_resv_topo 599 / 428.  The parent commit's kernels are the same code: only the plan accessor is new.
At base-hbm the solve takes 3,237 full sorts and 10,760 counted stable moves at slice length 4,100 through HBM.
lds_nq at the mid size: 505 (base, pref, ports), 1,281 (topo), 1,832 (resv), 2,608 (pref_resv_topo, ports_resv_topo);
quick accepts there: 505, 25, 336, 256, 2,622, 1,583 and 1,448.
"""
import pytest

import dense_cases as DC
import parity
import test_gpu_profile_twins as PT
from kpsim import abi, model, native, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cats(golden):
    return DC.Catalogs(golden)


def _case(cats, name):
    family, size = name.rsplit("-", 1)
    return DC.build(cats, family, size)


def _assert_plan(case, plan, n_nodeclaims, twin=0):
    P = case.problem.pods.n
    for b in ("ports", "pref", "resv", "topo"):
        assert plan[b] == case.bits[b], (b, plan)
    assert plan["twin"] == twin
    assert plan["NCcap"] == P            # the re-plan for every pod ran
    assert plan["alloc_global"] == 1
    if case.size == "hbm":
        assert plan["slice_hbm"] == 1
    else:
        assert plan["slice_hbm"] == 0 and 0 < plan["lds_nq"] < n_nodeclaims, plan


@pytest.mark.parametrize("name", DC.NAMES)
def test_dense_parity(cats, name):
    case = _case(cats, name)
    orc = DC.run_oracle(case)
    P = case.problem.pods.n
    ctx = native.Context(0, preference_policy=case.preference_policy)  # its own ctx: the grown capacity stays with it
    try:
        dev = parity.run_device(ctx, case.problem)
        plan, cyc, ms = ctx.solve_plan(), ctx.ffd_cycles(), ctx.kernel_times_ms()
    finally:
        ctx.close()
    st = dev[0].stats
    print(name, "kernel_ms %.1f" % ms[3], "plan", plan, "sorts_full", st["sorts_full"], "sorts_fast", st["sorts_fast"],
          "quick", cyc[12], "slow", cyc[13], "popped", st["pods_popped"])
    parity.assert_same(dev, orc)
    _assert_plan(case, plan, orc[0].n_nodeclaims)
    assert st["sorts_full"] > 0
    assert cyc[13] > 0   # slow-path pods
    assert st["sorts_fast"] > 0
    assert cyc[12] > 0   # quick accepts
    if case.bits["pref"]:
        assert st["pods_popped"] > P


@pytest.mark.parametrize("family", ["base", "topo"])
def test_dense_twin(cats, family):
    case = _case(cats, family + "-hbm")
    orc = DC.run_oracle(case)
    plain, cp, pp = PT._solve(case.problem, case.preference_policy, profile=False, want_plan=True)
    twin, ct, pt = PT._solve(case.problem, case.preference_policy, profile=True, want_plan=True)
    parity.assert_same(plain, orc)
    parity.assert_same(twin, plain)
    for f, _ in abi.kp_solve_stats._fields_:
        if not f.startswith("ns_"):
            assert plain[0].stats[f] == twin[0].stats[f], f
    for k in PT.ALWAYS:
        assert cp[k] == ct[k], k
    assert ct["cyc_fast_loop"] > 0
    for k in PT.PROFILING_ONLY:
        assert cp[k] == 0, k
    _assert_plan(case, pp, orc[0].n_nodeclaims, twin=0)
    _assert_plan(case, pt, orc[0].n_nodeclaims, twin=1)


def _fetch(ctx, prob):
    cap_nc = max(16, prob.pods.n + 1)
    out = model.OutputBuffers(prob.pods.n, cap_nc, cap_nc * prob.max_instance_types)
    ctx.fetch(out)
    r = out.results()
    return r, [model.parse_requirements_blob(ctx.nodeclaim_requirements(i)) for i in range(r.n_nodeclaims)]


def test_dense_split_calls_and_plan_reset(cats, golden):
    case = _case(cats, "base-hbm")
    prob, P = case.problem, case.problem.pods.n
    small = synth.subsample(synth.config2(catalog=golden), 500)
    ctx = native.Context(0)
    fresh = native.Context(0)
    try:
        ctx.upload_catalog(model.CatalogView(prob.catalog))
        iv = model.SolveInputView(prob)
        ctx.prepare(iv)
        ctx.execute()
        with pytest.raises(native.KpError) as e:
            _fetch(ctx, prob)
        assert e.value.status == abi.KP_E_UNSUPPORTED and "in-flight NodeClaim capacity exceeded" in str(e.value)
        first = ctx.solve_plan()
        assert first["NCcap"] == 4096 and first["slice_hbm"] == 0, first
        # the next prepare, and only that one, plans for every pod
        ctx.prepare(iv)
        ctx.execute()
        dev = _fetch(ctx, prob)
        _assert_plan(case, ctx.solve_plan(), case.n_nodeclaims)
        parity.assert_same(dev, DC.run_oracle(case))
        got = parity.run_device(ctx, small)
        plan = ctx.solve_plan()
        assert plan["NCcap"] == 500 and plan["slice_hbm"] == 0 and plan["alloc_global"] == 0, plan
        parity.assert_same(got, parity.run_device(fresh, small))
    finally:
        ctx.close()
        fresh.close()
