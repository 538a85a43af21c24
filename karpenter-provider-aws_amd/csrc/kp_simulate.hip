// kp_simulate.hip — simulate_kernel: SimulateScheduling with up to KP_SIM_MAX_NODECLAIMS new NodeClaims (gfx950).
//
// Reference semantics ([core] sigs.k8s.io/karpenter pkg/controllers/disruption/helpers.go SimulateScheduling and
// provisioning/scheduling/scheduler.go Solve / add, recalled; DESIGN.md §4 "SimulateScheduling results"): the probe's
// pods (pending + its candidates' reschedulable pods) in queue order; each popped pod tries the existing nodes in
// scheduling order (the candidates removed), then the in-flight NodeClaims in sort.Slice(newNodeClaims, len(Pods))
// order, then the NodePool templates in weight order; a pod nothing takes is pushed back, and the queue ends when it
// cycles without progress (lastLen).  Drift and command validation need the Results of that simulation, not
// computeConsolidation's verdict, so unlike consolidate_kernel (kp_consolidate.hip) the probe does not stop at its second
// NodeClaim.
//
// One wave per probe, plainly serial: no window pass, no LDS node store, no chunk summaries.  The probe keeps its
// excluded candidates, modified-node bitmap and remaining NodePool limits in LDS, the requests it added to existing
// nodes in its delta slab, its queue in its ring, and its NodeClaims (requirements digest, options, requests, template)
// in its 12 entries of the nc_* slabs; the entry under evaluation is staged in LDS for eval_wave / eval_fits_only /
// merge_noop_at (kp_eval.h) and written back when the pod joins it.  finalize_kernel (kp_kernels.hip) then truncates
// the slabs' NodeClaims as it does a Solve's.
//
// A probe that reschedules a mutator's pod (kp_cons.h MUT, KpCons::mut_s / mut_m) applies ExistingNode.Add's requirement
// merge to its own copies of the nodes it changes, as consolidate_body's MUT instantiation does: a copy per changed node
// in the worker's ov_* slab, the changed nodes in an LDS bitmap, and class x node compatibility of such a node evaluated
// against its copy.
//
// TOPO (simulate_topo_kernel; a pass with topology groups, behind kp_device_opts::simulate_topology): as
// consolidate_body's TOPO instantiation, each probe keeps its own domain counts (ProbeTopo, kp_eval.h: the prepared base
// minus the pods it reschedules), with one hostname column per NodeClaim id (E + id) where consolidate_body has one for
// its only NodeClaim.  A pod of a constrained class (CF_TOPO_CONS) runs Topology.AddRequirements on every fitting node
// in order, on each in-flight NodeClaim and on the templates (host E + n_nc: no pod counted there); every placement of
// a counted class (CF_TOPO) is recorded.
//
// Not covered (the host refuses, kp_simulate_execute): reserved offerings, preference relaxation; and per
// probe (KP_SIM_UNSUPPORTED_PROBE): a probe that reschedules a pod with host ports or with claims on a limited CSI driver
// (their per-probe overlays are not modelled here).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kp_cons.h"
#include "kp_device.h"
#include "kp_eval.h"
#include "kp_layout.h"
#include "kp_sim.h"

namespace {

struct SimShared {
    ClassCache CC;
    WaveScratch ws;
    Roles roles;
    int64_t nc_req[KP_MAX_R];
};

__device__ __forceinline__ int32_t sld32(const int32_t* p) {
    return __hip_atomic_load(const_cast<int32_t*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint64_t sld64(const uint64_t* p) {
    return __hip_atomic_load(const_cast<uint64_t*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// this wave's stores have landed and its later loads see them (slab entries are written by some lanes, read by others)
__device__ __forceinline__ void sim_sync_mem() {
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
}

// types whose Capacity exceeds the probe's remaining NodePool limits (filterByRemainingResources); as
// kp_consolidate.hip's limit_filter_rem
__device__ inline uint64_t sim_limit_filter(const KpDev& d, int j, uint64_t o, const int64_t* rem, int lane) {
    bool any_limit = false;
    for (int r = 0; r < d.R; r++) any_limit |= d.limit_set[(size_t)j * d.R + r] != 0;
    if (!any_limit) return o;
    uint64_t out = 0;
    for (int w = 0; w < d.TW; w++) {
        const uint64_t cw = rl64(o, w);
        if (!cw) continue;
        const int t = w * 64 + lane;
        bool keep = (cw >> lane) & 1ull;
        if (keep) {
            for (int r = 0; r < d.R; r++)
                if (d.limit_set[(size_t)j * d.R + r] && d.cap[(size_t)r * d.T + t] > rem[j * d.R + r]) keep = false;
        }
        const uint64_t nb = ballot(keep);
        if (lane == w) out = nb;
    }
    return out;
}

}  // namespace

static_assert(KP_PT_SIM_COLS == KP_SIM_MAX_NODECLAIMS, "a hostname column per NodeClaim id");

// d / k / x: device copies of the launch's tables, read through const references (a by-value KpDev indexed dynamically
// goes to scratch per lane, see kp_consolidate.hip).  Block b runs probe k.probe0 + b of k.mode (SINGLE or MULTI) as
// worker b: one probe per worker, so the batch's slabs hold every probe's NodeClaims when the kernel ends.
template <bool TOPO>
__device__ __forceinline__ void simulate_body(const KpDev& d, const KpCons& k, const KpSim& x) {
    constexpr int CT = 2;  // kp_eval.h: a simulate probe's ProbeTopo
    extern __shared__ __attribute__((aligned(16))) char smem[];
    SimShared& S = *reinterpret_cast<SimShared*>(smem);
    ReqHdr* nch = reinterpret_cast<ReqHdr*>(smem + x.off_hdr);
    uint64_t* ncw = reinterpret_cast<uint64_t*>(smem + x.off_words);
    int64_t* rem = reinterpret_cast<int64_t*>(smem + x.off_rem);
    uint64_t* excl = reinterpret_cast<uint64_t*>(smem + x.off_excl);
    uint64_t* modb = reinterpret_cast<uint64_t*>(smem + x.off_mod);
    uint64_t* mutn = reinterpret_cast<uint64_t*>(smem + x.off_mutn);  // nodes whose requirements the probe changed
    const int lane = threadIdx.x;
    const int wid = blockIdx.x;
    if (wid >= k.n_probes) return;
    const int32_t* const pcls = d.pod_cls0 ? d.pod_cls0 : d.pod_cls;
    const int32_t* const pshape = d.pod_shape0 ? d.pod_shape0 : d.pod_shape;
    const int E = d.E, EW = d.EW, A = d.n_active, R = d.R, K = d.K, DW = d.DW, TW = d.TW, T = d.T, NT = d.NT;
    const int cap = k.ring_cap;
    ProbeTopo P{};
    if constexpr (TOPO) {
        P.cnt = x.pt_cnt + (size_t)wid * k.G * 64;
        P.known = x.pt_known + (size_t)wid * k.G;
        P.touched = reinterpret_cast<uint64_t*>(smem + x.off_touch);
        P.hd = x.pt_hd + (size_t)wid * (k.HG > 0 ? k.HG : 1) * (E + KP_PT_SIM_COLS);
        P.hmod = reinterpret_cast<uint64_t*>(smem + x.off_hmod);
        P.dgk = k.pt_dgk;
        P.hpos = reinterpret_cast<int32_t*>(smem + x.off_hpos);
        P.ha = k.tg_ha;
        P.born = reinterpret_cast<uint64_t*>(smem + x.off_born);
        P.excl = excl;
        P.E = E;
        P.HG = k.HG;
    }
    int32_t* ring = k.ring + (size_t)wid * cap;
    int32_t* rlast = k.ring_last + (size_t)wid * cap;
    int64_t* delta = k.delta + (size_t)wid * (A > 0 ? A : 1) * (E > 0 ? E : 1);
    uint64_t* pbits = k.pbits + (size_t)wid * k.PW;
    int32_t* plog = x.log + (size_t)wid * cap * 2;
    int32_t* const ov_slot = x.ov_slot + (size_t)wid * (E > 0 ? E : 1);
    ReqHdr* const ov_hdr = x.ov_hdr + (size_t)wid * x.ov_cap * K;
    uint64_t* const ov_words = x.ov_words + (size_t)wid * x.ov_cap * DW;
    // this worker's slab entries, NodeClaim-major over the batch (entry of NodeClaim i: i * workers + worker), so the
    // NodeClaims the batch created lie in the first max-count * workers entries and finalize_kernel runs over those alone
    const size_t nwk = (size_t)k.n_probes;
    auto ent_of = [&](int i) -> size_t { return (size_t)i * nwk + (size_t)wid; };

    const bool single = k.mode == KP_CONSOLIDATE_SINGLE;
    const int gp = k.probe0 + wid;
    const int c0 = single ? gp : 0, c1 = single ? gp + 1 : gp + 2;

    // a worker's unused slab entries must read as empty NodeClaims to finalize_kernel
    auto clear_entries = [&](int from) {
        for (int i = from; i < KP_SIM_MAX_NODECLAIMS; i++) {
            const size_t e = ent_of(i);
            if (lane < TW) d.nc_opts[e * TW + lane] = 0ull;
            if (lane < R) d.nc_req[e * R + lane] = 0;
            if (lane == 0) {
                d.nc_tmpl[e] = 0;
                d.nc_npods[e] = 0;
                d.nc_slice_pos[e] = -1;
                x.nc_nonpend[e] = 0;
            }
        }
    };
    // a MUT probe (kp_cons.h): ExistingNode.Add's requirement merge may change a node in a way a later pod sees
    const bool mutp = k.mut && __builtin_amdgcn_readfirstlane(single ? k.mut_s[gp] : k.mut_m[gp]) != 0;
    int n_ov = 0;  // node digest copies taken by this probe

    if (lane < 5) {
        const int rk = lane == 0 ? d.key_zone : lane == 1 ? d.key_ct : lane == 2 ? d.key_zoneid : lane == 3 ? d.key_resvid : d.key_resvtype;
        S.roles.key[lane] = rk;
        S.roles.woff[lane] = rk >= 0 ? d.woff[rk] : 0;
        S.roles.nw[lane] = rk >= 0 ? d.nw[rk] : 0;
    }
    if (lane == 0) S.CC.cls = -1;
    for (int w = lane; w < EW; w += 64) {
        excl[w] = 0;
        modb[w] = 0;
        mutn[w] = 0;
    }
    for (int i = lane; i < NT * R; i += 64) rem[i] = d.remaining[i];
    __syncthreads();
    EvalEnv Ev;
    Ev.alloc = k.alloc_act;
    Ev.astride = k.astride;
    Ev.avail = d.avail_zc;
    Ev.multi16 = nullptr;
    Ev.slot_zone = d.slot_zone;
    Ev.slot_ct = d.slot_ct;
    Ev.slot_zoneid = d.slot_zoneid;
    Ev.roles = &S.roles;
    {
        uint64_t mmask = 0;  // templates whose requirements carry minValues
        for (int j = 0; j < NT; j++)
            if (d.min_keys[(size_t)j * KP_MAX_CLASS_KEYS] >= 0) mmask |= 1ull << j;
        Ev.min_tmpl_mask = mmask;
    }
    Ev.ro = nullptr;
    Ev.type_ro = nullptr;
    Ev.rcap = nullptr;
    Ev.resv_on = 0;
    Ev.pt = TOPO ? &P : nullptr;
    Ev.snap = nullptr;

    // ---- probe state: excluded candidates, NodePool limits + the candidates' capacity ----
    for (int c = c0 + lane; c < c1; c += 64) {
        const int node = k.cand_i[c * 4 + 0];
        if (node >= 0 && node < E) atomicOr((unsigned long long*)&excl[node >> 6], 1ull << (node & 63));
        const int tj = k.cand_i[c * 4 + 3];
        if (tj >= 0 && tj < NT)
            for (int r = 0; r < R; r++)
                if (d.limit_set[(size_t)tj * R + r])
                    atomicAdd((unsigned long long*)&rem[tj * R + r], (unsigned long long)k.cand_cap[(size_t)c * R + r]);
    }
    __syncthreads();
    if constexpr (TOPO) {
        // this probe's NewTopology: no row copied yet, no node column of its own, every NodeClaim column empty; then the
        // pods it reschedules come off the base counts
        for (int w = lane; w < ((k.G + 63) >> 6); w += 64) P.touched[w] = 0;
        for (int w = lane; w < EW; w += 64) P.hmod[w] = 0;
        for (int i = lane; i < k.HG * KP_PT_SIM_COLS; i += 64)
            __hip_atomic_store(&P.hd[(size_t)(i / KP_PT_SIM_COLS) * (E + KP_PT_SIM_COLS) + E + i % KP_PT_SIM_COLS], 0,
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        const int r0 = single ? k.dec_soff[gp] : k.dec_moff[gp], r1 = single ? k.dec_soff[gp + 1] : k.dec_moff[gp + 1];
        for (int r = r0; r < r1; r++) {
            const int g = k.dec_g[r];
            if (g >= 0 && g < k.G) pt_init_row(d, P, g, k.dec_v + (size_t)r * 64, lane);
        }
        for (int ga = lane; ga < k.n_ha; ga += 64) P.hpos[ga] = k.hpos0[(size_t)(single ? gp : k.n_cand + gp) * k.n_ha + ga];
        if (lane == 0) {
            *P.born = k.born_s ? (single ? k.born_s[gp] : k.born_m[gp]) : ~0ull;
            if (d.late_sib) S.CC.cls = -1;  // the class caches route variant groups by this probe's births
        }
        sim_sync_mem();
        __syncthreads();
    }

    // ---- the probe's pods in queue order: mark queue positions, then scan the bitmap with the pending pods ----
    const int po0 = k.cand_off[c0], po1 = k.cand_off[c1];
    const int n_np = po1 - po0;
    int n = 0;
    for (int i = po0 + lane; i < po1; i += 64) {
        const int r = k.rank[k.cand_pods[i]];
        __hip_atomic_fetch_or(&pbits[r >> 6], 1ull << (r & 63), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    sim_sync_mem();
    for (int wb = 0; wb < k.PW; wb += 64) {
        const int w = wb + lane;
        const uint64_t mine = w < k.PW ? sld64(&pbits[w]) : 0ull;
        const uint64_t pend = (w < k.PW && k.n_pending) ? k.pend_bits[w] : 0ull;
        uint64_t xb = mine | pend;
        if (!ballot(xb != 0)) continue;
        const int cnt = __popcll(xb);
        const int v = (int)wave_scan_add32((uint32_t)cnt);
        const int total = __builtin_amdgcn_readlane(v, 63);
        int pos = n + v - cnt;
        while (xb) {
            const int b = __ffsll((unsigned long long)xb) - 1;
            xb &= xb - 1;
            if (pos < cap) {
                ring[pos] = d.queue0[w * 64 + b] | (int32_t)(((pend >> b) & 1ull) << 31);
                rlast[pos] = -1;
            }
            pos++;
        }
        if (mine) __hip_atomic_store(&pbits[w], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        n += total;
    }
    sim_sync_mem();
    __syncthreads();

    int status = KP_SIM_OK;
    bool bad = false;
    // a pod with host ports or with claims on a limited driver keeps per-probe node state this kernel does not model:
    // the probe is refused, never approximated
    if (mutp && (d.PW > 0 || d.VD > 0) && n <= cap) {
        bool hit = false;
        for (int i = lane; i < n; i += 64) {
            const int p = sld32(&ring[i]) & 0x3fffffff;
            if (p < d.P) {
                if (d.PW > 0 && (d.cls_flags[pcls[p]] & CF_PORTS)) hit = true;
                if (d.VD > 0 && d.shape_vs[pshape[p]] != 0) hit = true;
            }
        }
        if (ballot(hit)) {
            clear_entries(0);
            if (lane == 0) {
                KpSimRow o{};
                o.status = KP_SIM_UNSUPPORTED_PROBE;
                x.rows[wid] = o;
                x.n_log[wid] = 0;
            }
            return;
        }
    }
    if (n > cap) {  // the host sizes the ring by the probe's pods: a longer queue is an error, not an overrun
        if (lane == 0) atomicExch(x.err, 2);
        n = 0;
        bad = true;
    }

    // ---- Solve ----
    // slice state, one lane per slice position: the NodeClaim there and its pod count; by NodeClaim id (lane = id):
    // its template, the class it last absorbed, its non-pending pods
    int sl_nc = -1, sl_cnt = 0;
    int id_tmpl = -1, id_lc = -1, id_np = 0;
    int n_nc = 0, staged = -1, ok_np = 0, placements = 0;
    uint64_t nc_opts = 0;  // lane w < TW: option word w of the staged NodeClaim
    int prev_shape = -1, xstart = 0;
    int64_t st_pops = 0, st_nc = 0, st_tmpl = 0;
    // Queue.Pop runs at most once per pod between two placements plus one full cycle: a larger count means the ring or
    // its lastLen entries are inconsistent (an internal error, never a hang)
    const int64_t pop_bound = (int64_t)n * ((int64_t)n + 2) + 8;

    auto stage = [&](int id) {
        const size_t e = ent_of(id);
        for (int kk = lane; kk < K; kk += 64) {
            const uint64_t* src = reinterpret_cast<const uint64_t*>(d.nc_hdr + e * K + kk);
            uint64_t* dst = reinterpret_cast<uint64_t*>(nch + kk);
            dst[0] = sld64(src);
            dst[1] = sld64(src + 1);
            dst[2] = sld64(src + 2);
        }
        for (int i = lane; i < DW; i += 64) ncw[i] = sld64(&d.nc_words[e * DW + i]);
        if (lane < R) S.nc_req[lane] = ld_req(&d.nc_req[e * R + lane]);
        nc_opts = lane < TW ? sld64(&d.nc_opts[e * TW + lane]) : 0ull;
        staged = id;
        __syncthreads();
    };
    auto write_back = [&](int id) {
        const size_t e = ent_of(id);
        for (int kk = lane; kk < K; kk += 64) d.nc_hdr[e * K + kk] = nch[kk];
        for (int i = lane; i < DW; i += 64) d.nc_words[e * DW + i] = ncw[i];
        if (lane < R) d.nc_req[e * R + lane] = S.nc_req[lane];
        if (lane < TW) d.nc_opts[e * TW + lane] = nc_opts;
        sim_sync_mem();
    };
    auto log_place = [&](int pod, int res) {
        if (lane == 0 && placements < cap) {
            plog[placements * 2 + 0] = pod;
            plog[placements * 2 + 1] = res;
        }
        placements++;
    };

    int head = 0, count = n;
    while (count > 0) {
        head = __builtin_amdgcn_readfirstlane(head);
        count = __builtin_amdgcn_readfirstlane(count);
        n_nc = __builtin_amdgcn_readfirstlane(n_nc);
        staged = __builtin_amdgcn_readfirstlane(staged);
        xstart = __builtin_amdgcn_readfirstlane(xstart);
        prev_shape = __builtin_amdgcn_readfirstlane(prev_shape);
        if (st_pops >= pop_bound) {
            if (lane == 0) atomicExch(x.err, 2);
            bad = true;
            break;
        }
        const int slot = head % cap;
        const int ent = __builtin_amdgcn_readfirstlane(sld32(&ring[slot]));
        const int elast = __builtin_amdgcn_readfirstlane(sld32(&rlast[slot]));
        if (elast == count) break;  // Queue.Pop: cycled through the queue without progress
        head++;
        count--;
        st_pops++;
        const bool pend = ent < 0;
        const int p = ent & 0x3fffffff;
        if (p >= d.P) {  // a corrupt queue entry
            if (lane == 0) atomicExch(x.err, 2);
            bad = true;
            break;
        }
        const int c = __builtin_amdgcn_readfirstlane(pcls[p]);
        const int shape = __builtin_amdgcn_readfirstlane(pshape[p]);
        const int64_t* preq = d.pod_req + (size_t)p * R;
        if (shape != prev_shape) {  // nodes before xstart rejected this shape and only lose headroom
            prev_shape = shape;
            xstart = 0;
        }
        // TOPO: a class counted by some group records each placement; a constrained class's node rejections depend on
        // counts (scan from the first node, no resume)
        uint32_t cflags = 0;
        if constexpr (TOPO) {
            cflags = __builtin_amdgcn_readfirstlane(d.cls_flags[c]);
            if ((cflags & CF_TOPO) && S.CC.cls != c) fill_class_cache<true>(d, c, S.CC, lane, 64, *P.born);
        }
        const bool ctopo = TOPO && (cflags & CF_TOPO);
        const bool tcons = TOPO && (cflags & CF_TOPO_CONS);
        const int xs = tcons ? 0 : xstart;
        // MUT: the requirements digest of node j as this probe sees it (its copy once a merge changed it)
        auto node_digest = [&](int j, const ReqHdr*& h, const uint64_t*& w) {
            h = d.ex_hdr + (size_t)j * K;
            w = d.ex_words + (size_t)j * DW;
            if (mutp && ((mutn[j >> 6] >> (j & 63)) & 1ull)) {
                const int sl = __builtin_amdgcn_readfirstlane(sld32(&ov_slot[j]));
                h = ov_hdr + (size_t)sl * K;
                w = ov_words + (size_t)sl * DW;
            }
        };

        // ---- 1. ExistingNode.Add: first fit in scheduling order, 64 nodes per ballot ----
        int jf = -1;
        for (int base = xs & ~63; base < E; base += 64) {
            const int w = base >> 6;
            const int j = base + lane;
            const uint64_t ge = xs > base ? (~0ull << (xs - base)) : ~0ull;
            uint64_t xw = d.XT[(size_t)c * EW + w] & ~excl[w];
            if (mutp) {
                // the nodes this probe changed, re-evaluated against their copies: taints tolerated, static fit,
                // Requirements.Compatible(node copy, class)
                const uint64_t mw = mutn[w] & ~excl[w];
                if (mw) {
                    bool okc = false;
                    if ((mw >> lane) & 1ull) {
                        const int sl = sld32(&ov_slot[j]);
                        okc = d.ex_static[j] && ((d.ex_tol[(size_t)c * EW + w] >> lane) & 1ull) &&
                              node_compatible(d, ov_hdr + (size_t)sl * K, ov_words + (size_t)sl * DW, c);
                    }
                    xw = (xw & ~mw) | ballot(okc);
                }
            }
            xw &= ge;
            if (!xw) continue;
            const uint64_t mw = modb[w];
            bool cand = j < E && ((xw >> lane) & 1ull);
            const bool md = (mw >> lane) & 1ull;
            for (int ai = 0; ai < A && ballot(cand); ai++) {
                if (cand) {
                    int64_t h = d.ex_head[(size_t)ai * E + j];
                    if (md) h -= ld_req(&delta[(size_t)ai * E + j]);
                    cand = preq[d.active_axes[ai]] <= h;
                }
            }
            uint64_t m = ballot(cand);
            if constexpr (TOPO) {
                if (tcons) {  // ExistingNode.Add's topology step on each fitting node, in order (at most 64 per word)
                    while (m) {
                        const int jj = __builtin_amdgcn_readfirstlane(base + __ffsll((unsigned long long)m) - 1);
                        const ReqHdr* nh;
                        const uint64_t* nwd;
                        node_digest(jj, nh, nwd);
                        if (existing_topo_try<true, CT>(d, S.CC, S.ws, jj, lane, &P, nh, nwd)) break;
                        m &= m - 1;
                    }
                }
            }
            if (m) {
                jf = base + __ffsll((unsigned long long)m) - 1;
                break;
            }
        }
        jf = __builtin_amdgcn_readfirstlane(jf);
        if (jf >= 0) {
            // the node's requests within this probe: the delta slab, valid once its bit of modb is set
            const bool was = (modb[jf >> 6] >> (jf & 63)) & 1ull;
            for (int ai = lane; ai < A; ai += 64) {
                int64_t* dq = &delta[(size_t)ai * E + jf];
                __hip_atomic_store(dq, (was ? ld_req(dq) : 0) + preq[d.active_axes[ai]], __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
            }
            __syncthreads();
            if (lane == 0) modb[jf >> 6] |= 1ull << (jf & 63);
            sim_sync_mem();
            __syncthreads();
            if constexpr (TOPO) {
                if (ctopo) {  // Topology.Record with the node's merged requirements and taints
                    const ReqHdr* nh;
                    const uint64_t* nwd;
                    node_digest(jf, nh, nwd);
                    if (!tcons) existing_topo_try<false, CT>(d, S.CC, S.ws, jf, lane, &P, nh, nwd);
                    topo_record<CT>(d, S.CC, S.ws, nh, nwd, jf, -1, false, lane, jf, &P);
                }
            }
            if (mutp) {
                // ExistingNode.Add: nodeRequirements.Add(pod requirements).  A node's labels are single values that a
                // compatible merge keeps, so only a class key the node lacks can change it: the first such merge copies
                // the node's digest
                int sl = -1;
                if (!((mutn[jf >> 6] >> (jf & 63)) & 1ull)) {
                    bool ch = false;
                    for (int i = d.cls_xkoff[c] + lane; i < d.cls_xkoff[c + 1]; i += 64)
                        ch |= !(d.ex_hdr[(size_t)jf * K + d.cls_xkeys[i]].flags & RF_DEF);
                    if (ballot(ch)) {
                        if (n_ov >= x.ov_cap) {  // sized by the probe's pods: cannot happen
                            if (lane == 0) atomicExch(x.err, 2);
                            bad = true;
                            break;
                        }
                        sl = n_ov++;
                        for (int i = lane; i < K; i += 64) ov_hdr[(size_t)sl * K + i] = d.ex_hdr[(size_t)jf * K + i];
                        for (int i = lane; i < DW; i += 64) ov_words[(size_t)sl * DW + i] = d.ex_words[(size_t)jf * DW + i];
                        if (lane == 0) {
                            __hip_atomic_store(&ov_slot[jf], sl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            mutn[jf >> 6] |= 1ull << (jf & 63);
                        }
                        sim_sync_mem();
                        __syncthreads();
                    }
                } else {
                    sl = __builtin_amdgcn_readfirstlane(sld32(&ov_slot[jf]));
                }
                if (sl >= 0) {
                    ReqHdr* nh = ov_hdr + (size_t)sl * K;
                    uint64_t* nwd = ov_words + (size_t)sl * DW;
                    if (ctopo) {  // ... then .Add(topology requirements): ws holds the merged class keys
                        if (lane < S.CC.nck) {
                            const int kk = S.CC.key[lane];
                            nh[kk] = S.ws.hdr[lane];
                            for (int i = 0; i < S.CC.nw[lane]; i++) nwd[S.CC.woff[lane] + i] = S.ws.words[S.CC.wsoff[lane] + i];
                        }
                    } else {
                        for (int i = d.cls_xkoff[c] + lane; i < d.cls_xkoff[c + 1]; i += 64) {
                            const int kk = d.cls_xkeys[i];
                            ReqHdr a = nh[kk];
                            req_merge_inplace(d, kk, a, nwd + d.woff[kk], d.cls_hdr[(size_t)c * K + kk],
                                              d.cls_words + (size_t)c * DW + d.woff[kk]);
                            nh[kk] = a;
                        }
                    }
                    sim_sync_mem();
                }
            }
            if (!tcons) xstart = jf;
            if (!pend) {
                // SimulateScheduling: a non-pending pod on an uninitialized node is an error
                // (the pod has a place all the same: it is not among the unscheduled)
                ok_np++;
                if (!((k.init_bits[jf >> 6] >> (jf & 63)) & 1ull)) bad = true;
            }
            log_place(p, -2 - jf);
            continue;
        }
        if (!tcons) xstart = E;

        // ---- 2. the in-flight NodeClaims in sort.Slice(newNodeClaims, len(Pods)) order ----
        // at most 12 elements: Go's pdqsort_func is insertionSort, a stable sort of the slice as the last sort left it
        if (n_nc > 1) {
            int rank = 0;
            for (int q = 0; q < n_nc; q++) {
                const int cq = rl32(sl_cnt, q);
                rank += (cq < sl_cnt || (cq == sl_cnt && q < lane)) ? 1 : 0;
            }
            int nnc = sl_nc, ncnt = sl_cnt;
            for (int q = 0; q < n_nc; q++) {
                const int rq = rl32(rank, q);
                const int a = rl32(sl_nc, q), b = rl32(sl_cnt, q);
                if (lane == rq) {
                    nnc = a;
                    ncnt = b;
                }
            }
            if (lane < n_nc) {
                sl_nc = nnc;
                sl_cnt = ncnt;
            }
        }
        bool placed = false;
        for (int pos = 0; pos < n_nc && !placed; pos++) {
            const int id = __builtin_amdgcn_readfirstlane(__shfl(sl_nc, pos));
            const int tj = __builtin_amdgcn_readfirstlane(__shfl(id_tmpl, id));
            const int lc = __builtin_amdgcn_readfirstlane(__shfl(id_lc, id));
            if (staged != id) stage(id);
            if (S.CC.cls != c) fill_class_cache<TOPO>(d, c, S.CC, lane, 64, TOPO ? *P.born : 0ull);
            EvalIn a;
            a.Ahdr = nch;
            a.Aw = ncw;
            a.opts = nc_opts;
            a.base_req = S.nc_req;
            a.pod_req = preq;
            a.tmpl = tj;
            a.compat = true;
            a.force_off = false;
            a.prof = nullptr;
            a.host = TOPO ? E + id : E;  // the NodeClaim's hostname column
            a.held = 0;
            st_nc++;
            // the NodeClaim has absorbed the class, or the class's requirement merge changes nothing: Fits (+ minValues);
            // never for a class some topology group counts or constrains
            bool absorbed = c == lc && !ctopo;
            if (!absorbed && !ctopo && ((d.tol[c] >> tj) & 1ull) && merge_noop_at(d, S.ws, nch, ncw, c, lane)) absorbed = true;
            bool ok;
            if (absorbed) {
                ok = eval_fits_only<true>(d, Ev, a, S.ws, lane);
            } else {
                if constexpr (TOPO)
                    ok = tcons ? eval_wave<true, false, false, true, CT>(d, Ev, S.CC, a, S.ws, lane)
                               : eval_wave<false, false, false>(d, Ev, S.CC, a, S.ws, lane);
                else
                    ok = eval_wave<false, false, false>(d, Ev, S.CC, a, S.ws, lane);
                if (ok && lane < S.CC.nck) {
                    const int kk = S.CC.key[lane];
                    nch[kk] = S.ws.hdr[lane];
                    for (int i = 0; i < S.CC.nw[lane]; i++) ncw[S.CC.woff[lane] + i] = S.ws.words[S.CC.wsoff[lane] + i];
                }
            }
            if (!ok) continue;
            nc_opts = lane < TW ? S.ws.opts[lane] : 0ull;
            if (lane < R) S.nc_req[lane] += preq[lane];
            __syncthreads();
            if (d.best_effort) {  // the Add's relaxed minValues
                if (lane < S.ws.n_minrel) nch[S.ws.minrel_k[lane]].minv = S.ws.minrel_v[lane];
                __syncthreads();
            }
            write_back(id);
            if constexpr (TOPO)
                if (ctopo) topo_record<CT>(d, S.CC, S.ws, nch, ncw, E + id, tj, true, lane, -1, &P);
            if (lane == id) {
                id_lc = c;
                if (!pend) id_np++;
            }
            if (lane == pos) sl_cnt++;
            if (!pend) ok_np++;
            log_place(p, id);
            placed = true;
        }
        if (placed) continue;

        // ---- 3. a new NodeClaim from the templates in weight order ----
        bool overflow = false;
        for (int j = 0; j < NT && !placed; j++) {
            uint64_t o = (lane < TW && d.tmpl_ok[j]) ? d.tmpl_opts[(size_t)j * TW + lane] : 0ull;
            o = sim_limit_filter(d, j, o, rem, lane);
            if (!ballot(o != 0)) continue;
            if (S.CC.cls != c) fill_class_cache<TOPO>(d, c, S.CC, lane, 64, TOPO ? *P.born : 0ull);
            EvalIn a;
            a.Ahdr = d.cls_hdr + (size_t)(d.C + j) * K;
            a.Aw = d.cls_words + (size_t)(d.C + j) * DW;
            a.opts = o;
            a.base_req = d.daemon + (size_t)j * R;
            a.pod_req = preq;
            a.tmpl = j;
            a.compat = true;
            a.force_off = false;
            a.prof = nullptr;
            // a new NodeClaim's hostname: no pod counted there yet (TOPO: the next id's column; with 12 in flight it lies
            // past the row and reads as empty)
            a.host = TOPO ? E + n_nc : E + 1;
            a.held = 0;
            st_tmpl++;
            if constexpr (TOPO) {
                if (!(tcons ? eval_wave<true, false, false, true, CT>(d, Ev, S.CC, a, S.ws, lane)
                            : eval_wave<false, false, false>(d, Ev, S.CC, a, S.ws, lane)))
                    continue;
            } else {
                if (!eval_wave<false, false, false>(d, Ev, S.CC, a, S.ws, lane)) continue;
            }
            if (n_nc >= KP_SIM_MAX_NODECLAIMS) {  // a thirteenth NodeClaim: the slice sort would no longer be insertionSort
                overflow = true;
                break;
            }
            const int id = n_nc;
            for (int kk = lane; kk < K; kk += 64) nch[kk] = d.cls_hdr[(size_t)(d.C + j) * K + kk];
            for (int i = lane; i < DW; i += 64) ncw[i] = d.cls_words[(size_t)(d.C + j) * DW + i];
            __syncthreads();
            if (lane < S.CC.nck) {
                const int kk = S.CC.key[lane];
                nch[kk] = S.ws.hdr[lane];
                for (int i = 0; i < S.CC.nw[lane]; i++) ncw[S.CC.woff[lane] + i] = S.ws.words[S.CC.wsoff[lane] + i];
            }
            nc_opts = lane < TW ? S.ws.opts[lane] : 0ull;
            if (lane < R) S.nc_req[lane] = d.daemon[(size_t)j * R + lane] + preq[lane];
            __syncthreads();
            // subtractMax(remaining, nodeClaim.InstanceTypeOptions)
            for (int r = 0; r < R; r++) {
                if (!d.limit_set[(size_t)j * R + r]) continue;
                int64_t mx = INT64_MIN;
                for (int w = 0; w < TW; w++) {
                    const uint64_t ow = rl64(nc_opts, w);
                    if ((ow >> lane) & 1ull) {
                        const int64_t cp = d.cap[(size_t)r * T + w * 64 + lane];
                        mx = cp > mx ? cp : mx;
                    }
                }
                mx = wave_max64(mx);
                if (lane == 0) rem[j * R + r] -= mx;
            }
            __syncthreads();
            if (d.best_effort) {
                if (lane < S.ws.n_minrel) nch[S.ws.minrel_k[lane]].minv = S.ws.minrel_v[lane];
                __syncthreads();
            }
            staged = id;
            write_back(id);
            if constexpr (TOPO) {  // the NodeClaim's hostname column starts empty; Record the pod
                for (int r = lane; r < k.HG; r += 64)
                    __hip_atomic_store(&P.hd[(size_t)r * (E + KP_PT_SIM_COLS) + E + id], 0, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                if (ctopo) topo_record<CT>(d, S.CC, S.ws, nch, ncw, E + id, j, true, lane, -1, &P);
            }
            if (lane == 0) d.nc_tmpl[ent_of(id)] = j;
            if (lane == id) {
                id_tmpl = j;
                id_lc = c;
                id_np = pend ? 0 : 1;
                sl_nc = id;  // append(s.newNodeClaims, nodeClaim): slice position = count so far = id
                sl_cnt = 1;
            }
            n_nc++;
            if (!pend) ok_np++;
            log_place(p, id);
            placed = true;
        }
        if (overflow) {
            status = KP_SIM_NODECLAIM_OVERFLOW;
            break;
        }
        if (placed) continue;

        // ---- Queue.Push(pod, relaxed = false): lastLen = len after the append ----
        const int tail = head + count;
        if (lane == 0) {
            __hip_atomic_store(&ring[tail % cap], ent, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&rlast[tail % cap], count + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        count++;
        sim_sync_mem();
    }

    // ---- results: the slice positions and pod counts of the NodeClaims, the row ----
    n_nc = __builtin_amdgcn_readfirstlane(n_nc);
    if (status != KP_SIM_OK) n_nc = 0;
    if (lane < n_nc) {
        d.nc_npods[ent_of(sl_nc)] = sl_cnt;
        d.nc_slice_pos[ent_of(sl_nc)] = lane;
        x.nc_nonpend[ent_of(lane)] = id_np;
    }
    clear_entries(n_nc);
    if (lane == 0) {
        KpSimRow o{};
        o.status = status;
        if (status == KP_SIM_OK) {
            o.bad = bad ? 1 : 0;
            o.n_nc = n_nc;
            o.n_pods = n;
            o.n_np = n_np;
            o.ok_np = ok_np;
        }
        x.rows[wid] = o;
        x.n_log[wid] = status == KP_SIM_OK ? (placements < cap ? placements : cap) : 0;
        atomicAdd((unsigned long long*)&x.stats[SS_POPS], (unsigned long long)st_pops);
        atomicAdd((unsigned long long*)&x.stats[SS_NC_EVALS], (unsigned long long)st_nc);
        atomicAdd((unsigned long long*)&x.stats[SS_TMPL_EVALS], (unsigned long long)st_tmpl);
        atomicAdd((unsigned long long*)&x.stats[SS_PROBES], 1ull);
    }
}

__global__ __launch_bounds__(64) void simulate_kernel(const KpDev* __restrict__ dp, const KpCons* __restrict__ kp,
                                                      const KpSim* __restrict__ xp) {
    simulate_body<false>(*dp, *kp, *xp);
}
// the same over a pass with topology groups (a ProbeTopo per worker)
__global__ __launch_bounds__(64) void simulate_topo_kernel(const KpDev* __restrict__ dp, const KpCons* __restrict__ kp,
                                                           const KpSim* __restrict__ xp) {
    simulate_body<true>(*dp, *kp, *xp);
}

// Dynamic LDS of simulate_kernel: fixed block, the staged NodeClaim digest, limits, candidate / modified-node bitmaps.
// G > 0: a pass with topology groups (n_ha of them hostname pod affinities).
bool kp_sim_plan_lds(const KpDev& d, KpSim& x, int max_bytes, int G, int n_ha) {
    auto al = [](size_t v) { return (v + 15) & ~(size_t)15; };
    size_t off = al(sizeof(SimShared));
    x.off_hdr = (int)off;
    off = al(off + sizeof(ReqHdr) * (size_t)(d.K > 0 ? d.K : 1));
    x.off_words = (int)off;
    off = al(off + 8 * (size_t)(d.DW > 0 ? d.DW : 1));
    x.off_rem = (int)off;
    off = al(off + 8 * (size_t)(d.NT * d.R > 0 ? d.NT * d.R : 1));
    x.off_excl = (int)off;
    off = al(off + 8 * (size_t)(d.EW > 0 ? d.EW : 1));
    x.off_mod = (int)off;
    off = al(off + 8 * (size_t)(d.EW > 0 ? d.EW : 1));
    x.off_mutn = (int)off;
    off = al(off + 8 * (size_t)(d.EW > 0 ? d.EW : 1));
    x.off_touch = x.off_hmod = x.off_hpos = x.off_born = 0;
    if (G > 0) {  // simulate_topo_kernel's ProbeTopo words
        x.off_touch = (int)off;
        off = al(off + 8 * (size_t)((G + 63) / 64));
        x.off_hmod = (int)off;
        off = al(off + 8 * (size_t)(d.EW > 0 ? d.EW : 1));
        x.off_hpos = (int)off;
        off = al(off + 4 * (size_t)(n_ha > 0 ? n_ha : 1));
        x.off_born = (int)off;
        off = al(off + 8);
    }
    x.lds_bytes = (int)off;
    return (int)off <= max_bytes;
}

hipError_t kp_launch_simulate(const KpCons& k, const KpSim& x, hipStream_t s, const KpDev* d_dev, const KpCons* d_k,
                              const KpSim* d_x) {
    if (k.n_probes <= 0) return hipSuccess;
    const void* fn = k.G > 0 ? (const void*)simulate_topo_kernel : (const void*)simulate_kernel;
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, KP_LDS_BYTES);
    if (e != hipSuccess) return e;
    if (k.G > 0)
        hipLaunchKernelGGL(simulate_topo_kernel, dim3(k.n_probes), dim3(64), (size_t)x.lds_bytes, s, d_dev, d_k, d_x);
    else
        hipLaunchKernelGGL(simulate_kernel, dim3(k.n_probes), dim3(64), (size_t)x.lds_bytes, s, d_dev, d_k, d_x);
    return hipGetLastError();
}
