// kp_explain.hip — explain_kernel: why a new NodeClaim of each NodePool refuses an unschedulable pod (gfx950).
//
// One wave per (distinct unschedulable shape, template), read-only over the state the Solve kernels leave in HBM.  The
// wave restates the template evaluation of eval_wave (kp_eval.h) as a diagnosis: the same stages in core's order
// ([core] scheduling/scheduler.go add, nodeclaim.go Add), each reported instead of short-circuited, and the instance
// type filter as filterResults keeps it (three criteria per type, their pairs, and counts).  DESIGN.md §4
// "Explanations"; the rows are kp_explain.h's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kp_eval.h"
#include "kp_explain.h"

static __device__ __forceinline__ int wave_sum_i32(int x) {
    return (int)wave_reduce32((uint32_t)x, [](uint32_t a, uint32_t b) { return a + b; });
}

// TOPO: the solve has topology groups (classes under CF_TOPO_CONS run Topology.AddRequirements between the requirement
// merge and the type sweep, and keys carried only for narrowing merge as the template's requirement).
template <bool TOPO>
__global__ __launch_bounds__(64) void explain_kernel(KpDev d, KpExplain x) {
    __shared__ ClassCache CC;
    __shared__ WaveScratch ws;
    __shared__ Roles roles;
    const int s = blockIdx.x, j = blockIdx.y, lane = threadIdx.x;
    if (s >= x.n_shapes || j >= d.NT) return;
    const int pod = x.rep[s];
    const int c = d.pod_cls[pod];  // the pod's final relaxation stage
    const int TW = d.TW, T = d.T, R = d.R;
    fill_class_cache<TOPO>(d, c, CC, lane, 64, x.born);
    if (lane < 5) {
        const int rk = lane == 0 ? d.key_zone : lane == 1 ? d.key_ct : lane == 2 ? d.key_zoneid : lane == 3 ? d.key_resvid : d.key_resvtype;
        roles.key[lane] = rk;
        roles.woff[lane] = rk >= 0 ? d.woff[rk] : 0;
        roles.nw[lane] = rk >= 0 ? d.nw[rk] : 0;
    }
    __syncthreads();

    KpExplainRow row{};
    auto finish = [&](int reason) {
        row.reason = reason;
        if (lane == 0) x.rows[(size_t)s * d.NT + j] = row;
    };

    // ---- 1. filterByRemainingResources: the template's options whose capacity is within the remaining limits ----
    // (recomputed from KpDev.remaining as the Solve left it; tmpl_lmask is the FFD kernel's scratch)
    const uint64_t tmpl_o = (lane < TW && d.tmpl_ok[j]) ? d.tmpl_opts[(size_t)j * TW + lane] : 0ull;
    uint32_t lm = 0;
    for (int r = 0; r < R; r++)
        if (d.limit_set[(size_t)j * R + r]) lm |= 1u << r;
    uint64_t lmask = ~0ull;
    for (int w = 0; w < TW && lm; w++) {
        const int t = w * 64 + lane;
        bool keep = t < T;
        for (uint32_t m = lm; m && keep; m &= m - 1) {
            const int r = __ffs(m) - 1;
            keep = d.cap[(size_t)r * T + t] <= d.remaining[(size_t)j * R + r];
        }
        const uint64_t nb = ballot(keep);
        if (lane == w) lmask = nb;
    }
    const uint64_t opts = tmpl_o & lmask;  // lane w < TW: option word w
    row.n_options = wave_sum_i32(__popcll(opts));
    if (ballot(tmpl_o != 0) && !ballot(opts != 0)) return finish(KPX_LIMITS);

    // ---- 2. taints, 3. host ports of the template's daemonsets ----
    // (x.tol, not CC.tol: KpDev.tol is also cleared by a hostname requirement, which belongs to stage 4)
    if (!((x.tol[c] >> j) & 1ull)) return finish(KPX_TAINTS);
    if (d.PW > 0 && (CC.flags & CF_PORTS)) {
        uint64_t hit = 0;
        for (int w = 0; w < d.PW; w++) hit |= d.tmpl_ports[(size_t)j * d.PW + w] & d.cls_ports[(size_t)c * d.PW + w];
        if (hit) return finish(KPX_HOST_PORTS);
    }

    // ---- 4. Compatible(template requirements, pod requirements) + Add, one class key per lane (eval_wave's merge) ----
    const ReqHdr* Ahdr = d.cls_hdr + (size_t)(d.C + j) * d.K;
    const uint64_t* Aw = d.cls_words + (size_t)(d.C + j) * d.DW;
    const int nck = CC.nck;
    bool fail = false, kill = false, rrow = false;
    uint64_t adm = ~0ull;
    int kmul = -1;
    if (lane == 0) ws.memo_ok = 1;
    auto classify = [&](int k, const ReqHdr& O, const uint64_t* ow, int cnt) {
        const uint32_t kf = CC.kflags[lane];
        if (!(O.flags & RF_DEF)) return;
        if (kf & (KF_CAT_SINGLE | KF_CAT_MULTI | KF_RESV_ROWS)) kill = !op_notin_or_dne(req_op(O.flags, cnt));
        rrow = d.ro && (kf & KF_RESV_ROWS) != 0;
        if (kf & KF_CAT_MULTI) {
            kmul = CC.kmulti[lane];
            const int nv = CC.nval[lane] < 64 ? CC.nval[lane] : 64;
            const uint64_t vm = nv >= 64 ? ~0ull : ((1ull << nv) - 1ull);
            if (!(O.flags & (RF_GT | RF_LT))) {
                adm = ((O.flags & RF_CMP) ? ~ow[0] : ow[0]) & vm;
            } else {
                adm = 0;
                for (int v = 0; v < nv; v++)
                    if (req_has(d, k, v, O, ow)) adm |= 1ull << v;
            }
        }
    };
    const bool topo_cls = TOPO && (CC.flags & CF_TOPO_CONS);
    if (lane < nck) {
        const int k = CC.key[lane], n = CC.nw[lane];
        const ReqHdr A = Ahdr[k];
        const uint64_t* aw = Aw + CC.woff[lane];
        const ReqHdr B = CC.hdr[lane];
        const uint64_t* bw = CC.words + CC.wsoff[lane];
        uint64_t* ow = ws.words + CC.wsoff[lane];
        ReqHdr O;
        int cnt;
        const int nb = CC.nbB[lane];
        if (topo_cls && ((CC.kneutral >> lane) & 1u)) {
            O = A;
            for (int i = 0; i < n; i++) ow[i] = (A.flags & RF_DEF) ? aw[i] : 0ull;
            cnt = 0;
        } else if (!(A.flags & RF_DEF)) {
            if (!op_notin_or_dne(req_op(B.flags, nb)) && !(CC.kflags[lane] & KF_WELL_KNOWN)) fail = true;
            O = B;
            for (int i = 0; i < n; i++) ow[i] = bw[i];
            cnt = nb;
        } else {
            cnt = req_intersect(d, k, A, aw, B, bw, O, ow);
            if (!(O.flags & RF_CMP) && cnt == 0) {
                const int na = popc_words(aw, n);
                if (!(op_notin_or_dne(req_op(B.flags, nb)) && op_notin_or_dne(req_op(A.flags, na)))) fail = true;
            }
        }
        ws.hdr[lane] = O;
        if (!topo_cls) classify(k, O, ow, cnt);
    }
    {
        // the class's hostname requirement is not among its keys; when it cannot meet hostname In [placeholder] of a
        // new NodeClaim (x.hblock), Compatible fails on it whatever the other keys do
        const uint64_t fm = ballot(fail);
        const bool hb = x.hblock[c] != 0;
        if (fm || hb) {
            row.kmask = (uint32_t)fm;  // nck <= KP_MAX_CLASS_KEYS = 32
            row.hostkey = hb ? 1 : 0;
            return finish(KPX_REQUIREMENTS);
        }
    }

    // ---- 5. Topology.AddRequirements at a fresh hostname (the count rows' spare zero column) ----
    if (topo_cls) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        if (!topo_narrow<false>(d, CC, ws, d.E + d.NCcap, true, lane)) return finish(KPX_TOPOLOGY);
        if (lane < nck) {
            const ReqHdr O = ws.hdr[lane];
            const uint64_t* ow = ws.words + CC.wsoff[lane];
            classify(CC.key[lane], O, ow, popc_words(ow, CC.nw[lane]));
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");

    // ---- 6. filterInstanceTypesByRequirements over every option: requirements, fits, offering ----
    EvalEnv E;
    E.alloc = nullptr;
    E.avail = d.avail_zc;
    E.multi16 = nullptr;
    E.astride = 0;
    E.slot_zone = d.slot_zone;
    E.slot_ct = d.slot_ct;
    E.slot_zoneid = d.slot_zoneid;
    E.roles = &roles;
    E.min_tmpl_mask = 0;
    E.ro = d.ro;
    E.type_ro = d.type_ro;
    E.rcap = nullptr;
    E.resv_on = 0;
    E.pt = nullptr;
    E.snap = nullptr;
    // requirements: V ∧ ¬DoesNotExist-types of keys whose merged operator is In / Exists
    uint64_t vreq = lane < TW ? opts & CC.V[lane] : 0ull;
    for (uint64_t km = ballot(kill); km; km &= km - 1) {
        const int i = __ffsll((unsigned long long)km) - 1;
        if (lane < TW)
            vreq &= ~(lane < KP_DNE_TW ? CC.dne[i][lane] : (CC.kcat[i] >= 0 ? d.dne_mask[(size_t)CC.kcat[i] * TW + lane] : 0ull));
    }
    const uint64_t mm = ballot(kmul >= 0);
    const uint64_t mrr = ballot(rrow);
    if (mrr) {  // the reservation-id label beyond 64 values: a type's values are its ResvTab rows' IDs
        const int i = __ffsll((unsigned long long)mrr) - 1;
        const ReqHdr O = ws.hdr[i];
        const uint64_t* ow = ws.words + CC.wsoff[i];
        for (int w = 0; w < TW; w++) {
            const uint64_t cw = rl64(vreq, w);
            if (cw == 0) continue;
            const int t = w * 64 + lane;
            bool ok = true;
            if ((cw >> lane) & 1ull) {
                const uint32_t tr = d.type_ro[t < T ? t : 0];
                const int r0 = (int)(tr >> 16) * 64 + (int)((tr >> 8) & 0xFFu), nr = (int)(tr & 0xFFu);
                ok = nr == 0;
                for (int r = 0; r < nr && !ok; r++) ok = req_has(d, CC.key[i], d.ro->ridv[r0 + r], O, ow);
            }
            const uint64_t m = ballot(ok);
            if (lane == w) vreq &= m;
        }
    }
    // offerings: admissible zone × capacity-type slots, and the compatible available reserved rows
    uint64_t mzc;
    {
        bool ok = false;
        if (lane < d.n_slots) {
            const int zid = E.slot_zoneid[lane];
            ok = role_adm(d, E, CC, ws, Ahdr, Aw, 0, E.slot_zone[lane]) && role_adm(d, E, CC, ws, Ahdr, Aw, 1, E.slot_ct[lane]) &&
                 (zid < 0 || role_adm(d, E, CC, ws, Ahdr, Aw, 2, zid)) && role_dneok(d, E, CC, ws, Ahdr, Aw, 3) &&
                 role_dneok(d, E, CC, ws, Ahdr, Aw, 4);
        }
        mzc = ballot(ok);
    }
    const uint64_t mro = d.ro ? resv_adm(d, E, CC, ws, Ahdr, Aw, lane) : 0ull;
    const bool mro_any = ballot(mro != 0) != 0;

    int n_req = 0, n_fit = 0, n_off = 0;  // wave-uniform (popcounts of ballots)
    uint32_t crit = 0;
    uint64_t anyw = 0, newword = 0;
    for (int w = 0; w < TW; w++) {
        const uint64_t ow = rl64(opts, w);
        if (ow == 0) continue;
        const int t = w * 64 + lane, tt = t < T ? t : 0;
        const bool in = t < T && ((ow >> lane) & 1ull);  // bits past T in the last word never count
        bool rq = (rl64(vreq, w) >> lane) & 1ull;
        for (uint64_t mmm = mm; mmm; mmm &= mmm - 1) {
            const int i = __ffsll((unsigned long long)mmm) - 1;
            const uint64_t tm = d.multi_mask[(size_t)rl32(kmul, i) * T + tt];
            rq &= (tm == 0) | ((tm & rl64(adm, i)) != 0);
        }
        bool ft = true;  // resources.Fits(daemon overhead + pod requests, allocatable)
        for (int ai = 0; ai < d.n_active; ai++) {
            const int r = act_axis(d, ai);
            const int64_t tot = d.daemon[(size_t)j * R + r] + d.pod_req[(size_t)pod * R + r];
            if (tot > 0) ft &= tot <= d.alloc[(size_t)r * T + tt];
        }
        bool of = (d.avail_zc[tt] & mzc) != 0;
        if (mro_any) {
            const uint32_t tr = d.type_ro[tt];
            of |= (shfl64(mro, (int)(tr >> 16)) & ro_span_bits(tr)) != 0;
        }
        rq &= in;
        ft &= in;
        of &= in;
        const uint64_t br = ballot(rq), bf = ballot(ft), bo = ballot(of);
        n_req += __popcll(br);
        n_fit += __popcll(bf);
        n_off += __popcll(bo);
        crit |= (br ? KPX_C_REQ : 0u) | (bf ? KPX_C_FITS : 0u) | (bo ? KPX_C_OFF : 0u) | ((br & bf) ? KPX_C_REQ_FITS : 0u) |
                ((br & bo) ? KPX_C_REQ_OFF : 0u) | ((bf & bo) ? KPX_C_FITS_OFF : 0u);
        const uint64_t nb = br & bf & bo;
        if (lane == w) newword = nb;
        anyw |= nb;
    }
    row.n_requirements = n_req;
    row.n_fits = n_fit;
    row.n_offering = n_off;
    if (anyw == 0) {
        row.criteria = crit;
        return finish(KPX_INSTANCE_TYPES);
    }

    // ---- 7. minValues over what remains (Strict; BestEffort relaxes instead of failing), counted as eval_wave does ----
    if (!d.best_effort && d.min_keys[(size_t)j * KP_MAX_CLASS_KEYS] >= 0) {
        const int* mk = d.min_keys + (size_t)j * KP_MAX_CLASS_KEYS;
        uint32_t unmet = 0;
        for (int q = 0; q < KP_MAX_CLASS_KEYS; q++) {
            const int k = mk[q];
            if (k < 0) break;
            int ci = -1;
            for (int i = 0; i < nck; i++)
                if (CC.key[i] == k) ci = i;
            const ReqHdr h = ci >= 0 ? ws.hdr[ci] : Ahdr[k];
            if (!(h.flags & RF_MIN)) continue;
            int count = 0;
            const int kc = d.kcat[k];
            if (kc >= 0 && (d.kflags[k] & KF_CAT_MULTI)) {
                uint64_t acc = 0;
                for (int w = 0; w < TW; w++) {
                    const uint64_t nwd = rl64(newword, w);
                    if ((nwd >> lane) & 1ull) acc |= d.multi_mask[(size_t)d.kmulti[k] * T + w * 64 + lane];
                }
                count = __popcll(wave_or64(acc));
            } else if (kc >= 0) {
                const int nwk = (d.nval[k] + 63) / 64;
                for (int i = lane; i < KP_MAX_MIN_WORDS; i += 64) ws.minbits[i] = 0;
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                for (int w = 0; w < TW; w++) {
                    const uint64_t nwd = rl64(newword, w);
                    if ((nwd >> lane) & 1ull) {
                        const uint16_t v = d.type_val[(size_t)kc * T + w * 64 + lane];
                        if (v < VAL_ABSENT && v < KP_MAX_MIN_WORDS * 64)
                            atomicOr((unsigned long long*)&ws.minbits[v >> 6], 1ull << (v & 63));  // LDS
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                int cn = 0;
                for (int i = lane; i < nwk && i < KP_MAX_MIN_WORDS; i += 64) cn += __popcll(ws.minbits[i]);
                count = wave_sum_i32(cn);
            }
            if (count < h.minv) unmet |= 1u << q;
        }
        if (unmet) {
            row.kmask = unmet;
            return finish(KPX_MIN_VALUES);
        }
    }

    // ---- 8. the residual.  Every stage that the final state decides passes: when the Add's reservation step is live
    // (a remaining type has a compatible available reserved offering), it is what refused the pod — the reservation
    // capacities themselves live in the FFD kernel's LDS and are not kept.  Otherwise the reason is not known here.
    bool cm = false;
    if (d.ro && d.resv_on) {
        const ResvTab& X = *d.ro;
        for (int q = 0; q < X.w; q++) {
            const int i = q * 64 + lane;
            const int tt = i < X.n ? X.type[i] : -1;
            const uint64_t wd = shfl64(newword, tt >= 0 ? tt >> 6 : 0);
            const bool comp = tt >= 0 && ((rl64(mro, q) >> lane) & 1ull) && ((wd >> (tt & 63)) & 1ull);
            cm |= ballot(comp) != 0;
        }
    }
    finish(cm ? KPX_RESERVED : KPX_UNKNOWN);
}

hipError_t kp_launch_explain(const KpDev& d, const KpExplain& x, hipStream_t s) {
    if (x.n_shapes <= 0 || d.NT <= 0) return hipSuccess;
    const dim3 g(x.n_shapes, d.NT);
    if (d.G > 0) hipLaunchKernelGGL(explain_kernel<true>, g, dim3(64), 0, s, d, x);
    else hipLaunchKernelGGL(explain_kernel<false>, g, dim3(64), 0, s, d, x);
    return hipGetLastError();
}
