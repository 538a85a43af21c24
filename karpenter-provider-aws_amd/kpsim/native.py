"""Loader for libkpsim.so (the gfx950 library).  Fails loudly if it is missing: there is no CPU fallback."""
import ctypes as C
import os

from . import abi

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(PKG_DIR, "..", "lib", "libkpsim.so")

EXPORTS = [
    "kp_ctx_create", "kp_ctx_destroy", "kp_last_error", "kp_version", "kp_catalog_upload", "kp_catalog_patch_avail",
    "kp_catalog_patch_price", "kp_solve", "kp_solve_prepare", "kp_solve_execute", "kp_solve_fetch",
    "kp_result_nodeclaim_requirements", "kp_last_kernel_times", "kp_last_solve_plan", "kp_consolidate_probe_count",
    "kp_consolidate", "kp_consolidate_stats", "kp_consolidate_prepare", "kp_consolidate_execute", "kp_launch_select",
    "kp_launch_stats", "kp_nodeclaim_labels", "kp_catalog_build", "kp_catalog_get_view", "kp_catalog_overhead",
    "kp_catalog_resource_name", "kp_catalog_free", "kp_consolidate_command", "kp_consolidate_replacement",
    "kp_solve_volume_encoding",
    "kp_solve_explain", "kp_solve_explain_key", "kp_solve_explain_stats", "kp_consolidate_explain",
    "kp_consolidate_explain_pods", "kp_consolidate_explain_key", "kp_consolidate_explain_stats",
    "kp_simulate_execute", "kp_simulate_nodeclaims", "kp_simulate_nodeclaim_requirements", "kp_drift_command",
    "kp_consolidate_validate", "kp_simulate_stats",
]

_lib = None


class KpError(RuntimeError):
    def __init__(self, status, msg=""):
        super().__init__("%s: %s" % (abi.STATUS_NAMES.get(status, status), msg))
        self.status = status


def load():
    global _lib
    if _lib is not None:
        return _lib
    path = os.path.normpath(os.environ.get("KPSIM_LIB", LIB_PATH))  # A/B diagnostics override
    if not os.path.exists(path):
        raise ImportError("libkpsim.so not built at %s (run __graft_entry__.build() or make -C karpenter-provider-aws_amd)"
                          % path)
    L = C.CDLL(path)
    L.kp_ctx_create.argtypes = [C.POINTER(abi.kp_device_opts), C.POINTER(C.c_void_p)]
    L.kp_ctx_destroy.argtypes = [C.c_void_p]
    L.kp_last_error.argtypes = [C.c_void_p]
    L.kp_last_error.restype = C.c_char_p
    L.kp_version.restype = C.c_char_p
    L.kp_catalog_upload.argtypes = [C.c_void_p, C.POINTER(abi.kp_catalog_view), C.c_uint64]
    L.kp_catalog_patch_avail.argtypes = [C.c_void_p, C.POINTER(C.c_uint8), C.c_int32, C.c_uint64]
    L.kp_catalog_patch_price.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_double), C.c_int32, C.c_uint64]
    # the whole C struct: ctypes then refuses the shorter mirror abi.kp_solve_input, which ends before the volume tables
    L.kp_solve.argtypes = [C.c_void_p, C.POINTER(abi.kp_solve_input_full), C.POINTER(abi.kp_solve_output)]
    L.kp_solve_prepare.argtypes = [C.c_void_p, C.POINTER(abi.kp_solve_input_full)]
    if hasattr(L, "kp_solve_volume_encoding"):  # (absent from older libraries, A/B only)
        L.kp_solve_volume_encoding.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.c_int64, C.POINTER(C.c_int64)]
    L.kp_solve_execute.argtypes = [C.c_void_p]
    if hasattr(L, "kp_solve_explain"):  # (absent from older libraries, A/B only)
        L.kp_solve_explain.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(abi.kp_pod_explanation),
                                       C.c_int64, C.POINTER(C.c_int64)]
        L.kp_solve_explain_key.argtypes = [C.c_void_p, C.c_int32, C.c_char_p, C.c_int64, C.POINTER(C.c_int64)]
        L.kp_solve_explain_stats.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.c_int32]
    L.kp_solve_fetch.argtypes = [C.c_void_p, C.POINTER(abi.kp_solve_output)]
    L.kp_result_nodeclaim_requirements.argtypes = [C.c_void_p, C.c_int32, C.c_char_p, C.c_int64, C.POINTER(C.c_int64)]
    L.kp_last_kernel_times.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_int32]
    if hasattr(L, "kp_last_solve_plan"):  # (absent from older libraries, A/B only)
        L.kp_last_solve_plan.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.c_int32]
    L.kp_consolidate_probe_count.argtypes = [C.POINTER(abi.kp_consolidate_input)]
    L.kp_consolidate.argtypes = [C.c_void_p, C.POINTER(abi.kp_consolidate_input), C.POINTER(abi.kp_probe_result),
                                 C.c_int32]
    L.kp_consolidate_prepare.argtypes = [C.c_void_p, C.POINTER(abi.kp_consolidate_input)]
    L.kp_consolidate_execute.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(abi.kp_probe_result),
                                         C.c_int32]
    L.kp_consolidate_stats.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.c_int32]
    L.kp_consolidate_command.argtypes = [C.c_void_p, C.c_int32, C.POINTER(abi.kp_consolidation_command)]
    if hasattr(L, "kp_consolidate_replacement"):  # (absent from pre-round-5 libraries, A/B only)
        L.kp_consolidate_replacement.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(abi.kp_consolidation_command)]
    if hasattr(L, "kp_consolidate_explain"):  # (absent from older libraries, A/B only)
        L.kp_consolidate_explain.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                             C.POINTER(abi.kp_probe_explanation), C.c_int32]
        L.kp_consolidate_explain_pods.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                                  C.POINTER(abi.kp_pod_explanation), C.c_int64, C.POINTER(C.c_int64)]
        L.kp_consolidate_explain_key.argtypes = [C.c_void_p, C.c_int32, C.c_char_p, C.c_int64, C.POINTER(C.c_int64)]
        L.kp_consolidate_explain_stats.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.c_int32]
    if hasattr(L, "kp_simulate_execute"):  # (absent from older libraries, A/B only)
        L.kp_simulate_execute.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(abi.kp_sim_result),
                                          C.c_int32]
        L.kp_simulate_nodeclaims.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(abi.kp_sim_nodeclaims)]
        L.kp_simulate_nodeclaim_requirements.argtypes = [C.c_void_p, C.c_int32, C.c_char_p, C.c_int64,
                                                         C.POINTER(C.c_int64)]
        L.kp_drift_command.argtypes = [C.c_void_p, C.POINTER(abi.kp_drift_command_out)]
        L.kp_consolidate_validate.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                              C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.kp_simulate_stats.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.c_int32]
    L.kp_launch_select.argtypes = [C.c_void_p, C.c_int32, C.POINTER(abi.kp_launch_request), C.c_int32,
                                   C.POINTER(abi.kp_launch_result), C.POINTER(C.c_int32), C.c_int32,
                                   C.POINTER(C.c_int32), C.c_int32]
    L.kp_launch_stats.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_int32]
    L.kp_nodeclaim_labels.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_char_p, C.c_char_p, C.c_int32, C.c_char_p,
                                      C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    for f in EXPORTS:
        if os.environ.get("KPSIM_LIB") and not hasattr(L, f):
            continue  # A/B diagnostics: an older library without a later entry point (its callers are not used)
        if f not in ("kp_last_error", "kp_version", "kp_catalog_resource_name"):
            getattr(L, f).restype = C.c_int32
    _lib = L
    return L


class Context:
    """One kp_ctx (device stream + buffers).  Not thread-safe; use one per thread."""

    def __init__(self, device=0, preference_policy=abi.KP_PREFERENCE_RESPECT, devices=None, reserved_capacity=1,
                 simulate_topology=0):
        L = load()
        self.L = L
        h = C.c_void_p()
        opts = abi.kp_device_opts(device=device, preference_policy=preference_policy, reserved_capacity=reserved_capacity,
                                   simulate_topology=simulate_topology)
        if devices:
            import numpy as np
            self._devs = np.ascontiguousarray(devices, np.int32)
            opts.n_devices = len(self._devs)
            opts.devices = self._devs.ctypes.data_as(C.POINTER(C.c_int32))
        st = L.kp_ctx_create(C.byref(opts), C.byref(h))
        if st != 0:
            raise KpError(st, "kp_ctx_create(device=%d) — a gfx950 device is required" % device)
        self.h = h
        self._catalog = None
        # bumped by every call that replaces the ctx's catalog or prepared pass (kp_catalog_*, kp_solve*,
        # kp_consolidate[_prepare]): lets a caller tell whether the pass it prepared is still the ctx's
        self.pass_gen = 0

    def check(self, st, what):
        if st != 0:
            raise KpError(st, "%s: %s" % (what, self.L.kp_last_error(self.h).decode()))

    def upload_catalog(self, catalog_view, epoch=1):
        self.pass_gen += 1
        self.check(self.L.kp_catalog_upload(self.h, C.byref(catalog_view.view), epoch), "kp_catalog_upload")
        self._catalog = catalog_view

    def patch_avail(self, available, epoch):
        self.pass_gen += 1
        import numpy as np
        a = np.ascontiguousarray(available, np.uint8)
        self.check(self.L.kp_catalog_patch_avail(self.h, a.ctypes.data_as(C.POINTER(C.c_uint8)), len(a), epoch),
                   "kp_catalog_patch_avail")

    def patch_price(self, idx, price, epoch):
        self.pass_gen += 1
        import numpy as np
        i = np.ascontiguousarray(idx, np.int32)
        p = np.ascontiguousarray(price, np.float64)
        self.check(self.L.kp_catalog_patch_price(self.h, i.ctypes.data_as(C.POINTER(C.c_int32)),
                                                 p.ctypes.data_as(C.POINTER(C.c_double)), len(i), epoch),
                   "kp_catalog_patch_price")

    def launch_select(self, batch, M=60):
        """kp_launch_select over a model.LaunchBatchView → model.LaunchResults (instance.go:132-137 per request)."""
        from kpsim import model
        st, res = model.launch_call(lambda *a: self.L.kp_launch_select(self.h, *a), self._catalog, batch, M)
        self.check(st, "kp_launch_select")
        return res

    def nodeclaim_labels(self, type_index, offering, zone_id=None, nodepool=None, efa_enabled=False):
        """kp_nodeclaim_labels (instanceToNodeClaim, cloudprovider.go:381-444) → (labels dict, capacity[R],
        allocatable[R]) for an instance of catalog row type_index launched through offering row `offering`."""
        import numpy as np
        from kpsim import model
        need = C.c_int64(0)
        buf = C.create_string_buffer(1 << 14)
        cap = np.zeros(model.R, np.int64)
        alloc = np.zeros(model.R, np.int64)
        self.check(self.L.kp_nodeclaim_labels(self.h, type_index, offering, zone_id.encode() if zone_id else None,
                                              nodepool.encode() if nodepool else None, 1 if efa_enabled else 0, buf,
                                              len(buf), C.byref(need), cap.ctypes.data_as(C.POINTER(C.c_int64)),
                                              alloc.ctypes.data_as(C.POINTER(C.c_int64))), "kp_nodeclaim_labels")
        labels = dict(line.split("\t", 1) for line in buf.value.decode().splitlines() if line)
        return labels, cap, alloc

    def launch_stats(self, n=2):
        """[kernel ms, whole call ms] (n=6 adds the host phases: encode, merge + upload, download waits, expand;
        n=7 the number of sub-batches the call was pipelined over)."""
        ms = (C.c_double * n)()
        self.check(self.L.kp_launch_stats(self.h, ms, n), "kp_launch_stats")
        return list(ms)

    def prepare(self, input_view):
        self.pass_gen += 1
        self.check(self.L.kp_solve_prepare(self.h, C.byref(input_view.view)), "kp_solve_prepare")

    def execute(self):
        self.check(self.L.kp_solve_execute(self.h), "kp_solve_execute")

    def volume_encoding(self):
        """kp_solve_volume_encoding of the prepared Solve or consolidation pass, as a dict of numpy arrays."""
        import numpy as np
        need = C.c_int64(0)
        st = self.L.kp_solve_volume_encoding(self.h, None, 0, C.byref(need))
        if st not in (abi.KP_OK, abi.KP_E_BUFFER):
            self.check(st, "kp_solve_volume_encoding")
        buf = np.zeros(max(1, need.value), np.int64)
        self.check(self.L.kp_solve_volume_encoding(self.h, buf.ctypes.data_as(C.POINTER(C.c_int64)), buf.size,
                                                   C.byref(need)), "kp_solve_volume_encoding")
        VD, VW, bits, NS, P, E = (int(x) for x in buf[:6])
        out, pos = {"VD": VD, "VW": VW, "bits": bits, "NS": NS}, 6
        for name, shape in (("limited_driver", (VD,)), ("pod_signature", (P,)), ("signature_count", (NS, VD)),
                            ("signature_mask", (NS, VW)), ("driver_mask", (VD, VW)), ("node_count", (VD, E)),
                            ("node_limit", (VD, E)), ("node_mask", (E, VW)), ("node_over_limit", (E,))):
            n = int(np.prod(shape))
            a = buf[pos:pos + n].reshape(shape) if VD > 0 else np.zeros((0,) * len(shape), np.int64)
            out[name] = a.view(np.uint64) if name.endswith("mask") else a
            pos += n if VD > 0 else 0
        return out

    def explain(self, pods=None):
        """kp_solve_explain of the executed Solve: one row per (unschedulable pod, NodePool) as a numpy array of
        abi.EXPLANATION_DTYPE, grouped by pod in ascending pod index, a pod's rows in template order.  pods=None: every
        unschedulable pod; else the listed ones (KP_E_INVALID for a scheduled pod or an index out of range)."""
        import numpy as np
        need = C.c_int64(0)
        n, lst = 0, None
        if pods is not None:
            self._x_pods = np.ascontiguousarray(pods, np.int32)
            n, lst = len(self._x_pods), self._x_pods.ctypes.data_as(C.POINTER(C.c_int32))
        st = self.L.kp_solve_explain(self.h, n, lst, None, 0, C.byref(need))
        if st not in (abi.KP_OK, abi.KP_E_BUFFER):
            self.check(st, "kp_solve_explain")
        out = np.zeros(max(1, need.value), abi.EXPLANATION_DTYPE)
        if need.value:
            self.check(self.L.kp_solve_explain(self.h, n, lst, out.ctypes.data_as(C.POINTER(abi.kp_pod_explanation)),
                                               len(out), C.byref(need)), "kp_solve_explain")
        return out[:need.value]

    def explain_key(self, key):
        """Name of key `key` of kp_pod_explanation.key (kp_solve_explain_key)."""
        need = C.c_int64(0)
        buf = C.create_string_buffer(256)
        st = self.L.kp_solve_explain_key(self.h, key, buf, len(buf), C.byref(need))
        if st == abi.KP_E_BUFFER:
            buf = C.create_string_buffer(need.value)
            st = self.L.kp_solve_explain_key(self.h, key, buf, len(buf), C.byref(need))
        self.check(st, "kp_solve_explain_key")
        return buf.value.decode()

    def explain_stats(self):
        """(ms[kernel, whole call], counters[(shape, NodePool) pairs evaluated, distinct shapes, pods reported]) of the
        last explain()."""
        ms = (C.c_double * 2)()
        ct = (C.c_int64 * 3)()
        self.check(self.L.kp_solve_explain_stats(self.h, ms, ct, 3), "kp_solve_explain_stats")
        return list(ms), list(ct)

    def fetch(self, out_buffers):
        self.check(self.L.kp_solve_fetch(self.h, C.byref(out_buffers.view)), "kp_solve_fetch")

    def solve(self, input_view, out_buffers):
        self.pass_gen += 1
        self.check(self.L.kp_solve(self.h, C.byref(input_view.view), C.byref(out_buffers.view)), "kp_solve")

    def nodeclaim_requirements(self, nc):
        need = C.c_int64(0)
        buf = C.create_string_buffer(1 << 16)
        st = self.L.kp_result_nodeclaim_requirements(self.h, nc, buf, len(buf), C.byref(need))
        if st == abi.KP_E_BUFFER:
            buf = C.create_string_buffer(need.value)
            st = self.L.kp_result_nodeclaim_requirements(self.h, nc, buf, len(buf), C.byref(need))
        self.check(st, "kp_result_nodeclaim_requirements")
        return buf.value.decode()

    def kernel_times_ms(self):
        """[queue sort, class masks, template filter, FFD, finalize] of the last execute (HIP events)."""
        a = (C.c_double * 5)()
        self.check(self.L.kp_last_kernel_times(self.h, a, 5), "kp_last_kernel_times")
        return list(a)

    def ffd_cycles(self):
        """FFD-kernel counters of the last fetched solve (kpsim.h kp_last_kernel_times [5..19]): s_memtime cycles
        (with KPSIM_PROFILE=1) of the fast loop, sort, slow-path rounds, templates, -, full sort, six evaluation
        stages; then quick accepts, slow-path pods, witness misses, quick-path cycles (pop, scan, check, commit)."""
        a = (C.c_double * 42)()
        self.check(self.L.kp_last_kernel_times(self.h, a, 42), "kp_last_kernel_times")
        return list(a)[5:]

    def solve_plan(self):
        """kp_last_solve_plan of the last execute as a dict (abi.SOLVE_PLAN_FIELDS): the planned NodeClaim capacity and
        LDS layout, and the feature bits that selected the Solve entry point.  Diagnostics."""
        a = (C.c_int32 * len(abi.SOLVE_PLAN_FIELDS))()
        self.check(self.L.kp_last_solve_plan(self.h, a, len(a)), "kp_last_solve_plan")
        return dict(zip(abi.SOLVE_PLAN_FIELDS, (int(x) for x in a)))

    def consolidate(self, cons_view):
        """kp_consolidate over the view's probe range -> numpy array of abi.PROBE_DTYPE (one row per probe)."""
        self.pass_gen += 1
        import numpy as np
        v = cons_view.view
        n = self.L.kp_consolidate_probe_count(C.byref(v))
        b0 = max(0, v.probe_begin)
        b1 = v.probe_end if 0 < v.probe_end < n else n
        out = np.zeros(max(1, b1 - b0), abi.PROBE_DTYPE)
        self.check(self.L.kp_consolidate(self.h, C.byref(v), out.ctypes.data_as(C.POINTER(abi.kp_probe_result)),
                                         len(out)), "kp_consolidate")
        return out[:max(0, b1 - b0)]

    def consolidate_prepare(self, cons_view):
        self.pass_gen += 1
        self.check(self.L.kp_consolidate_prepare(self.h, C.byref(cons_view.view)), "kp_consolidate_prepare")

    def consolidate_execute(self, mode, n_probes, begin=0, end=0):
        """Probes [begin, end) of `mode` over the prepared pass; n_probes = the mode's probe count."""
        import numpy as np
        b1 = end if 0 < end < n_probes else n_probes
        out = np.zeros(max(1, b1 - begin), abi.PROBE_DTYPE)
        self.check(self.L.kp_consolidate_execute(self.h, mode, begin, end,
                                                 out.ctypes.data_as(C.POINTER(abi.kp_probe_result)), len(out)),
                   "kp_consolidate_execute")
        return out[:max(0, b1 - begin)]

    def consolidate_command(self, mode):
        """kp_consolidate_command over the prepared pass -> kpsim.consolidation.Command (with the replacement)."""
        from kpsim import consolidation
        st, cmd = consolidation.command_call(lambda cc: self.L.kp_consolidate_command(self.h, mode, C.byref(cc)))
        self.check(st, "kp_consolidate_command")
        return cmd

    def consolidate_replacement(self, mode, probe):
        """kp_consolidate_replacement: the command of one probe of the prepared pass (its row and, for a REPLACE, the
        replacement NodeClaim) -> kpsim.consolidation.Command."""
        from kpsim import consolidation
        st, cmd = consolidation.command_call(
            lambda cc: self.L.kp_consolidate_replacement(self.h, mode, probe, C.byref(cc)))
        self.check(st, "kp_consolidate_replacement")
        return cmd

    def consolidate_stats(self):
        """(ms[prep, probe kernel, call], counters[20]) of the last kp_consolidate (kpsim.h kp_consolidate_stats)."""
        ms = (C.c_double * 3)()
        ct = (C.c_int64 * 20)()
        self.check(self.L.kp_consolidate_stats(self.h, ms, ct, 20), "kp_consolidate_stats")
        return list(ms), list(ct)

    def consolidate_explain(self, mode, n_probes, begin=0, end=0):
        """kp_consolidate_explain: why each probe [begin, end) of `mode` (SINGLE or MULTI) of the prepared pass found no
        command -> numpy array of abi.PROBE_EXPLANATION_DTYPE; n_probes = the mode's probe count."""
        import numpy as np
        b1 = end if 0 < end < n_probes else n_probes
        out = np.zeros(max(1, b1 - begin), abi.PROBE_EXPLANATION_DTYPE)
        self.check(self.L.kp_consolidate_explain(self.h, mode, begin, end,
                                                 out.ctypes.data_as(C.POINTER(abi.kp_probe_explanation)), len(out)),
                   "kp_consolidate_explain")
        return out[:max(0, b1 - begin)]

    def consolidate_explain_pods(self, mode, probe, max_pods=0):
        """kp_consolidate_explain_pods: the first max_pods (<= 0: all) non-pending pods a PODS_UNSCHEDULABLE probe left
        without a place, one row per (pod, NodePool) as abi.EXPLANATION_DTYPE; empty for any other probe."""
        import numpy as np
        need = C.c_int64(0)
        st = self.L.kp_consolidate_explain_pods(self.h, mode, probe, max_pods, None, 0, C.byref(need))
        if st not in (abi.KP_OK, abi.KP_E_BUFFER):
            self.check(st, "kp_consolidate_explain_pods")
        out = np.zeros(max(1, need.value), abi.EXPLANATION_DTYPE)
        if need.value:
            self.check(self.L.kp_consolidate_explain_pods(self.h, mode, probe, max_pods,
                                                          out.ctypes.data_as(C.POINTER(abi.kp_pod_explanation)), len(out),
                                                          C.byref(need)), "kp_consolidate_explain_pods")
        return out[:need.value]

    def consolidate_explain_key(self, key):
        """Name of key `key` of a kp_consolidate_explain_pods row (kp_consolidate_explain_key)."""
        need = C.c_int64(0)
        buf = C.create_string_buffer(256)
        st = self.L.kp_consolidate_explain_key(self.h, key, buf, len(buf), C.byref(need))
        if st == abi.KP_E_BUFFER:
            buf = C.create_string_buffer(need.value)
            st = self.L.kp_consolidate_explain_key(self.h, key, buf, len(buf), C.byref(need))
        self.check(st, "kp_consolidate_explain_key")
        return buf.value.decode()

    def consolidate_explain_stats(self):
        """(ms[kernels, whole call], counters[probes explained, (shape, NodePool) pairs diagnosed]) of the last
        consolidate_explain() / consolidate_explain_pods()."""
        ms = (C.c_double * 2)()
        ct = (C.c_int64 * 2)()
        self.check(self.L.kp_consolidate_explain_stats(self.h, ms, ct, 2), "kp_consolidate_explain_stats")
        return list(ms), list(ct)

    def simulate_execute(self, mode, n_probes, begin=0, end=0):
        """kp_simulate_execute: SimulateScheduling's Results of probes [begin, end) of `mode` (SINGLE or MULTI) of the
        prepared pass, with up to 12 new NodeClaims -> numpy array of abi.SIM_DTYPE; n_probes = the mode's probe count."""
        import numpy as np
        b1 = end if 0 < end < n_probes else n_probes
        out = np.zeros(max(1, b1 - begin), abi.SIM_DTYPE)
        self.check(self.L.kp_simulate_execute(self.h, mode, begin, end, out.ctypes.data_as(C.POINTER(abi.kp_sim_result)),
                                              len(out)), "kp_simulate_execute")
        return out[:max(0, b1 - begin)]

    def simulate_nodeclaims(self, mode, probe):
        """kp_simulate_nodeclaims of one probe -> (row dict, pods, model.Results, requirements): pods lists the probe's
        pods (pending first, then its candidates' pods) as indices into cluster.pods, the Results' pod arrays follow that
        list (an existing node is -2 - j, j into cluster.existing), requirements[i] is NodeClaim i's parsed
        requirements.  A row that is not KP_SIM_OK comes with no pods and no NodeClaims."""
        import numpy as np
        from kpsim import model
        cap_t, cap_p = 1024, 1024
        for _ in range(2):
            arr = {k: np.full(max(1, n), -7, np.int32) for k, n in
                   (("type_ids", cap_t), ("pods", cap_p), ("pod_result", cap_p), ("pod_order", cap_p))}
            o = abi.kp_sim_nodeclaims()
            o.cap_type_ids, o.cap_pods = cap_t, cap_p
            for k, a in arr.items():
                setattr(o, k, a.ctypes.data_as(abi.c_int32_p))
            st = self.L.kp_simulate_nodeclaims(self.h, mode, probe, C.byref(o))
            if st != abi.KP_E_BUFFER:
                break
            cap_t, cap_p = max(cap_t, o.n_type_ids), max(cap_p, o.n_pods)
        self.check(st, "kp_simulate_nodeclaims")
        n, m = o.n_nodeclaims, o.n_pods
        off = list(o.nodeclaim_type_offset)
        res = model.Results(np.array(o.nodeclaim_nodepool[:n], np.int32), np.array(o.nodeclaim_n_pods[:n], np.int32),
                            np.array(o.nodeclaim_slice_pos[:n], np.int32), np.array(o.nodeclaim_n_options[:n], np.int32),
                            [arr["type_ids"][off[i]:off[i + 1]].tolist() for i in range(n)],
                            arr["pod_result"][:m].copy(), arr["pod_order"][:m].copy(), {})
        reqs = [model.parse_requirements_blob(self.simulate_nodeclaim_requirements(i)) for i in range(n)]
        row = {f: int(getattr(o.row, f)) for f, _ in abi.kp_sim_result._fields_}
        return row, arr["pods"][:m].copy(), res, reqs

    def simulate_nodeclaim_requirements(self, nc):
        need = C.c_int64(0)
        buf = C.create_string_buffer(1 << 16)
        st = self.L.kp_simulate_nodeclaim_requirements(self.h, nc, buf, len(buf), C.byref(need))
        if st == abi.KP_E_BUFFER:
            buf = C.create_string_buffer(need.value)
            st = self.L.kp_simulate_nodeclaim_requirements(self.h, nc, buf, len(buf), C.byref(need))
        self.check(st, "kp_simulate_nodeclaim_requirements")
        return buf.value.decode()

    def drift_command(self, cap_candidates=4096):
        """kp_drift_command over the prepared candidates -> dict(decision, candidates, n_nodeclaims, row); a REPLACE's
        NodeClaims are read with simulate_nodeclaims(KP_CONSOLIDATE_SINGLE, candidates[0])."""
        import numpy as np
        for _ in range(2):
            cands = np.zeros(max(1, cap_candidates), np.int32)
            o = abi.kp_drift_command_out()
            o.cap_candidates = len(cands)
            o.candidates = cands.ctypes.data_as(abi.c_int32_p)
            st = self.L.kp_drift_command(self.h, C.byref(o))
            if st != abi.KP_E_BUFFER:
                break
            cap_candidates = max(cap_candidates, o.n_candidates)
        self.check(st, "kp_drift_command")
        return dict(decision=int(o.decision), candidates=[int(x) for x in cands[:o.n_candidates]],
                    n_nodeclaims=int(o.n_nodeclaims),
                    row={f: int(getattr(o.row, f)) for f, _ in abi.kp_sim_result._fields_})

    def consolidate_validate(self, mode, probe, had_replacement, type_ids=()):
        """kp_consolidate_validate: ValidateCommand's verdict (abi.KP_VALIDATE_*) for the command of one probe."""
        import numpy as np
        t = np.ascontiguousarray(type_ids, np.int32)
        v = C.c_int32(-1)
        self.check(self.L.kp_consolidate_validate(self.h, mode, probe, 1 if had_replacement else 0, len(t),
                                                  t.ctypes.data_as(abi.c_int32_p) if len(t) else None, C.byref(v)),
                   "kp_consolidate_validate")
        return int(v.value)

    def simulate_stats(self):
        """(ms[simulate kernel, finalize kernel, whole call], counters[pods popped, NodeClaim evaluations, template
        evaluations, probes run, overflow rows, unsupported rows, batches]) of the last simulate / drift / validate call."""
        ms = (C.c_double * 3)()
        ct = (C.c_int64 * 7)()
        self.check(self.L.kp_simulate_stats(self.h, ms, ct, 7), "kp_simulate_stats")
        return list(ms), list(ct)

    def close(self):
        if getattr(self, "h", None):
            self.L.kp_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
