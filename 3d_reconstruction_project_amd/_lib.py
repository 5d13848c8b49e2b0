"""ctypes binding of libr3d_hip.so (C ABI: include/r3d.h).  There is NO CPU fallback: if the HIP library is missing
or no gfx950 device is visible, every entry point raises."""
import ctypes
import os

import numpy as np

# HIP maps streams onto at most GPU_MAX_HW_QUEUES hardware queues (default 4), in order per queue.  The library pipelines maps over
# three lanes (own stream each) next to the context stream(s) and the caller's streams: with four queues two of them share one and
# their kernels serialise -- measured at C2 with three maps in flight: 338-340 maps/s with 4 queues, 365-370 with 8 (16: the same);
# the 8-view batch on one GPU 31.2-31.6 -> 29.4-29.9 ms.  The HIP runtime reads the variable when it initialises, i.e. at the first
# GPU call of the PROCESS, so it is the application's to set (bench.py and its rank launcher do; INTEGRATION.md recommends it):
# importing this package does not touch the environment.  The batch entry points warn once when the setting is below what they use.
RECOMMENDED_ENV = {"GPU_MAX_HW_QUEUES": "8"}
_warned_queues = False


def warn_if_few_hw_queues(streams_in_use):
    """One warning per process when the batch paths would like more hardware queues than the runtime was started with."""
    global _warned_queues
    if _warned_queues:
        return
    try:
        have = int(os.environ.get("GPU_MAX_HW_QUEUES", "4"))
    except ValueError:
        return
    if have < streams_in_use:
        _warned_queues = True
        import warnings
        warnings.warn(f"3d_reconstruction_project_amd: {streams_in_use} streams are in use but the HIP runtime maps them onto "
                      f"GPU_MAX_HW_QUEUES={have} hardware queues (streams that share a queue serialise; measured -8 % on the pipelined "
                      "batch paths).  Export GPU_MAX_HW_QUEUES=8 before the process makes its first GPU call.", RuntimeWarning, stacklevel=3)


_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libr3d_hip.so")

R3D_OK = 0
HIP_STREAM_LEGACY = 1       # hipStreamLegacy ((hipStream_t)1, hip_runtime_api.h): the null stream with legacy synchronisation
ERR_NAMES = {-1: "R3D_E_BADARG", -2: "R3D_E_HIP", -3: "R3D_E_OOM", -4: "R3D_E_UNSUPPORTED", -5: "R3D_E_NODEVICE", -6: "R3D_E_INTERNAL"}


class SgbmParams(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in (
        "minDisparity", "numDisparities", "blockSize", "P1", "P2", "disp12MaxDiff", "preFilterCap",
        "uniquenessRatio", "speckleWindowSize", "speckleRange", "mode")]


class IcpParams(ctypes.Structure):
    _fields_ = [("mode", ctypes.c_int32), ("max_iteration", ctypes.c_int32),
                ("max_correspondence_distance", ctypes.c_double), ("relative_fitness", ctypes.c_double),
                ("relative_rmse", ctypes.c_double), ("gicp_epsilon", ctypes.c_double)]


class ColoredIcpParams(ctypes.Structure):
    """r3d_colored_icp_params: the registration parameters (icp.mode = 3) + the coloured mode's own."""
    _fields_ = [("icp", IcpParams), ("lambda_geometric", ctypes.c_double), ("gradient_radius", ctypes.c_double),
                ("gradient_max_nn", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class IcpStats(ctypes.Structure):
    _fields_ = [("iterations", ctypes.c_int32), ("converged", ctypes.c_int32), ("correspondences", ctypes.c_int64),
                ("fitness", ctypes.c_double), ("inlier_rmse", ctypes.c_double), ("setup_ms", ctypes.c_double),
                ("loop_ms", ctypes.c_double)]


class ResourceCounts(ctypes.Structure):
    """r3d_resource_counts: what the library holds on the GPU right now, over the whole process."""
    _fields_ = [(n, ctypes.c_int64) for n in ("device_allocs", "device_bytes", "pinned_allocs", "events", "streams")]


class PoseGraphParams(ctypes.Structure):
    """r3d_posegraph_params: GlobalOptimizationOption and GlobalOptimizationConvergenceCriteria in one block"""
    _fields_ = [(n, ctypes.c_double) for n in (
        "max_correspondence_distance", "edge_prune_threshold", "preference_loop_closure", "min_relative_increment",
        "min_relative_residual_increment", "min_right_term", "min_residual")] + [(n, ctypes.c_int32) for n in (
            "reference_node", "max_iteration", "max_iteration_lm", "trace_capacity")]


class PoseGraphStats(ctypes.Structure):
    """r3d_posegraph_stats"""
    _fields_ = [(n, ctypes.c_int32) for n in (
        "outer_iterations", "trials", "rejected_trials", "failed_factorizations", "edges_pruned", "stop_first", "stop_second",
        "reserved")] + [(n, ctypes.c_double) for n in (
            "first_objective", "final_objective", "linearize_ms", "factor_ms", "substitute_ms", "rest_ms")]


_lib = None

_vp = ctypes.c_void_p
_posegraph_optimize_sig = ([_vp, ctypes.POINTER(PoseGraphParams), ctypes.c_int64, _vp, ctypes.c_int64, _vp, _vp, _vp, _vp, _vp, _vp,
                            ctypes.POINTER(PoseGraphStats), _vp], ctypes.c_int)
_i32, _i64 = ctypes.c_int32, ctypes.c_int64
_i64p = ctypes.POINTER(ctypes.c_int64)
# ctx, nv, nt, vertices, triangles, cap_clusters, triangle_clusters, cluster_n_triangles, cluster_area, out_n_clusters
_meshtopo_components_sig = ([_vp, _i64, _i64, _vp, _vp, _i64, _vp, _vp, _vp, _i64p], ctypes.c_int)
# ctx, nv, nt, vertices, normals, colors, triangles, flags, cap_vertices, cap_triangles, out_vertices, out_normals, out_colors, out_triangles,
# vertex_map, triangle_origin, out_nv, out_nt
_meshtopo_dedup_sig = ([_vp, _i64, _i64, _vp, _vp, _vp, _vp, _i32, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i64p, _i64p], ctypes.c_int)
_SIGS = {
    "r3d_init": ([ctypes.c_int, ctypes.POINTER(_vp)], ctypes.c_int),
    "r3d_destroy": ([_vp], None),
    "r3d_last_error": ([_vp], ctypes.c_char_p),
    "r3d_sync": ([_vp], ctypes.c_int),
    "r3d_set_stream": ([_vp, _vp], ctypes.c_int),
    "r3d_get_stream": ([_vp], _vp),
    "r3d_selftest": ([_vp], ctypes.c_int),
    "r3d_debug_streambench": ([_vp, ctypes.c_int32, ctypes.c_int32, ctypes.c_uint64, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_float)], ctypes.c_int),
    "r3d_dev_alloc": ([_vp, ctypes.c_uint64, ctypes.POINTER(_vp)], ctypes.c_int),
    "r3d_dev_free": ([_vp, _vp], ctypes.c_int),
    "r3d_copy_h2d": ([_vp, _vp, _vp, ctypes.c_uint64], ctypes.c_int),
    "r3d_copy_d2h": ([_vp, _vp, _vp, ctypes.c_uint64], ctypes.c_int),
    "r3d_event_create": ([_vp, ctypes.POINTER(_vp)], ctypes.c_int),
    "r3d_event_destroy": ([_vp, _vp], ctypes.c_int),
    "r3d_event_record": ([_vp, _vp], ctypes.c_int),
    "r3d_event_elapsed_ms": ([_vp, _vp, _vp, ctypes.POINTER(ctypes.c_float)], ctypes.c_int),
    "r3d_sgbm_compute": ([_vp, ctypes.POINTER(SgbmParams), _vp, _vp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _vp], ctypes.c_int),
    "r3d_sgbm_compute_dev": ([_vp, ctypes.POINTER(SgbmParams), _vp, _vp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _vp], ctypes.c_int),
    "r3d_sgbm_compute_batch_dev": ([_vp, ctypes.POINTER(SgbmParams), ctypes.c_int32, _vp, _vp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _vp], ctypes.c_int),
    "r3d_sgbm_compute_batch_events_dev": ([_vp, ctypes.POINTER(SgbmParams), ctypes.c_int32, _vp, _vp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _vp, _vp], ctypes.c_int),
    "r3d_sgbm_compute_cn": ([_vp, ctypes.POINTER(SgbmParams), _vp, _vp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _vp], ctypes.c_int),
    "r3d_sgbm_compute_cn_dev": ([_vp, ctypes.POINTER(SgbmParams), _vp, _vp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _vp], ctypes.c_int),
    "r3d_sgbm_compute_batch_cn_dev": ([_vp, ctypes.POINTER(SgbmParams), ctypes.c_int32, _vp, _vp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _vp, _vp], ctypes.c_int),
    "r3d_stream_wait_event": ([_vp, _vp], ctypes.c_int),
    "r3d_filter_speckles": ([_vp, _vp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32], ctypes.c_int),
    "r3d_set_profiling": ([_vp, ctypes.c_int], ctypes.c_int),
    "r3d_sgbm_profile": ([_vp, ctypes.POINTER(ctypes.c_float), ctypes.c_int32, ctypes.c_char_p, ctypes.c_int32], ctypes.c_int),
    "r3d_sgbm_debug_fetch": ([_vp, _vp, _vp, _vp], ctypes.c_int),
    "r3d_sgbm_debug_hh_partial": ([_vp, ctypes.c_int32, _vp], ctypes.c_int),
    # the selection stage on caller-supplied volumes: ctx, params, w, h, cost, cspec, hsum, cost_pad, hsum_pad, raw_out, mins_out, lrd_out
    "r3d_sgbm_debug_select": ([_vp, ctypes.POINTER(SgbmParams), ctypes.c_int32, ctypes.c_int32, _vp, _vp, _vp, ctypes.c_int32, ctypes.c_int32, _vp, _vp, _vp], ctypes.c_int),
    # raw_wta, mins, lrd of the last compute or debug_select call
    "r3d_sgbm_debug_fetch_select": ([_vp, _vp, _vp, _vp], ctypes.c_int),
    "r3d_debug_resources": ([ctypes.POINTER(ResourceCounts)], ctypes.c_int),
    # ctx, params, n_nodes, poses, n_edges, edge_nodes, edge_T, edge_info, edge_uncertain, edge_confidence, edge_kept, stats, trace
    "r3d_posegraph_optimize": _posegraph_optimize_sig,
    "r3d_posegraph_optimize_dev": _posegraph_optimize_sig,
    # ctx, params, n_nodes, poses, n_edges, edge_nodes, edge_T, edge_info, edge_uncertain, edge_confidence, e, l, H, b, F
    "r3d_debug_posegraph_linearize": ([_vp, ctypes.POINTER(PoseGraphParams), ctypes.c_int64, _vp, ctypes.c_int64, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                       _vp, _vp, ctypes.POINTER(ctypes.c_double)], ctypes.c_int),
    # ctx, n, A, b, lambda, L, delta, failed_pivot
    "r3d_debug_posegraph_solve": ([_vp, ctypes.c_int32, _vp, _vp, ctypes.c_double, _vp, _vp, ctypes.POINTER(ctypes.c_int32)], ctypes.c_int),
    # ctx, nv, nt, triangles, cap, edges, counts, stats, out_n
    "r3d_meshtopo_edges": ([_vp, _i64, _i64, _vp, _i64, _vp, _vp, _vp, _i64p], ctypes.c_int),
    "r3d_meshtopo_components": _meshtopo_components_sig,
    "r3d_meshtopo_components_dev": _meshtopo_components_sig,
    "r3d_meshtopo_dedup": _meshtopo_dedup_sig,
    "r3d_meshtopo_dedup_dev": _meshtopo_dedup_sig,
    # ctx, keys, values, n, bits, out_keys, out_values
    "r3d_debug_sort_pairs_u64": ([_vp, _vp, _vp, _i64, _i32, _vp, _vp], ctypes.c_int),
}


def exported_symbols():
    """Every symbol include/r3d.h declares (used by the CPU-side ABI test)."""
    return sorted(_SIGS)


torch_preloaded = None      # True / False once load() has run: whether torch's HIP runtime was in the process before ours


def _preload_torch():
    """ONE HIP runtime per process.  The PyTorch ROCm wheel bundles its own libamdhip64.so / libhsa-runtime64.so with the
    system library's SONAME (libamdhip64.so.7) but asks for it by the bare name libamdhip64.so: imported AFTER libr3d_hip.so
    (which needs libamdhip64.so.7 from /opt/rocm) the loader maps a SECOND runtime, and the second one finds no device
    ("no ROCm-capable device is detected"); imported BEFORE, our DT_NEEDED entry matches the SONAME already in the process and
    both share torch's runtime.  So when torch is installed it is imported first (set R3D_NO_TORCH_PRELOAD=1 to keep a
    torch-free process on the system runtime, e.g. for a rocprofv3 pass; distributed.init() then refuses to run)."""
    global torch_preloaded
    import sys
    if "torch" in sys.modules:
        torch_preloaded = True
    elif os.environ.get("R3D_NO_TORCH_PRELOAD") == "1":
        torch_preloaded = False
    else:
        import importlib.util
        if importlib.util.find_spec("torch") is not None:
            import torch  # noqa: F401
            torch_preloaded = True
        else:
            torch_preloaded = False


_allow_missing = False


def use_library(path, allow_missing=False):
    """Binds another build of libr3d_hip.so instead of lib/libr3d_hip.so; call it BEFORE the first load() (the A/B tools time
    the library of another commit against this one, process by process).  allow_missing: entry points that build does not
    export stay unbound (calling one raises AttributeError) instead of failing the load.  Returns the unbound names."""
    global LIB_PATH, _allow_missing
    if _lib is not None:
        raise RuntimeError("use_library: the library is already loaded")
    LIB_PATH, _allow_missing = os.path.abspath(path), bool(allow_missing)
    if not allow_missing:
        return []
    _preload_torch()
    lib = ctypes.CDLL(LIB_PATH)
    return [name for name in _SIGS if not hasattr(lib, name)]


def load():
    """Loads libr3d_hip.so (no GPU needed to dlopen; any compute call needs one)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with 3d_reconstruction_project_amd/csrc/build.sh "
                "(or __graft_entry__.build()). There is no CPU fallback.")
        _preload_torch()
        lib = ctypes.CDLL(LIB_PATH)
        for name, (argt, rest) in _SIGS.items():
            if _allow_missing and not hasattr(lib, name):
                continue
            fn = getattr(lib, name)
            fn.argtypes = argt
            fn.restype = rest
        _lib = lib
    return _lib


def register(sigs):
    """Lets sibling modules (cloud ops) add their entry points to the table before load()."""
    _SIGS.update(sigs)
    global _lib
    if _lib is not None:
        for name, (argt, rest) in sigs.items():
            fn = getattr(_lib, name)
            fn.argtypes = argt
            fn.restype = rest


def live_resources():
    """The library's live GPU resources over the whole process, as a dict (r3d_debug_resources; needs no context)."""
    c = ResourceCounts()
    rc = load().r3d_debug_resources(ctypes.byref(c))
    if rc != R3D_OK:
        raise R3DError(rc, "r3d_debug_resources failed")
    return {n: int(getattr(c, n)) for n, _ in ResourceCounts._fields_}


def ptr(a):
    """a numpy array's data as the void pointer the entry points take; None stays None (an absent array)"""
    return None if a is None else a.ctypes.data_as(_vp)


class R3DError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"{ERR_NAMES.get(code, code)}: {msg}")
        self.code = code


class Context:
    """One HIP device + stream + device workspace (r3d_ctx).  Not thread-safe: one Context per thread."""

    def __init__(self, device=0):
        self._lib = load()
        h = _vp()
        rc = self._lib.r3d_init(int(device), ctypes.byref(h))
        if rc != R3D_OK:
            raise R3DError(rc, (self._lib.r3d_last_error(None) or b"").decode())
        self._h = h
        self.device = int(device)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.r3d_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, rc):
        if rc != R3D_OK:
            raise R3DError(rc, (self._lib.r3d_last_error(self._h) or b"").decode())

    def call(self, name, *args):
        self.check(getattr(self._lib, name)(self._h, *args))

    def count_then_fill(self, name, head, n_outputs, alloc, n_counts=1):
        """The count / capacity protocol of an entry point whose arguments end (capacities..., outputs..., counts...): one call with
        capacities 0 and null outputs for the counts; alloc(*counts) -> the n_outputs host arrays in the entry point's order (None:
        an output it does not have); then, unless every count is 0, the call again with the counts as capacities, which must
        report the same counts.  -> (counts, arrays)"""
        def run(caps, outs):
            got = [ctypes.c_int64() for _ in caps]
            self.call(name, *head, *caps, *outs, *map(ctypes.byref, got))
            return tuple(g.value for g in got)
        counts = run((0,) * n_counts, (None,) * n_outputs)
        arrays = tuple(alloc(*counts))
        assert len(arrays) == n_outputs
        if any(counts):
            assert run(counts, [ptr(a) for a in arrays]) == counts
        return counts, arrays

    # --- memory / timing plumbing
    def alloc(self, nbytes):
        p = _vp()
        self.call("r3d_dev_alloc", ctypes.c_uint64(int(nbytes)), ctypes.byref(p))
        return p.value

    def free(self, ptr):
        self.call("r3d_dev_free", _vp(ptr))

    def h2d(self, dptr, arr):
        arr = np.ascontiguousarray(arr)
        self.call("r3d_copy_h2d", _vp(dptr), arr.ctypes.data_as(_vp), ctypes.c_uint64(arr.nbytes))

    def d2h(self, arr, dptr):
        assert arr.flags["C_CONTIGUOUS"]
        self.call("r3d_copy_d2h", arr.ctypes.data_as(_vp), _vp(dptr), ctypes.c_uint64(arr.nbytes))

    def to_device(self, arr):
        arr = np.ascontiguousarray(arr)
        p = self.alloc(arr.nbytes)
        self.h2d(p, arr)
        return p

    def sync(self):
        self.call("r3d_sync")

    def set_stream(self, stream_ptr):
        """stream_ptr: a hipStream_t handle as int; None / 0 = back to the context's own stream.  (The legacy null stream is
        NOT reachable as 0: pass HIP_STREAM_LEGACY, or use distributed.shared_stream(), which never hands a 0 handle over.)"""
        self.call("r3d_set_stream", _vp(stream_ptr))

    def get_stream(self):
        return self._lib.r3d_get_stream(self._h) or 0

    def event(self):
        e = _vp()
        self.call("r3d_event_create", ctypes.byref(e))
        return e.value

    def record(self, ev):
        self.call("r3d_event_record", _vp(ev))

    def wait_event(self, ev):
        """The context stream waits for the event (no host synchronisation)."""
        self.call("r3d_stream_wait_event", _vp(ev))

    def elapsed_ms(self, a, b):
        ms = ctypes.c_float()
        self.call("r3d_event_elapsed_ms", _vp(a), _vp(b), ctypes.byref(ms))
        return ms.value

    def selftest(self):
        self.call("r3d_selftest")

    def set_profiling(self, on):
        self.call("r3d_set_profiling", int(bool(on)))

    def sgbm_profile(self):
        ms = (ctypes.c_float * 16)()
        names = ctypes.create_string_buffer(512)
        n = self._lib.r3d_sgbm_profile(self._h, ms, 16, names, 512)
        if n < 0:
            self.check(n)
        parts = names.raw.split(b"\0")
        return {parts[i].decode(): ms[i] for i in range(n)}


_default_ctx = {}


def default_context(device=0):
    if device not in _default_ctx:
        _default_ctx[device] = Context(device)
    return _default_ctx[device]


def parse_device(device):
    """'CUDA:0' / 'HIP:0' / 0 -> device index (the reference passes o3d.core.Device('CUDA:0') strings)."""
    if isinstance(device, int):
        return device
    s = str(device).upper()
    if s.startswith("CPU"):
        raise R3DError(-4, "this library has no CPU backend; pass 'CUDA:<n>' / 'HIP:<n>'")
    if ":" in s:
        return int(s.split(":")[1])
    return 0
