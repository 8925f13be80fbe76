"""ctypes binding of include/videovec.h and a small host-side engine object.

Mirrors the reference's solver-side view of the path (Solver::Solve loop body, solver.cpp:194-220):
`forward_backward()` == Net::ForwardBackward, `apply_update()` == ComputeUpdateValue + Net::Update.
"""
import contextlib
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
PREC = {"f16": 0, "bf16": 1}


class VVError(RuntimeError):
    """code: the VV_ERR_* value of the call that failed, where one call did (None otherwise)."""

    def __init__(self, msg, code=None):
        super().__init__(msg)
        self.code = code


def lib_path():
    """The product library.  VV_LIB names another build of the same ABI (tools/lab/*: the -DVV_LAB build with the ablated
    kernels; A/B of two builds); it must exist -- nothing falls back."""
    return os.environ.get("VV_LIB") or os.path.join(_HERE, "lib", "libvideovec.so")


class _StepCfg(C.Structure):
    _fields_ = [("B", C.c_int32), ("C", C.c_int32), ("Nn", C.c_int32),
                ("margin", C.c_float), ("norm", C.c_int32), ("loss_weight", C.c_float),
                ("ctx_coeff", C.c_void_p),
                ("dropout_ratio", C.c_float), ("dropout_mask", C.c_void_p),
                ("dropout_seed", C.c_uint64), ("global_count", C.c_int64),
                ("lr", C.c_float), ("momentum", C.c_float), ("weight_decay", C.c_float),
                ("lr_mult", C.c_float * 2), ("decay_mult", C.c_float * 2), ("reg", C.c_int32),
                ("solver_type", C.c_int32), ("delta", C.c_float), ("ip_regularization", C.c_float),
                ("item_weight", C.c_void_p)]


_lib = None


class _BoxProbe(C.Structure):
    _fields_ = [("gemm_tflops", C.c_double), ("gemm_ms", C.c_double), ("gemm_clock_mhz", C.c_double),
                ("copy_tbs", C.c_double), ("copy_ms", C.c_double),
                ("gemm_rows", C.c_int32), ("gemm_k", C.c_int32), ("gemm_n", C.c_int32), ("gemm_launches", C.c_int32),
                ("copy_bytes", C.c_int64)]


class _RankStats(C.Structure):
    _fields_ = [("median_rank", C.c_float), ("recall_1", C.c_float), ("recall_5", C.c_float), ("recall_10", C.c_float),
                ("mean_ap", C.c_float)]


class _H16Report(C.Structure):
    _fields_ = [("saturated", C.c_int64), ("faint_rows", C.c_int64), ("flagged_steps", C.c_int64),
                ("first_flagged_step", C.c_int64), ("fallback", C.c_int32), ("rows_f16", C.c_int32)]


class _ClipReport(C.Structure):
    _fields_ = [("norm", C.c_float), ("scale", C.c_float), ("clipped", C.c_int32), ("reserved_", C.c_int32),
                ("updates", C.c_int64), ("clipped_updates", C.c_int64)]


class _EmaReport(C.Structure):
    _fields_ = [("updates", C.c_int64), ("decay", C.c_float), ("in_use", C.c_int32)]


class _AbsStat(C.Structure):
    _fields_ = [("asum", C.c_double), ("amax", C.c_float), ("reserved_", C.c_int32), ("count", C.c_int64), ("nonfinite", C.c_int64)]


# include/videovec.h's VV_STAT_* in order: name -> bit of vv_debug_stats_queue's mask, index of vv_debug_stats_get's record
STAT_NAMES = ("W", "B", "HIST_W", "HIST_B", "DW", "DB", "TARGET_SCORE", "NEGATIVE_SCORES", "UPD_W", "UPD_B")


class _AccumReport(C.Structure):
    _fields_ = [("banked", C.c_int32), ("last_count", C.c_int32), ("last_mean_loss", C.c_float), ("last_mean_violations", C.c_float),
                ("updates", C.c_int64)]


class _EvalReport(C.Structure):
    _fields_ = [("passes", C.c_int64), ("terms", C.c_int64), ("loss_sum", C.c_double), ("viol_sum", C.c_double),
                ("last_loss", C.c_float), ("last_violations", C.c_float), ("mean_loss", C.c_float), ("mean_violations", C.c_float)]


class EvalStats:
    """vv_eval_report: the forward-only passes since eval_reset().  last_* / mean_* are np.float32, the sums Python floats (double)."""
    __slots__ = ("passes", "terms", "loss_sum", "viol_sum", "last_loss", "last_violations", "mean_loss", "mean_violations")

    def __init__(self, r):
        self.passes, self.terms = int(r.passes), int(r.terms)
        self.loss_sum, self.viol_sum = float(r.loss_sum), float(r.viol_sum)
        self.last_loss, self.last_violations = np.float32(r.last_loss), np.float32(r.last_violations)
        self.mean_loss, self.mean_violations = np.float32(r.mean_loss), np.float32(r.mean_violations)

    def __repr__(self):
        return "EvalStats(%s)" % ", ".join("%s=%r" % (k, getattr(self, k)) for k in self.__slots__)


class _ClassStats(C.Structure):
    _fields_ = [("mean_ap", C.c_float), ("hit_at_1", C.c_float), ("hit_at_5", C.c_float), ("n_scored", C.c_int32)]


class _ClassificationReport(C.Structure):
    _fields_ = [("total_accuracy", C.c_float), ("mean_ap", C.c_float), ("classes_present", C.c_int32), ("reserved_", C.c_int32),
                ("n", C.c_int64)]


class _LinearCfg(C.Structure):
    _fields_ = [("iters", C.c_int32), ("batch", C.c_int32), ("lr", C.c_float), ("momentum", C.c_float), ("weight_decay", C.c_float),
                ("loss_weight", C.c_float)]


class _LinearReport(C.Structure):
    _fields_ = [("loss_first", C.c_float), ("loss_last", C.c_float), ("accuracy_last", C.c_float), ("reserved_", C.c_int32),
                ("steps", C.c_int64), ("nonfinite_rows", C.c_int64)]


class _KmeansCfg(C.Structure):
    _fields_ = [("num_clusters", C.c_int32), ("iters", C.c_int32), ("metric", C.c_int32), ("reserved_", C.c_int32)]


class _KmeansReport(C.Structure):
    _fields_ = [("n", C.c_int64), ("num_clusters", C.c_int32), ("iters", C.c_int32), ("empty_last", C.c_int32),
                ("degenerate_last", C.c_int32), ("moved_last", C.c_int64), ("objective_last", C.c_double), ("nonfinite_rows", C.c_int64)]


def load_library():
    """Load libvideovec.so; raises (never falls back) when the HIP library is not built."""
    global _lib
    if _lib is not None:
        return _lib
    # PyTorch wheels bundle their own libamdhip64 with the same SONAME as /opt/rocm's.  Whichever is
    # loaded first serves the whole process, and torch fails ("no ROCm-capable device") when it finds the
    # system runtime already loaded: import torch first so streams / tensors / RCCL and this library
    # share ONE HIP runtime.
    if "torch" not in __import__("sys").modules and not os.environ.get("VV_NO_TORCH_PRELOAD"):
        try:
            import torch  # noqa: F401
        except Exception:
            pass
    p = lib_path()
    if not os.path.exists(p):
        raise VVError("%s is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                      "(hipcc --offload-arch=gfx950); there is no CPU fallback" % p)
    L = C.CDLL(p)
    L.vv_last_error.restype = C.c_char_p
    L.vv_version.restype = C.c_char_p
    vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
    sigs = {
        "vv_create": [C.c_int, C.c_int, C.POINTER(vp)],
        "vv_destroy": [vp], "vv_set_stream": [vp, vp], "vv_synchronize": [vp],
        "vv_device_query": [C.c_int, C.c_char_p, C.c_size_t],
        "vv_set_option": [vp, C.c_char_p, C.c_double], "vv_get_option": [vp, C.c_char_p, C.POINTER(C.c_double)],
        "vv_set_dedup": [vp, C.c_int], "vv_dedup_stats": [vp, C.POINTER(i64), C.POINTER(i64)],
        "vv_grad_scale_stats": [vp, C.POINTER(i64), C.POINTER(C.c_float)],
        "vv_h16_stats": [vp, C.POINTER(_H16Report)],
        "vv_table_set": [vp, vp, i64, i32], "vv_table_synth": [vp, C.c_uint64, i64, i32],
        "vv_table_get": [vp, vp, i64, vp],
        "vv_params_set": [vp, i32, vp, vp, vp, vp], "vv_params_get": [vp, vp, vp, vp, vp],
        "vv_step_cfg_default": [vp],
        "vv_forward_backward": [vp, vp, vp, C.c_int], "vv_apply_update": [vp, vp],
        "vv_forward_backward_q1": [vp, vp, vp, vp],
        "vv_step": [vp, vp, vp, C.c_int],
        "vv_update_hint": [vp, vp],
        "vv_forward_backward_ring": [vp, vp, vp, i32, i32, vp, C.c_double],
        "vv_dev_alloc": [vp, C.c_size_t, C.POINTER(vp)], "vv_dev_free": [vp, vp],
        "vv_dev_upload": [vp, vp, vp, C.c_size_t], "vv_dev_download": [vp, vp, vp, C.c_size_t],
        "vv_dev_memset": [vp, vp, C.c_int, C.c_size_t],
        "vv_op_copy2d": [vp, vp, i64, vp, i64, i64, i64, C.c_int],
        "vv_op_axpby": [vp, i64, f32, vp, f32, vp], "vv_op_mul": [vp, i64, vp, vp, vp, C.c_int],
        "vv_op_relu": [vp, i64, vp, vp, f32], "vv_op_relu_bwd": [vp, i64, vp, vp, vp, f32],
        "vv_op_dropout": [vp, i64, vp, vp, vp, f32, C.c_uint64, C.c_int],
        "vv_op_rowsum": [vp, i64, i32, vp, i32, vp], "vv_op_rowsum_bwd": [vp, i64, i32, i32, vp, vp],
        "vv_op_normalize": [vp, i64, i32, vp, vp], "vv_op_normalize_bwd": [vp, i64, i32, vp, vp, vp],
        "vv_op_max_margin": [vp, i32, vp, vp, vp, f32, i32, C.POINTER(f32), C.POINTER(f32)],
        "vv_op_max_margin_bwd": [vp, i32, vp, vp, vp, f32, i32, f32, vp, vp],
        "vv_op_gather_rows": [vp, vp, i64, vp],
        "vv_op_inner_product": [vp, vp, i64, vp], "vv_op_inner_product_bwd": [vp, vp, i64, f32],
        "vv_op_gram": [vp, vp, i32, i32, f32, vp],
        "vv_comm_init": [vp, i32, i32, C.c_char_p, i32], "vv_comm_overlap": [vp, C.c_int], "vv_comm_schedule": [vp, C.c_int],
        "vv_allreduce_grads": [vp], "vv_comm_destroy": [vp],
        "vv_loss_get": [vp, C.POINTER(f32), C.POINTER(f32)],
        "vv_grads_device": [vp, C.POINTER(vp), C.POINTER(i64)], "vv_grads_get": [vp, vp, vp],
        "vv_grads_bind": [vp, vp],
        "vv_blobs_get": [vp, vp, vp, vp, vp],
        "vv_dedup_groups_get": [vp, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(f32)],
        "vv_embed": [vp, vp, i64, C.c_int, C.c_int, vp],
        "vv_embed_mean": [vp, vp, i64, i32, vp, C.c_int, C.c_int, vp],
        "vv_retrieval_stats": [vp, vp, i32, i32, vp, vp, vp, i32, C.c_int, C.POINTER(f32), C.POINTER(f32), C.POINTER(f32)],
        "vv_gallery_create": [vp, vp, i64, i32, vp, C.POINTER(vp)],
        "vv_gallery_from_table": [vp, vp, i64, i32, vp, C.c_int, C.c_int, vp, C.POINTER(vp)],
        "vv_gallery_destroy": [vp, vp],
        "vv_gallery_topk": [vp, vp, vp, i32, i32, vp, vp],
        "vv_gallery_rank_stats": [vp, vp, vp, i32, vp, C.POINTER(_RankStats), vp, vp, vp, vp],
        "vv_gallery_get": [vp, C.c_char_p, C.POINTER(C.c_double)],
        "vv_gallery_pool_by_id": [vp, vp, C.POINTER(vp)],
        "vv_gallery_class_stats": [vp, vp, vp, vp, i32, C.c_int, C.POINTER(_ClassStats), vp, vp, vp, vp],
        "vv_gallery_nearest": [vp, vp, vp, i32, vp, i32, vp, vp],
        "vv_gallery_nearest_self": [vp, vp, i32, C.c_int, vp, vp],
        "vv_gallery_scores": [vp, vp, vp, i32, vp],
        "vv_gallery_knn_scores": [vp, vp, vp, i32, vp, i32, vp, i32, i32, f32, vp, vp],
        "vv_gallery_knn_scores_self": [vp, vp, vp, i32, i32, C.c_int, i32, f32, vp, vp],
        "vv_kmeans_cfg_default": [C.POINTER(_KmeansCfg)],
        "vv_gallery_kmeans": [vp, vp, C.POINTER(_KmeansCfg), vp, vp, vp, vp, vp, vp, vp, C.POINTER(_KmeansReport)],
        "vv_kmeans_init_rows": [C.c_uint64, i32, i32, vp],
        "vv_ivf_create": [vp, vp, vp, i32, i32, vp, C.POINTER(vp)], "vv_ivf_destroy": [vp, vp],
        "vv_ivf_search": [vp, vp, vp, i32, i32, i32, vp, vp, vp],
        "vv_ivf_get": [vp, C.c_char_p, C.POINTER(C.c_double)], "vv_ivf_lists": [vp, vp, vp, vp],
        "vv_pq_train": [vp, vp, i32, i32, i32, C.c_uint64, vp, vp], "vv_pq_encode": [vp, vp, vp, i32, i32, vp],
        "vv_ivfpq_create": [vp, vp, vp, i32, i32, vp, vp, i32, i32, C.POINTER(vp)], "vv_ivfpq_destroy": [vp, vp],
        "vv_ivfpq_search": [vp, vp, vp, i32, i32, i32, vp, vp, vp],
        "vv_ivfpq_get": [vp, C.c_char_p, C.POINTER(C.c_double)], "vv_ivfpq_lists": [vp, vp, vp, vp], "vv_ivfpq_codes": [vp, vp, vp],
        "vv_classification_stats": [vp, vp, i64, i32, vp, C.c_int, vp, vp, vp, C.POINTER(_ClassificationReport)],
        "vv_linear_create": [vp, i32, i32, C.c_int, C.POINTER(vp)], "vv_linear_destroy": [vp, vp],
        "vv_linear_get": [vp, vp, vp, vp, vp, vp, C.POINTER(i64)], "vv_linear_put": [vp, vp, vp, vp, vp, vp, i64],
        "vv_linear_cfg_default": [C.POINTER(_LinearCfg)],
        "vv_linear_fit": [vp, vp, vp, vp, C.POINTER(_LinearCfg), vp, vp, C.POINTER(_LinearReport)],
        "vv_linear_grad": [vp, vp, vp, vp, i64, i64, f32, vp, vp, C.POINTER(f32)],
        "vv_linear_scores": [vp, vp, vp, vp, i64, vp],
        "vv_op_softmax_loss": [vp, vp, i64, i32, i64, vp, f32, vp, vp, C.POINTER(f32), C.POINTER(i64)],
        "vv_linear_loss_set": [vp, vp, i32, i32], "vv_linear_loss_get": [vp, vp, C.POINTER(i32), C.POINTER(i32)],
        "vv_op_hinge_loss": [vp, vp, i64, i32, i64, vp, i32, f32, vp, C.POINTER(f32), C.POINTER(i64)],
        "vv_op_gemm_tn": [vp, vp, i64, vp, i64, i64, i32, i32, vp],
        "vv_linear_fit_rows": [vp, vp, vp, vp, vp, i64, C.POINTER(_LinearCfg), vp, vp, C.POINTER(_LinearReport)],
        "vv_linear_grad_rows": [vp, vp, vp, vp, vp, i64, f32, vp, vp, C.POINTER(f32)],
        "vv_linear_scores_rows": [vp, vp, vp, vp, i64, vp],
        "vv_rows_shuffled": [C.c_uint64, i32, i32, vp],
        "vv_rows_fold": [C.c_uint64, i32, i32, i32, vp, C.POINTER(i64), vp, C.POINTER(i64)],
        "vv_profile_enable": [vp, C.c_int],
        "vv_profile_select": [vp, C.c_char_p],
        "vv_profile_get": [vp, C.c_char_p, C.POINTER(C.c_double), C.POINTER(i64)],
        "vv_box_probe": [vp, C.POINTER(_BoxProbe)],
        "vv_solver_ext_set": [vp, f32, f32], "vv_solver_ext_get": [vp, C.POINTER(f32), C.POINTER(f32)],
        "vv_solver_iter_set": [vp, i64], "vv_solver_iter_get": [vp, C.POINTER(i64)],
        "vv_history2_set": [vp, vp, vp], "vv_history2_get": [vp, vp, vp],
        "vv_clip_gradients_set": [vp, f32], "vv_clip_gradients_get": [vp, C.POINTER(f32)],
        "vv_clip_stats": [vp, C.POINTER(_ClipReport)],
        "vv_grads_bank": [vp], "vv_grads_bank_reset": [vp], "vv_accum_stats": [vp, C.POINTER(_AccumReport)],
        "vv_forward": [vp, vp, vp, C.c_int], "vv_eval_reset": [vp], "vv_eval_stats": [vp, C.POINTER(_EvalReport)],
        "vv_op_asum": [vp, vp, i64, C.POINTER(_AbsStat)],
        "vv_debug_stats_queue": [vp, C.c_uint32], "vv_debug_mark_update": [vp], "vv_debug_stats_get": [vp, C.POINTER(_AbsStat)],
        "vv_ema_set": [vp, f32], "vv_ema_get_decay": [vp, C.POINTER(f32)], "vv_ema_get": [vp, vp, vp], "vv_ema_put": [vp, vp, vp], "vv_ema_use": [vp, C.c_int],
        "vv_ema_stats": [vp, C.POINTER(_EmaReport)],
        "vv_run_state_size": [vp, C.POINTER(i64)], "vv_run_state_get": [vp, vp, i64, C.POINTER(i64)], "vv_run_state_put": [vp, vp, i64],
        "vv_sampler_state_size": [vp, C.POINTER(i64)], "vv_sampler_state_get": [vp, vp, i64, C.POINTER(i64)],
        "vv_sampler_state_put": [vp, vp, i64],
    }
    for name, args in sigs.items():
        fn = getattr(L, name)
        fn.argtypes = args
        fn.restype = None if name in ("vv_step_cfg_default", "vv_linear_cfg_default", "vv_kmeans_cfg_default") else C.c_int
    L.vv_sampler_state_error.argtypes = []
    L.vv_sampler_state_error.restype = C.c_char_p
    _lib = L
    return L


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


KNN_WEIGHTINGS = {"uniform": 0, "exp": 1}      # VV_KNN_UNIFORM, VV_KNN_EXP
KMEANS_METRICS = {"euclidean": 0, "spherical": 1}      # VV_KMEANS_EUCLIDEAN, VV_KMEANS_SPHERICAL


def kmeans_init_rows(seed, n, num_clusters):
    """vv_kmeans_init_rows: int32 [num_clusters] distinct item indices, the head of rows_shuffled(seed, n, 1)."""
    out = np.zeros(max(int(num_clusters), 1), np.int32)
    _rows_chk(load_library().vv_kmeans_init_rows(int(seed) & 0xFFFFFFFFFFFFFFFF, int(n), int(num_clusters), _ptr(out)))
    return out[:int(num_clusters)].copy()


class KMeansResult:
    """What Gallery.kmeans returns: centroids fp32 [C][dim], assign int32 [n_ref], counts int32 [C], objective float64 [iters + 1],
    moved int64 [iters + 1], report (dict of vv_kmeans_report's fields), metric (VV_KMEANS_*); gallery() puts the centroids on the
    device as a Gallery, ivf(items) builds an inverted-file index of `items` on them, ivfpq(items, codebooks) one that keeps
    product-quantised codes."""

    def __init__(self, eng, centroids, assign, counts, objective, moved, report, metric=0):
        self.eng, self.centroids, self.assign, self.counts = eng, centroids, assign, counts
        self.objective, self.moved, self.report, self.metric = objective, moved, report, metric

    def gallery(self):
        return self.eng.gallery(self.centroids)

    def ivf(self, items):
        """An IVFIndex of the Gallery `items` on these centroids under this clustering's metric; the index assigns for itself."""
        return self.eng.ivf(items, self.centroids, metric=self.metric, assign=None)

    def ivfpq(self, items, codebooks):
        """An IVFPQIndex of the Gallery `items` on these centroids under this clustering's metric, coded against `codebooks`
        (Engine.pq_train); the index assigns for itself."""
        return self.eng.ivfpq(items, self.centroids, codebooks, metric=self.metric, assign=None)


class _CoarseIndex:
    """What IVFIndex and IVFPQIndex share; `_fn` is the C functions' prefix (vv_ivf, vv_ivfpq)."""
    _fn = None

    def __init__(self, eng, handle):
        self.eng, self.h = eng, handle

    def _call(self, what):
        return getattr(self.eng.L, "%s_%s" % (self._fn, what))

    def get(self, name):
        v = C.c_double()
        self.eng._chk(self._call("get")(self.h, name.encode(), C.byref(v)))
        return v.value

    n_ref = property(lambda self: int(self.get("n_ref")))
    dim = property(lambda self: int(self.get("dim")))
    num_clusters = property(lambda self: int(self.get("num_clusters")))

    def search(self, q, k, nprobe):
        """(idx int32 [n_q][k], dist fp32 [n_q][k], n_candidates int32 [n_q]): the k <= 32 nearest items -- on an IVFPQIndex, those of
        smallest approximate distance -- among those of each query's nprobe nearest clusters, ascending (distance, item index); slots
        past a query's candidates read -1 / 0."""
        q = np.ascontiguousarray(q, dtype=np.float32)
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise VVError("queries must be [n_q][%d]" % self.dim)
        idx = np.empty((q.shape[0], max(int(k), 0)), np.int32)
        dist = np.empty(idx.shape, np.float32)
        ncand = np.zeros(q.shape[0], np.int32)
        self.eng._chk(self._call("search")(self.eng.h, self.h, _ptr(q), q.shape[0], int(nprobe), int(k), _ptr(idx), _ptr(dist), _ptr(ncand)))
        return idx, dist, ncand

    def lists(self):
        """(start int32 [C + 1], list int32 [n_ref]): cluster c's items, ascending, are list[start[c]:start[c + 1]]."""
        start = np.zeros(self.num_clusters + 1, np.int32)
        lst = np.zeros(self.n_ref, np.int32)
        self.eng._chk(self._call("lists")(self.eng.h, self.h, _ptr(start), _ptr(lst)))
        return start, lst

    def close(self):
        if self.h is not None:
            h, self.h = self.h, None
            if self.eng.h:                      # (an engine closed first took its device with it)
                self.eng._chk(self._call("destroy")(self.eng.h, h))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class IVFIndex(_CoarseIndex):
    """An inverted-file index held on the device by an Engine (vv_ivf_create; include/videovec.h states the arithmetic)."""
    _fn = "vv_ivf"


class IVFPQIndex(_CoarseIndex):
    """An inverted-file index of product-quantised codes held on the device by an Engine (vv_ivfpq_create; include/videovec.h states
    the arithmetic): M one-byte codes per item in place of its fp32 row."""
    _fn = "vv_ivfpq"
    M = property(lambda self: int(self.get("M")))

    def codes(self):
        """uint8 [n_ref][M] in list-position order: row p holds the codes of item lists()[1][p]."""
        out = np.zeros((self.n_ref, self.M), np.uint8)
        self.eng._chk(self.eng.L.vv_ivfpq_codes(self.eng.h, self.h, _ptr(out)))
        return out


class Gallery:
    """A reference set held on the device by an Engine (RetrievalRankStatsFixedRefLayer's bottom[2] / bottom[3])."""

    def __init__(self, eng, handle, ids=None):
        self.eng, self.h, self.ids = eng, handle, ids          # ids: the int32 [n_ref] the gallery was created with, or None

    def get(self, name):
        v = C.c_double()
        self.eng._chk(self.eng.L.vv_gallery_get(self.h, name.encode(), C.byref(v)))
        return v.value

    @property
    def n_ref(self):
        return int(self.get("n_ref"))

    @property
    def dim(self):
        return int(self.get("dim"))

    @property
    def scratch_bytes(self):
        return int(self.get("scratch_bytes"))

    def _queries(self, q):
        q = np.ascontiguousarray(q, dtype=np.float32)
        if q.ndim != 2 or q.shape[1] != self.dim:
            raise VVError("queries must be [n_q][%d]" % self.dim)
        return q

    def topk(self, q, k):
        """(idx int32 [n_q][k], dist fp32 [n_q][k]): the k nearest reference items, ascending (distance, index)."""
        q = self._queries(q)
        idx = np.empty((q.shape[0], max(int(k), 0)), np.int32)
        dist = np.empty(idx.shape, np.float32)
        self.eng._chk(self.eng.L.vv_gallery_topk(self.eng.h, self.h, _ptr(q), q.shape[0], int(k), _ptr(idx), _ptr(dist)))
        return idx, dist

    def nearest(self, q, k, q_ids=None):
        """(idx int32 [n_q][k], dist fp32 [n_q][k]): the k <= 2048 nearest reference items, ascending (distance, index); with q_ids
        [n_q] only items whose id differs from the query's.  Slots past a query's eligible items read -1 / 0."""
        q = self._queries(q)
        qid = None
        if q_ids is not None:
            qid = np.ascontiguousarray(q_ids, dtype=np.int32)
            if qid.shape != (q.shape[0],):
                raise VVError("nearest: q_ids must be [n_q]")
        idx = np.empty((q.shape[0], max(int(k), 0)), np.int32)
        dist = np.empty(idx.shape, np.float32)
        self.eng._chk(self.eng.L.vv_gallery_nearest(self.eng.h, self.h, _ptr(q), q.shape[0], _ptr(qid), int(k), _ptr(idx), _ptr(dist)))
        return idx, dist

    def nearest_self(self, k, exclude_same_id=False):
        """(idx int32 [n_ref][k], dist fp32 [n_ref][k]): every item's k <= 2048 nearest OTHER items of the gallery; with
        exclude_same_id only items of another id.  Slots past an item's eligible items read -1 / 0."""
        idx = np.empty((self.n_ref, max(int(k), 0)), np.int32)
        dist = np.empty(idx.shape, np.float32)
        self.eng._chk(self.eng.L.vv_gallery_nearest_self(self.eng.h, self.h, int(k), int(bool(exclude_same_id)), _ptr(idx), _ptr(dist)))
        return idx, dist

    def rank_stats(self, q, q_ids, per_query=False):
        """dict(median_rank, recall_1, recall_5, recall_10, mean_ap); with per_query also best_rank [n_q], ap [n_q],
        top5_idx / top5_dist [n_q][5]."""
        q = self._queries(q)
        qid = np.ascontiguousarray(q_ids, dtype=np.int32)
        if qid.shape != (q.shape[0],):
            raise VVError("rank_stats: q_ids must be [n_q]")
        st = _RankStats()
        n = q.shape[0]
        br = np.empty(n, np.int32) if per_query else None
        ap = np.empty(n, np.float32) if per_query else None
        t5i = np.empty((n, 5), np.int32) if per_query else None
        t5d = np.empty((n, 5), np.float32) if per_query else None
        self.eng._chk(self.eng.L.vv_gallery_rank_stats(self.eng.h, self.h, _ptr(q), n, _ptr(qid), C.byref(st), _ptr(br), _ptr(ap),
                                                       _ptr(t5i), _ptr(t5d)))
        out = {f: getattr(st, f) for f, _ in _RankStats._fields_}
        if per_query:
            out.update(best_rank=br, ap=ap, top5_idx=t5i, top5_dist=t5d)
        return out

    def scores(self, q, out_dev=None):
        """The fp32 dot products of q [n_q][dim] with every reference item into DEVICE memory (vv_gallery_scores): out_dev is a
        DevBuf (or a device pointer) of [n_q][n_ref] floats; None allocates one.  Returns it -- get() downloads, and it feeds
        Engine.classification_stats without a host round trip."""
        q = self._queries(q)
        if out_dev is None:
            out_dev = DevBuf(self.eng, (q.shape[0], self.n_ref))
        ptr = out_dev.ptr if isinstance(out_dev, DevBuf) else C.c_void_p(int(out_dev.value if isinstance(out_dev, C.c_void_p) else out_dev))
        self.eng._chk(self.eng.L.vv_gallery_scores(self.eng.h, self.h, _ptr(q), q.shape[0], ptr))
        return out_dev

    def _knn_args(self, labels, num_classes, n_q, weighting, out, n_used):
        lab = np.ascontiguousarray(labels, dtype=np.int32)
        if lab.shape != (self.n_ref,):
            raise VVError("knn_scores: labels must be [n_ref]")
        if isinstance(weighting, str):                    # (an integer goes to the library as it is: VV_KNN_*)
            if weighting not in KNN_WEIGHTINGS:
                raise VVError("knn_scores: weighting must be one of %s" % ", ".join(sorted(KNN_WEIGHTINGS)))
            weighting = KNN_WEIGHTINGS[weighting]
        if out is None:
            out = DevBuf(self.eng, (n_q, max(int(num_classes), 1)))
        used = np.zeros(n_q, np.int32) if n_used else None
        return lab, int(weighting), out, used

    def knn_scores(self, q, labels, num_classes, k, q_ids=None, weighting="uniform", temperature=0.07, out=None, n_used=False):
        """The k-nearest-neighbour classifier's scores of q [n_q][dim] in DEVICE memory (vv_gallery_knn_scores): a DevBuf of
        [n_q][num_classes] floats, score[i][c] = the share of class c among the weights of query i's k <= 2048 nearest items (the
        lists of nearest(q, k, q_ids)); labels [n_ref]: the class of every item, in 0 .. num_classes - 1 (<= 4096).  weighting
        "uniform": every neighbour counts 1; "exp": exp((s_j - s_0) / temperature) with s the dot products.  out: a DevBuf (or a
        device pointer) to write instead of a new one.  n_used=True: returns (scores, m int32 [n_q]), m the neighbours each row had.
        The result feeds Engine.classification_stats without a host round trip."""
        q = self._queries(q)
        qid = None
        if q_ids is not None:
            qid = np.ascontiguousarray(q_ids, dtype=np.int32)
            if qid.shape != (q.shape[0],):
                raise VVError("knn_scores: q_ids must be [n_q]")
        lab, w, out, used = self._knn_args(labels, num_classes, q.shape[0], weighting, out, n_used)
        self.eng._chk(self.eng.L.vv_gallery_knn_scores(self.eng.h, self.h, _ptr(lab), int(num_classes), _ptr(q), q.shape[0], _ptr(qid),
                                                       int(k), w, float(temperature), _dev_ptr(out), _ptr(used)))
        return (out, used) if n_used else out

    def knn_scores_self(self, labels, num_classes, k, exclude_same_id=False, weighting="uniform", temperature=0.07, out=None,
                        n_used=False):
        """As knn_scores with every gallery item as a query against the others (vv_gallery_knn_scores_self, the lists of
        nearest_self): leave-one-item-out k-NN, with exclude_same_id leave-one-id-out.  [n_ref][num_classes]."""
        lab, w, out, used = self._knn_args(labels, num_classes, self.n_ref, weighting, out, n_used)
        self.eng._chk(self.eng.L.vv_gallery_knn_scores_self(self.eng.h, self.h, _ptr(lab), int(num_classes), int(k),
                                                            int(bool(exclude_same_id)), w, float(temperature), _dev_ptr(out), _ptr(used)))
        return (out, used) if n_used else out

    def kmeans(self, num_clusters, iters=20, metric="euclidean", init=None, seed=0):
        """k-means over the gallery's items on the device (vv_gallery_kmeans; include/videovec.h states the arithmetic): a KMeansResult.
        metric "euclidean" or "spherical".  init: None -- the rows kmeans_init_rows(seed, n_ref, num_clusters); a float array
        [num_clusters][dim] -- the initial centroids; an integer array [num_clusters] -- the items whose device rows start as centroids."""
        Cn = int(num_clusters)
        if isinstance(metric, str):                       # (an integer goes to the library as it is: VV_KMEANS_*)
            if metric not in KMEANS_METRICS:
                raise VVError("kmeans: metric must be one of %s" % ", ".join(sorted(KMEANS_METRICS)))
            metric = KMEANS_METRICS[metric]
        cfg = _KmeansCfg()
        self.eng.L.vv_kmeans_cfg_default(C.byref(cfg))
        cfg.num_clusters, cfg.iters, cfg.metric = Cn, int(iters), int(metric)
        cent0 = rows0 = None
        if init is None:
            rows0 = kmeans_init_rows(seed, self.n_ref, Cn)
        else:
            a = np.asarray(init)
            if a.dtype.kind in "iu":
                rows0 = np.ascontiguousarray(a, dtype=np.int32).reshape(-1)
                if rows0.shape != (Cn,):
                    raise VVError("kmeans: init rows must be [num_clusters]")
            else:
                cent0 = np.ascontiguousarray(a, dtype=np.float32)
                if cent0.shape != (Cn, self.dim):
                    raise VVError("kmeans: init centroids must be [num_clusters][%d]" % self.dim)
        passes = max(int(iters), 0) + 1
        cent = np.zeros((max(Cn, 1), self.dim), np.float32)
        assign = np.zeros(self.n_ref, np.int32)
        counts = np.zeros(max(Cn, 1), np.int32)
        obj, moved = np.zeros(passes, np.float64), np.zeros(passes, np.int64)
        rep = _KmeansReport()
        self.eng._chk(self.eng.L.vv_gallery_kmeans(self.eng.h, self.h, C.byref(cfg), _ptr(cent0), _ptr(rows0), _ptr(cent), _ptr(assign),
                                                   _ptr(counts), _ptr(obj), _ptr(moved), C.byref(rep)))
        return KMeansResult(self.eng, cent, assign, counts, obj, moved, {f: getattr(rep, f) for f, _ in _KmeansReport._fields_}, int(metric))

    def rows(self):
        """The gallery's fp32 rows [n_ref][dim], downloaded from the device."""
        pitch = int(self.get("row_floats"))
        buf = np.empty((self.n_ref, pitch), np.float32)
        self.eng._chk(self.eng.L.vv_dev_download(self.eng.h, _ptr(buf), C.c_void_p(int(self.get("feat_device"))), buf.nbytes))
        return np.ascontiguousarray(buf[:, :self.dim])

    def pool_by_id(self):
        """A new Gallery with one item per distinct id, ids ascending, each row the mean of the id's rows (RetrievalStatsLayer's
        video_level_retrieval); its `ids` are those ids."""
        h = C.c_void_p()
        self.eng._chk(self.eng.L.vv_gallery_pool_by_id(self.eng.h, self.h, C.byref(h)))
        ids = None if self.ids is None else np.unique(self.ids).astype(np.int32)
        return Gallery(self.eng, h, ids)

    def class_stats(self, id2class, exclude_same_video=True, per_query=False):
        """RetrievalStatsLayer over the gallery's own items, every item a query against all the others: dict(mean_ap, hit_at_1,
        hit_at_5, n_scored); with per_query also ap / acc1 / acc5 [n_ref] (NaN for a query of negative class) and top5_idx
        [n_ref][5] (the nearest items of other ids, -1 where fewer exist).  id2class: {id: class}, an absent id reads as class 0."""
        mi = np.ascontiguousarray(list(id2class.keys()), dtype=np.int32)
        mc = np.ascontiguousarray(list(id2class.values()), dtype=np.int32)
        n = self.n_ref
        st = _ClassStats()
        ap = np.empty(n, np.float32) if per_query else None
        a1 = np.empty(n, np.float32) if per_query else None
        a5 = np.empty(n, np.float32) if per_query else None
        t5 = np.empty((n, 5), np.int32) if per_query else None
        self.eng._chk(self.eng.L.vv_gallery_class_stats(self.eng.h, self.h, _ptr(mi), _ptr(mc), len(mi), int(bool(exclude_same_video)),
                                                        C.byref(st), _ptr(ap), _ptr(a1), _ptr(a5), _ptr(t5)))
        out = {f: getattr(st, f) for f, _ in _ClassStats._fields_}
        if per_query:
            out.update(ap=ap, acc1=a1, acc5=a5, top5_idx=t5)
        return out

    def close(self):
        if self.h is not None:
            h, self.h = self.h, None
            if self.eng.h:                      # (an engine closed first took its device with it)
                self.eng._chk(self.eng.L.vv_gallery_destroy(self.eng.h, h))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


SOLVER_TYPES = {"SGD": 0, "NESTEROV": 1, "ADAGRAD": 2, "RMSPROP": 3, "ADAM": 5}     # (4, BVLC's ADADELTA: not implemented)


def _dev_ptr(x):
    """A DevBuf, a ctypes pointer or an integer device address as a c_void_p (None stays None)."""
    if x is None:
        return None
    if isinstance(x, DevBuf):
        return x.ptr
    return C.c_void_p(int(x.value if isinstance(x, C.c_void_p) else x))


def _rows_chk(rc):
    if rc != 0:
        raise VVError(load_library().vv_last_error().decode(), rc)


def rows_shuffled(seed, n, epochs=1):
    """vv_rows_shuffled: int32 [epochs * n], `epochs` permutations of 0 .. n - 1 one after the other, from one splitmix64 stream seeded
    with `seed` (videovector_amd/csrc/vv_rows.h states the rule).  The list Linear.fit(shuffle_seed=, epochs=) trains on."""
    out = np.zeros(max(int(n), 0) * max(int(epochs), 0), np.int32)
    _rows_chk(load_library().vv_rows_shuffled(int(seed) & 0xFFFFFFFFFFFFFFFF, int(n), int(epochs), _ptr(out)))
    return out


def rows_fold(seed, n, folds, fold):
    """vv_rows_fold: (train, held) int32 row lists of fold `fold` of `folds` over one shuffled epoch of `seed`; not stratified."""
    train, held = np.zeros(max(int(n), 1), np.int32), np.zeros(max(int(n), 1), np.int32)
    nt, nh = C.c_int64(), C.c_int64()
    _rows_chk(load_library().vv_rows_fold(int(seed) & 0xFFFFFFFFFFFFFFFF, int(n), int(folds), int(fold), _ptr(train), C.byref(nt), _ptr(held), C.byref(nh)))
    return train[:nt.value].copy(), held[:nh.value].copy()


def _row_list(rows):
    r = np.ascontiguousarray(rows, dtype=np.int32).reshape(-1)
    return r, (_ptr(r) if r.size else None)


LIN_LOSS_SOFTMAX, LIN_LOSS_HINGE = 0, 1          # VV_LIN_LOSS_*
NORM_L1, NORM_L2 = 1, 2                          # VV_NORM_*
_LIN_LOSSES = {"softmax": LIN_LOSS_SOFTMAX, "hinge": LIN_LOSS_HINGE}
_NORMS = {"L1": NORM_L1, "L2": NORM_L2}
_NORM_NAMES = {NORM_L1: "L1", NORM_L2: "L2"}


def cv_mean(v):
    """The mean cross_validate reports: the float32 sum in fold order over float32(folds)."""
    s = np.float32(0)
    for x in np.asarray(v, np.float32):
        s = np.float32(s + x)
    return np.float32(s / np.float32(len(v)))


def cv_best(results):
    """The weight decay cross_validate chooses: the largest mean_ap_mean, and of equal ones the smallest decay."""
    top = max(r["mean_ap_mean"] for r in results)
    return min(r["weight_decay"] for r in results if r["mean_ap_mean"] == top)


class Linear:
    """A linear classifier held on the device by an Engine (vv_linear_*): the reference's INNER_PRODUCT layer under SOFTMAX_LOSS or,
    after set_loss("hinge"), under HINGE_LOSS (one linear SVM per class), trained by SGD with momentum on a Gallery's embeddings."""

    def __init__(self, eng, handle, dim, num_classes, bias):
        self.eng, self.h, self.dim, self.num_classes, self.bias = eng, handle, int(dim), int(num_classes), bool(bias)

    def _labels(self, gallery, labels):
        lab = np.ascontiguousarray(labels, dtype=np.int32).reshape(-1)
        if lab.shape[0] != gallery.n_ref:
            raise VVError("labels must be [n_ref]")
        return lab

    @property
    def loss(self):
        """vv_linear_loss_get: ("softmax", None) or ("hinge", "L1" | "L2") -- the loss fit and grad run."""
        loss, norm = C.c_int32(), C.c_int32()
        self.eng._chk(self.eng.L.vv_linear_loss_get(self.eng.h, self.h, C.byref(loss), C.byref(norm)))
        return ("hinge", _NORM_NAMES[norm.value]) if loss.value == LIN_LOSS_HINGE else ("softmax", None)

    def set_loss(self, loss, norm="L2"):
        """vv_linear_loss_set: "softmax" or "hinge" (a linear SVM per class: the reference's HINGE_LOSS, norm "L1" or "L2"); sticky on
        the object, and neither parameters, histories, step counter nor cursor move.  Integers pass through as they are."""
        code = _LIN_LOSSES.get(loss, loss)
        nrm = _NORMS.get(norm, norm)
        if not isinstance(code, int) or not isinstance(nrm, int):
            raise VVError("set_loss: loss is 'softmax' or 'hinge', norm 'L1' or 'L2'")
        self.eng._chk(self.eng.L.vv_linear_loss_set(self.eng.h, self.h, code, nrm))

    def fit(self, gallery, labels, iters=100, batch=0, lr=0.1, momentum=0.9, weight_decay=0.0, loss_weight=1.0, lr_schedule=None,
            loss=None, norm=None, rows=None, epochs=None, shuffle_seed=None):
        """vv_linear_fit: `iters` steps on the gallery's items; returns (loss_trace fp32 [iters], report dict).  lr_schedule: [iters]
        learning rates that replace lr step by step.  loss / norm: set_loss first (it stays set).
        rows: vv_linear_fit_rows -- the steps take their batches from this list of gallery items (any order, repeats allowed) from its
        position 0, wrapping behind its last entry; labels stay [n_ref], by item; the object's cursor does not move.
        shuffle_seed with epochs: the list is rows_shuffled(shuffle_seed, n_ref, epochs).  rows and shuffle_seed together: ValueError."""
        if rows is not None and shuffle_seed is not None:
            raise ValueError("fit: give rows or shuffle_seed, not both")
        if (shuffle_seed is None) != (epochs is None):
            raise ValueError("fit: shuffle_seed and epochs go together")
        if shuffle_seed is not None:
            rows = rows_shuffled(shuffle_seed, gallery.n_ref, epochs)
        if loss is not None:
            self.set_loss(loss, "L2" if norm is None else norm)
        lab = self._labels(gallery, labels)
        cfg = _LinearCfg(int(iters), int(batch), lr, momentum, weight_decay, loss_weight)
        sched = None if lr_schedule is None else np.ascontiguousarray(lr_schedule, dtype=np.float32)
        if sched is not None and sched.shape != (int(iters),):
            raise VVError("lr_schedule must be [iters]")
        trace = np.zeros(max(int(iters), 0), np.float32)
        rep = _LinearReport()
        if rows is not None:
            r, rp = _row_list(rows)
            self.eng._chk(self.eng.L.vv_linear_fit_rows(self.eng.h, self.h, gallery.h, _ptr(lab), rp, r.size, C.byref(cfg), _ptr(sched), _ptr(trace),
                                                        C.byref(rep)))
        else:
            self.eng._chk(self.eng.L.vv_linear_fit(self.eng.h, self.h, gallery.h, _ptr(lab), C.byref(cfg), _ptr(sched), _ptr(trace), C.byref(rep)))
        return trace, dict(loss_first=np.float32(rep.loss_first), loss_last=np.float32(rep.loss_last),
                           accuracy_last=np.float32(rep.accuracy_last), steps=int(rep.steps), nonfinite_rows=int(rep.nonfinite_rows))

    def grad(self, gallery, labels, first=0, count=None, loss_weight=1.0, rows=None):
        """vv_linear_grad: (dW [C][dim], db [C], loss) of the batch [first, first + count) at the current parameters; nothing moves.
        rows: vv_linear_grad_rows -- the batch is this list of gallery items instead (first / count are not read)."""
        lab = self._labels(gallery, labels)
        count = gallery.n_ref - int(first) if count is None else int(count)
        dW, db = np.zeros((self.num_classes, self.dim), np.float32), np.zeros(self.num_classes, np.float32)
        loss = C.c_float()
        if rows is not None:
            r, rp = _row_list(rows)
            self.eng._chk(self.eng.L.vv_linear_grad_rows(self.eng.h, self.h, gallery.h, _ptr(lab), rp, r.size, loss_weight, _ptr(dW), _ptr(db),
                                                         C.byref(loss)))
            return dW, db, np.float32(loss.value)
        self.eng._chk(self.eng.L.vv_linear_grad(self.eng.h, self.h, gallery.h, _ptr(lab), int(first), count, loss_weight, _ptr(dW), _ptr(db),
                                                C.byref(loss)))
        return dW, db, np.float32(loss.value)

    def scores(self, src, out=None, rows=None):
        """vv_linear_scores: the logits [n][C] of a Gallery's device rows or of a host array [n][dim], as a DevBuf (`out`, or a new one):
        what Engine.classification_stats reads on the device.  rows (src a Gallery): vv_linear_scores_rows -- row i of the result is
        the logits of item rows[i]."""
        if rows is not None:
            if not isinstance(src, Gallery):
                raise VVError("scores: rows select items of a Gallery")
            r, rp = _row_list(rows)
            out = DevBuf(self.eng, (max(r.size, 1), self.num_classes)) if out is None else out
            self.eng._chk(self.eng.L.vv_linear_scores_rows(self.eng.h, self.h, src.h, rp, r.size, _dev_ptr(out)))
            return out
        if isinstance(src, Gallery):
            n, gh, q = src.n_ref, src.h, None
        else:
            q = np.ascontiguousarray(src, dtype=np.float32)
            if q.ndim != 2 or q.shape[1] != self.dim:
                raise VVError("scores: the rows must be [n][%d]" % self.dim)
            n, gh = q.shape[0], None
        out = DevBuf(self.eng, (n, self.num_classes)) if out is None else out
        self.eng._chk(self.eng.L.vv_linear_scores(self.eng.h, self.h, gh, _ptr(q), n, _dev_ptr(out)))
        return out

    def get(self):
        """(W [C][dim], b [C], hW, hb, steps)"""
        W, hW = (np.zeros((self.num_classes, self.dim), np.float32) for _ in range(2))
        b, hb = (np.zeros(self.num_classes, np.float32) for _ in range(2))
        steps = C.c_int64()
        self.eng._chk(self.eng.L.vv_linear_get(self.eng.h, self.h, _ptr(W), _ptr(b), _ptr(hW), _ptr(hb), C.byref(steps)))
        return W, b, hW, hb, steps.value

    def put(self, W=None, b=None, hW=None, hb=None, steps=0):
        """vv_linear_put: None leaves that array as it is; the batch cursor returns to 0."""
        def arr(a, shape):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=np.float32)
            if a.shape != shape:
                raise VVError("put: an array of shape %r is expected" % (shape,))
            return a
        ws, bs = (self.num_classes, self.dim), (self.num_classes,)
        W, hW, b, hb = arr(W, ws), arr(hW, ws), arr(b, bs), arr(hb, bs)
        self.eng._chk(self.eng.L.vv_linear_put(self.eng.h, self.h, _ptr(W), _ptr(b), _ptr(hW), _ptr(hb), int(steps)))

    def cross_validate(self, gallery, labels, folds, weight_decays, seed=0, **fit_kw):
        """k-fold cross-validation of the weight decay (the SVM's C) on the device.  For every weight decay, in the order given, and every
        fold f of rows_fold(seed, n_ref, folds, f): put zeros with counter 0; fit(rows=train_f, weight_decay=wd, **fit_kw);
        scores(gallery, rows=held_f) into one device buffer; Engine.classification_stats on it with labels[held_f], the scores read on
        the device -- nothing of size n x C crosses to the host.  Returns dict(results=[dict(weight_decay, mean_ap [folds],
        total_accuracy [folds], mean_ap_mean, total_accuracy_mean)], best=the weight decay with the largest mean_ap_mean, a tie going to
        the smaller decay).  The means are float32 sums in fold order over float32(folds).  Folds are not stratified.
        The classifier is LEFT HOLDING THE LAST FIT (the last weight decay's last fold): train on all items with `best` afterwards."""
        lab = self._labels(gallery, labels)
        n, folds = gallery.n_ref, int(folds)
        parts = [rows_fold(seed, n, folds, f) for f in range(folds)]
        buf = DevBuf(self.eng, (max(h.size for _, h in parts), self.num_classes))
        zW, zb = np.zeros((self.num_classes, self.dim), np.float32), np.zeros(self.num_classes, np.float32)
        results = []
        for wd in weight_decays:
            ap, acc = np.zeros(folds, np.float32), np.zeros(folds, np.float32)
            for f, (train, held) in enumerate(parts):
                self.put(W=zW, b=zb, hW=zW, hb=zb, steps=0)
                self.fit(gallery, lab, rows=train, weight_decay=wd, **fit_kw)
                self.scores(gallery, out=buf, rows=held)
                rep = self.eng.classification_stats(buf, lab[held], self.num_classes)[3]
                ap[f], acc[f] = rep["mean_ap"], rep["total_accuracy"]
            results.append(dict(weight_decay=wd, mean_ap=ap, total_accuracy=acc, mean_ap_mean=cv_mean(ap), total_accuracy_mean=cv_mean(acc)))
        buf.free()
        return dict(results=results, best=cv_best(results))

    def close(self):
        if self.h is not None and getattr(self.eng, "h", None):
            self.eng.L.vv_linear_destroy(self.eng.h, self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class StepConfig:
    """vv_step_cfg with the shipped project defaults (vv_step_cfg_default).  momentum2 (Adam's beta2) and rms_decay have no field in the
    struct: given here, the Engine forwards them through vv_solver_ext_set in front of every call that takes this configuration (the one
    not given keeps the context's value).  clip_gradients (BVLC SolverParameter.clip_gradients; vv_clip_gradients_set) is forwarded the
    same way: None keeps the context's threshold, a negative value disables clipping."""

    def __init__(self, B, C_, Nn, **kw):
        self.momentum2 = self.rms_decay = self.clip_gradients = None
        self.c = _StepCfg()
        load_library().vv_step_cfg_default(C.byref(self.c))
        self.c.B, self.c.C, self.c.Nn = B, C_, Nn
        self._keep = {}
        for k, v in kw.items():
            self.set(k, v)

    def set(self, k, v):
        if k == "ctx_coeff":
            a = None if v is None else np.ascontiguousarray(v, dtype=np.float32)
            self._keep[k] = a
            self.c.ctx_coeff = None if a is None else a.ctypes.data
        elif k == "dropout_mask":
            a = None if v is None else np.ascontiguousarray(v, dtype=np.uint8)
            self._keep[k] = a
            self.c.dropout_mask = None if a is None else a.ctypes.data
        elif k == "item_weight":
            a = None if v is None else np.ascontiguousarray(v, dtype=np.float32)
            self._keep[k] = a
            self.c.item_weight = None if a is None else a.ctypes.data
        elif k in ("lr_mult", "decay_mult"):
            getattr(self.c, k)[0], getattr(self.c, k)[1] = float(v[0]), float(v[1])
        elif k == "reg":
            self.c.reg = {"L1": 1, "L2": 2}.get(v, v)
        elif k == "solver_type":
            self.c.solver_type = SOLVER_TYPES.get(v, v)
        elif k in ("momentum2", "rms_decay", "clip_gradients"):
            setattr(self, k, None if v is None else float(v))
        elif k == "norm":
            self.c.norm = {"L1": 1, "L2": 2}.get(v, v)
        else:
            if not hasattr(self.c, k):
                raise AttributeError(k)
            setattr(self.c, k, v)
        return self


class Engine:
    """One context per process / GPU (vv_create)."""

    def __init__(self, device=0, prec="f16"):
        self.L = load_library()
        self.h = C.c_void_p()
        self.prec = prec
        self._chk(self.L.vv_create(device, PREC[prec], C.byref(self.h)))
        self.F = self.D = 0
        self.n_rows = 0
        self._ext_sent = None                      # the (momentum2, rms_decay) of a StepConfig last forwarded by _ext
        self._clip_sent = None                     # ... and its clip_gradients

    def _chk(self, rc):
        if rc != 0:
            raise VVError("videovec error %d: %s" % (rc, self.L.vv_last_error().decode()), rc)

    # ---- the step's carried state (vv_run_state_*): a run that resumes bit for bit
    def run_state(self):
        """What a training step reads that earlier steps left and no other getter returns (the dropout counter, the lagging 16-bit
        scales and the copy of W rounded at them, the report rings ...), as opaque bytes.  Synchronises."""
        n = C.c_int64()
        self._chk(self.L.vv_run_state_size(self.h, C.byref(n)))
        buf = C.create_string_buffer(n.value)
        w = C.c_int64()
        self._chk(self.L.vv_run_state_get(self.h, buf, n.value, C.byref(w)))
        return buf.raw[:w.value]

    def set_run_state(self, blob):
        """After params_set, history2_set and solver_iter (params_set resets part of this state)."""
        blob = bytes(blob)
        self._chk(self.L.vv_run_state_put(self.h, C.create_string_buffer(blob, len(blob)) if blob else None, len(blob)))

    def close(self):
        if getattr(self, "h", None) and self.h:
            self.L.vv_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- setup
    def set_stream(self, raw_stream):
        self._chk(self.L.vv_set_stream(self.h, C.c_void_p(raw_stream)))

    def synchronize(self):
        self._chk(self.L.vv_synchronize(self.h))

    def set_option(self, name, value):
        """Per-context execution switch by name (include/videovec.h: vv_set_option)."""
        self._chk(self.L.vv_set_option(self.h, name.encode(), float(value)))

    def get_option(self, name):
        v = C.c_double(0)
        self._chk(self.L.vv_get_option(self.h, name.encode(), C.byref(v)))
        return v.value

    def set_dedup(self, on):
        """Row de-duplication of the batch (include/videovec.h: vv_set_dedup); default on."""
        self._chk(self.L.vv_set_dedup(self.h, int(bool(on))))

    def dedup_stats(self):
        """(rows, distinct rows) of the last forward/backward pass."""
        r, u = C.c_int64(0), C.c_int64(0)
        self._chk(self.L.vv_dedup_stats(self.h, C.byref(r), C.byref(u)))
        return r.value, u.value

    def h16_stats(self):
        """Range loss of the f16 ip2 rows (include/videovec.h: vv_h16_stats; option "h16_guard"): a dict of saturated and
        faint_rows of the last completed step (synchronises), flagged_steps and first_flagged_step as the host has read them
        from the steps' reports (four steps late), fallback and rows_f16."""
        r = _H16Report()
        self._chk(self.L.vv_h16_stats(self.h, C.byref(r)))
        return {k: int(getattr(r, k)) for k, _ in _H16Report._fields_}

    def grad_scale_stats(self):
        """(steps whose 16-bit gradients had to be produced again at a smaller scale, current scale); videovec.h."""
        r, sc = C.c_int64(0), C.c_float(0)
        self._chk(self.L.vv_grad_scale_stats(self.h, C.byref(r), C.byref(sc)))
        return r.value, sc.value

    def table_set(self, rows):
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        self.n_rows, self.F = rows.shape
        self._chk(self.L.vv_table_set(self.h, _ptr(rows), rows.shape[0], rows.shape[1]))

    def table_synth(self, seed, n_rows, F):
        self.n_rows, self.F = n_rows, F
        self._chk(self.L.vv_table_synth(self.h, seed, n_rows, F))

    def table_get(self, rows=None, n=None):
        r = None if rows is None else np.ascontiguousarray(rows, dtype=np.int32)
        n = len(r) if r is not None else n
        out = np.empty((n, self.F), np.float32)
        self._chk(self.L.vv_table_get(self.h, _ptr(r), n, _ptr(out)))
        return out

    def params_set(self, W, b=None, hW=None, hb=None):
        W = np.ascontiguousarray(W, dtype=np.float32)
        self.D = W.shape[0]
        assert W.shape[1] == self.F, "W must be D x F with the table's F"
        cv = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float32)
        b, hW, hb = cv(b), cv(hW), cv(hb)
        self._chk(self.L.vv_params_set(self.h, self.D, _ptr(W), _ptr(b), _ptr(hW), _ptr(hb)))

    def params_get(self):
        W = np.empty((self.D, self.F), np.float32); b = np.empty(self.D, np.float32)
        hW = np.empty_like(W); hb = np.empty_like(b)
        self._chk(self.L.vv_params_get(self.h, _ptr(W), _ptr(b), _ptr(hW), _ptr(hb)))
        return W, b, hW, hb

    # ---- RMSProp / Adam (vv_solver_ext_*, vv_solver_iter_*, vv_history2_*)
    def solver_ext_set(self, momentum2, rms_decay):
        self._ext_sent = None
        self._chk(self.L.vv_solver_ext_set(self.h, float(momentum2), float(rms_decay)))

    def solver_ext_get(self):
        """(momentum2, rms_decay) of the context."""
        m, r = C.c_float(), C.c_float()
        self._chk(self.L.vv_solver_ext_get(self.h, C.byref(m), C.byref(r)))
        return m.value, r.value

    @property
    def solver_iter(self):
        """Adam updates applied so far (the next one is t = solver_iter + 1)."""
        t = C.c_int64()
        self._chk(self.L.vv_solver_iter_get(self.h, C.byref(t)))
        return t.value

    @solver_iter.setter
    def solver_iter(self, t):
        self._chk(self.L.vv_solver_iter_set(self.h, int(t)))

    def history2_set(self, vW=None, vb=None):
        cv = lambda a, shape: None if a is None else np.ascontiguousarray(a, dtype=np.float32).reshape(shape)
        vW, vb = cv(vW, (self.D, self.F)), cv(vb, (self.D,))
        self._chk(self.L.vv_history2_set(self.h, _ptr(vW), _ptr(vb)))

    def history2_get(self):
        vW = np.empty((self.D, self.F), np.float32); vb = np.empty(self.D, np.float32)
        self._chk(self.L.vv_history2_get(self.h, _ptr(vW), _ptr(vb)))
        return vW, vb

    # ---- gradient clipping by the global L2 norm (vv_clip_gradients_*, vv_clip_stats)
    def clip_gradients_set(self, clip):
        """clip < 0 disables, clip >= 0 is the threshold of the gradient's L2 norm (BVLC SGDSolver::ClipGradients)."""
        self._clip_sent = None
        self._chk(self.L.vv_clip_gradients_set(self.h, float(clip)))

    def clip_gradients_get(self):
        v = C.c_float()
        self._chk(self.L.vv_clip_gradients_get(self.h, C.byref(v)))
        return v.value

    def clip_stats(self):
        """norm / scale / clipped of the last completed clipping update (synchronises) and the updates / clipped_updates totals."""
        r = _ClipReport()
        self._chk(self.L.vv_clip_stats(self.h, C.byref(r)))
        return {"norm": np.float32(r.norm), "scale": np.float32(r.scale), "clipped": int(r.clipped), "updates": int(r.updates),
                "clipped_updates": int(r.clipped_updates)}

    # ---- gradient accumulation (BVLC SolverParameter.iter_size; vv_grads_bank, vv_grads_bank_reset, vv_accum_stats)
    def grads_bank(self):
        """Add the last forward_backward's gradient (and its loss and violations) into the bank; the next apply_update consumes the bank:
        the sum, clipped where clipping is active, times 1 / m, through the plain update."""
        self._chk(self.L.vv_grads_bank(self.h))

    def grads_bank_reset(self):
        """Discard the banked gradients (BVLC Net::ClearParamDiffs)."""
        self._chk(self.L.vv_grads_bank_reset(self.h))

    def accum_stats(self):
        """banked now; count / mean loss / mean violations of the last completed accumulated update (synchronises); their total."""
        r = _AccumReport()
        self._chk(self.L.vv_accum_stats(self.h, C.byref(r)))
        return {"banked": int(r.banked), "last_count": int(r.last_count), "last_mean_loss": np.float32(r.last_mean_loss),
                "last_mean_violations": np.float32(r.last_mean_violations), "updates": int(r.updates)}

    # ---- magnitude statistics (the reference's debug_info, net.cpp:580-636; vv_op_asum, vv_debug_stats_*, vv_debug_mark_update)
    @staticmethod
    def _abs_stat(r):
        return (float(r.asum), np.float32(r.amax), int(r.count), int(r.nonfinite))

    def op_asum(self, buf, n=None, offset=0):
        """(asum, amax, count, nonfinite) of n fp32 elements of a DevBuf (or a device pointer), `offset` floats into it; synchronises."""
        ptr = buf.ptr.value if isinstance(buf, DevBuf) else int(buf.value if isinstance(buf, C.c_void_p) else buf)
        if n is None:
            n = int(np.prod(buf.shape)) - offset
        r = _AbsStat()
        self._chk(self.L.vv_op_asum(self.h, C.c_void_p(ptr + 4 * int(offset)), int(n), C.byref(r)))
        return self._abs_stat(r)

    def debug_stats_queue(self, names):
        """Queue one measurement of the named tensors (STAT_NAMES; a single name or an iterable) as they are at this point of the stream."""
        mask = 0
        for name in ([names] if isinstance(names, str) else names):
            if name not in STAT_NAMES:
                raise VVError("debug_stats_queue: unknown entry %r (one of %s)" % (name, ", ".join(STAT_NAMES)))
            mask |= 1 << STAT_NAMES.index(name)
        self._chk(self.L.vv_debug_stats_queue(self.h, mask))

    def debug_mark_update(self):
        """Copy W and b into the shadow buffer: UPD_W / UPD_B queued after the next apply_update measure what it subtracted."""
        self._chk(self.L.vv_debug_mark_update(self.h))

    def debug_stats(self):
        """name -> (asum, amax, count, nonfinite) of every entry as its last queued measurement left it (synchronises); never queued: zeros."""
        arr = (_AbsStat * len(STAT_NAMES))()
        self._chk(self.L.vv_debug_stats_get(self.h, arr))
        return {name: self._abs_stat(arr[i]) for i, name in enumerate(STAT_NAMES)}

    # ---- the exponential moving average of the parameters (vv_ema_*; this project's own)
    def ema_set(self, decay):
        """decay < 0 turns the average off, 0 <= decay < 1 turns it on (started from the current W and b) or, while on, changes the decay."""
        self._chk(self.L.vv_ema_set(self.h, float(decay)))

    def ema_get(self):
        """(eW [D][F], eb [D]): the average as host fp32 (synchronises)."""
        W = np.empty((self.D, self.F), np.float32); b = np.empty(self.D, np.float32)
        self._chk(self.L.vv_ema_get(self.h, _ptr(W), _ptr(b)))
        return W, b

    def ema_put(self, W=None, b=None):
        """Replace the average by host values (a resumed run); None leaves that part."""
        cv = lambda a, shape: None if a is None else np.ascontiguousarray(a, dtype=np.float32).reshape(shape)
        W, b = cv(W, (self.D, self.F)), cv(b, (self.D,))
        self._chk(self.L.vv_ema_put(self.h, _ptr(W), _ptr(b)))

    def ema_use(self, on=True):
        """While on, forward / embed / embed_mean / gallery_from_table read the averaged parameters and everything that trains refuses."""
        self._chk(self.L.vv_ema_use(self.h, int(bool(on))))

    def ema_stats(self):
        """updates (k_ema launches since the activation), decay, in_use."""
        r = _EmaReport()
        self._chk(self.L.vv_ema_stats(self.h, C.byref(r)))
        return {"updates": int(r.updates), "decay": np.float32(r.decay), "in_use": bool(r.in_use)}

    @contextlib.contextmanager
    def ema(self):
        """with eng.ema(): ... -- ema_use(True) around the block, the training view again behind it."""
        self.ema_use(True)
        try:
            yield self
        finally:
            self.ema_use(False)

    def _ext(self, cfg):
        """StepConfig's momentum2 / rms_decay / clip_gradients -> the context, in front of a call that takes cfg."""
        if cfg.clip_gradients is not None and cfg.clip_gradients != self._clip_sent:
            self.clip_gradients_set(cfg.clip_gradients)
            self._clip_sent = cfg.clip_gradients
        if cfg.momentum2 is None and cfg.rms_decay is None:
            return
        want = (cfg.momentum2, cfg.rms_decay)
        if want == self._ext_sent:                 # (this engine already holds them: no call at all in a training loop)
            return
        m, r = self.solver_ext_get()
        self.solver_ext_set(m if cfg.momentum2 is None else cfg.momentum2, r if cfg.rms_decay is None else cfg.rms_decay)
        self._ext_sent = want

    # ---- iteration
    def forward_backward(self, cfg, idx=None, idx_dev_ptr=None, idx_ready=False):
        """idx: host array [B][C+Nn]; or idx_dev_ptr: device indices produced on the context's stream (ordered behind it),
        idx_ready=True when they are complete already (static batches: no ordering added)."""
        self._ext(cfg)
        if idx_dev_ptr is not None:
            self._chk(self.L.vv_forward_backward(self.h, C.byref(cfg.c), C.c_void_p(int(idx_dev_ptr)), 2 if idx_ready else 1))
        else:
            idx = np.ascontiguousarray(idx, dtype=np.int32)
            assert idx.shape == (cfg.c.B, cfg.c.C + cfg.c.Nn)
            self._chk(self.L.vv_forward_backward(self.h, C.byref(cfg.c), _ptr(idx), 0))

    # ---- the forward-only pass (Net::Forward under phase TEST; vv_forward, vv_eval_reset, vv_eval_stats)
    def forward(self, cfg, idx, on_device=0):
        """Held-out loss and violations with the current weights, no backward pass: nothing a training step owns is touched.
        idx: host array [B][C+Nn] (on_device=0), or a device pointer (1: produced on the context's stream, 2: complete already).
        The result accumulates in the record eval_stats() reads; loss() keeps returning the last TRAINING pass's values."""
        self._ext(cfg)
        if on_device:
            self._chk(self.L.vv_forward(self.h, C.byref(cfg.c), C.c_void_p(int(idx)), int(on_device)))
        else:
            idx = np.ascontiguousarray(idx, dtype=np.int32)
            assert idx.shape == (cfg.c.B, cfg.c.C + cfg.c.Nn)
            self._chk(self.L.vv_forward(self.h, C.byref(cfg.c), _ptr(idx), 0))

    def eval_reset(self):
        """Zero the evaluation record (queued behind the passes already issued)."""
        self._chk(self.L.vv_eval_reset(self.h))

    def eval_stats(self):
        """An EvalStats of the passes since eval_reset(): counts, double sums, the last pass's fp32 values, the means (synchronises)."""
        r = _EvalReport()
        self._chk(self.L.vv_eval_stats(self.h, C.byref(r)))
        return EvalStats(r)

    def forward_backward_q1(self, cfg, idx, last_src):
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        last_src = np.ascontiguousarray(last_src, dtype=np.int32)
        assert idx.shape == last_src.shape == (cfg.c.B, cfg.c.C + cfg.c.Nn)
        self._ext(cfg)
        self._chk(self.L.vv_forward_backward_q1(self.h, C.byref(cfg.c), _ptr(idx), _ptr(last_src)))

    def forward_backward_ring(self, cfg, ring, consumer=0, item_begin=0, label_out=None, timeout_s=60.0):
        """Next batch of the sampler's prefetch ring -> pinned staging -> async H2D -> forward/backward."""
        self._ext(cfg)
        self._chk(self.L.vv_forward_backward_ring(self.h, C.byref(cfg.c), ring.h, consumer, item_begin, _ptr(label_out),
                                                  float(timeout_s)))

    # ---- per-layer operators (vv_dev_* / vv_op_*): device buffers are DevBuf objects
    def dev(self, array_or_shape):
        """A device buffer: from a float32 / uint8 array (uploaded) or a shape (zeros, float32)."""
        return DevBuf(self, array_or_shape)

    def op(self, name, *args):
        """Call vv_op_<name>(ctx, ...); DevBuf arguments pass their device pointer."""
        conv = [a.ptr if isinstance(a, DevBuf) else (_ptr(a) if isinstance(a, np.ndarray) else a) for a in args]
        self._chk(getattr(self.L, "vv_op_" + name)(self.h, *conv))

    # ---- data parallel (vv_comm_*)
    def comm_init(self, world, rank, id_path, transport="rccl"):
        kinds = {"rccl": 0, "shm": 1, "peer": 2}
        if transport not in kinds:
            raise VVError("comm_init: unknown transport %r (rccl, shm, peer)" % (transport,))
        self._chk(self.L.vv_comm_init(self.h, world, rank, None if id_path is None else id_path.encode(), kinds[transport]))

    def comm_overlap(self, on=True):
        self._chk(self.L.vv_comm_overlap(self.h, int(bool(on))))

    def comm_schedule(self, name):
        """'sync', 'overlap' or 'sharded' (include/videovec.h: vv_comm_schedule)."""
        self._chk(self.L.vv_comm_schedule(self.h, {"sync": 0, "overlap": 1, "sharded": 2}[name]))

    def allreduce_grads(self):
        self._chk(self.L.vv_allreduce_grads(self.h))

    def comm_destroy(self):
        self._chk(self.L.vv_comm_destroy(self.h))

    def update_hint(self, cfg):
        """The next forward_backward* is followed by apply_update(cfg) and nothing reads the gradient in between (vv_update_hint)."""
        self._ext(cfg)
        self._chk(self.L.vv_update_hint(self.h, C.byref(cfg.c)))

    def apply_update(self, cfg):
        self._ext(cfg)
        self._chk(self.L.vv_apply_update(self.h, C.byref(cfg.c)))

    def step(self, cfg, idx=None, idx_dev_ptr=None):
        self.update_hint(cfg)                      # (what vv_step does: nothing reads the gradient between the two calls)
        self.forward_backward(cfg, idx, idx_dev_ptr)
        self.apply_update(cfg)

    def loss(self):
        l, v = C.c_float(), C.c_float()
        self._chk(self.L.vv_loss_get(self.h, C.byref(l), C.byref(v)))
        return l.value, v.value

    def grads_device(self):
        p, n = C.c_void_p(), C.c_int64()
        self._chk(self.L.vv_grads_device(self.h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def grads_bind(self, dev_ptr):
        self._chk(self.L.vv_grads_bind(self.h, C.c_void_p(dev_ptr)))

    def grads(self):
        dW = np.empty((self.D, self.F), np.float32); db = np.empty(self.D, np.float32)
        self._chk(self.L.vv_grads_get(self.h, _ptr(dW), _ptr(db)))
        return dW, db

    def blobs(self, cfg, ip2=True, scores=True, ip1_diff=False):
        B, CN, Nn = cfg.c.B, cfg.c.C + cfg.c.Nn, cfg.c.Nn
        out = {}
        a = np.empty((CN * B, self.D), np.float32) if ip2 else None
        st = np.empty((B, Nn), np.float32) if scores else None
        sn = np.empty((B, Nn), np.float32) if scores else None
        dy = np.empty((CN * B, self.D), np.float32) if ip1_diff else None
        self._chk(self.L.vv_blobs_get(self.h, _ptr(a), _ptr(st), _ptr(sn), _ptr(dy)))
        if ip2: out["ip2"] = a
        if scores: out["target_score"], out["negative_scores"] = st, sn
        if ip1_diff: out["ip1_diff"] = dy
        return out

    def dedup_groups(self, dyu=True):
        """The row grouping of the last de-duplicated pass (include/videovec.h: vv_dedup_groups_get) as a dict: R, Rp, U, rows,
        uniq_rows, map, ord, cnt, seg_start, pos, scale and (dyu=True) the per-slot 16-bit gradient sums dyu [Rp][D]."""
        R, U = self.dedup_stats()
        Rp = (R + 255) // 256 * 256
        i32 = lambda n: np.empty(n, np.int32)
        out = dict(R=R, Rp=Rp, U=U, rows=i32(Rp), uniq_rows=i32(Rp), map=i32(R), ord=i32(R), cnt=i32(Rp), seg_start=i32(U + 1), pos=i32(R))
        if dyu:
            out["dyu"] = np.empty((Rp, self.D), np.float32)
        sc = C.c_float(0)
        self._chk(self.L.vv_dedup_groups_get(self.h, *[_ptr(out[k]) for k in ("rows", "uniq_rows", "map", "ord", "cnt", "seg_start", "pos")],
                                             _ptr(out.get("dyu")), C.byref(sc)))
        out["scale"] = sc.value
        return out

    def embed(self, rows=None, n=None, relu=True, l2norm=False):
        r = None if rows is None else np.ascontiguousarray(rows, dtype=np.int32)
        n = len(r) if r is not None else n
        out = np.empty((n, self.D), np.float32)
        self._chk(self.L.vv_embed(self.h, _ptr(r), n, int(relu), int(l2norm), _ptr(out)))
        return out

    def embed_mean(self, rows, coeff=None, relu=True, l2norm=False):
        """TEST-branch embedding: fc7(+ReLU)(+normalise) of the weighted sum of k rows per sample."""
        r = np.ascontiguousarray(rows, dtype=np.int32)
        n, k = r.shape
        cf = None if coeff is None else np.ascontiguousarray(coeff, dtype=np.float32)
        out = np.empty((n, self.D), np.float32)
        self._chk(self.L.vv_embed_mean(self.h, _ptr(r), n, k, _ptr(cf), int(relu), int(l2norm), _ptr(out)))
        return out

    def retrieval_stats(self, feat, video_ids, id2class, exclude_same_video=True):
        """RetrievalStatsLayer forward: (mAP, hit@1, hit@5)."""
        feat = np.ascontiguousarray(feat, dtype=np.float32)
        vid = np.ascontiguousarray(video_ids, dtype=np.int32)
        mi = np.ascontiguousarray(list(id2class.keys()), dtype=np.int32)
        mc = np.ascontiguousarray(list(id2class.values()), dtype=np.int32)
        o = [C.c_float(), C.c_float(), C.c_float()]
        self._chk(self.L.vv_retrieval_stats(self.h, _ptr(feat), feat.shape[0], feat.shape[1], _ptr(vid), _ptr(mi),
                                            _ptr(mc), len(mi), int(exclude_same_video), *[C.byref(x) for x in o]))
        return tuple(x.value for x in o)

    def classification_stats(self, scores, labels, num_classes, n=None):
        """ClassificationStatsLayer on the device (vv_classification_stats): (accuracy fp32 [C], ap fp32 [C], count int32 [C], report)
        with report a dict(total_accuracy, mean_ap, classes_present, n).  scores: a numpy array [n][C] (host scores), or a DevBuf /
        device pointer of n x C floats (then n = len(labels) unless given); labels: [n] integers in 0 .. C - 1."""
        lab = np.ascontiguousarray(labels, dtype=np.int32).reshape(-1)
        Cn = int(num_classes)
        if isinstance(scores, np.ndarray):
            sc = np.ascontiguousarray(scores, dtype=np.float32)
            if sc.ndim != 2 or sc.shape[1] != Cn or sc.shape[0] != lab.shape[0]:
                raise VVError("classification_stats: scores must be [len(labels)][num_classes]")
            ptr, on_dev, rows = _ptr(sc), 0, sc.shape[0]
        else:
            ptr = scores.ptr if isinstance(scores, DevBuf) else C.c_void_p(int(scores.value if isinstance(scores, C.c_void_p) else scores))
            on_dev, rows = 1, lab.shape[0] if n is None else int(n)
            if rows != lab.shape[0]:
                raise VVError("classification_stats: labels must be [n]")
        acc, ap, cnt = np.zeros(max(Cn, 0), np.float32), np.zeros(max(Cn, 0), np.float32), np.zeros(max(Cn, 0), np.int32)
        rep = _ClassificationReport()
        self._chk(self.L.vv_classification_stats(self.h, ptr, rows, Cn, _ptr(lab), on_dev, _ptr(acc), _ptr(ap), _ptr(cnt), C.byref(rep)))
        return acc, ap, cnt, dict(total_accuracy=np.float32(rep.total_accuracy), mean_ap=np.float32(rep.mean_ap),
                                  classes_present=int(rep.classes_present), n=int(rep.n))

    def linear(self, dim, num_classes, bias=True):
        """A softmax linear classifier on the device, all zero (vv_linear_create)."""
        h = C.c_void_p()
        self._chk(self.L.vv_linear_create(self.h, int(dim), int(num_classes), int(bool(bias)), C.byref(h)))
        return Linear(self, h, dim, num_classes, bias)

    def op_softmax_loss(self, z, rows, cols, pitch, labels, loss_weight=1.0, prob=None, dz=None):
        """vv_op_softmax_loss on device logits z [rows][pitch] (DevBuf or device pointer); prob / dz: DevBufs [rows][pitch] or None.
        Returns (loss, correct)."""
        lab = np.ascontiguousarray(labels, dtype=np.int32).reshape(-1)
        if lab.shape[0] != int(rows):
            raise VVError("op_softmax_loss: labels must be [rows]")
        loss, correct = C.c_float(), C.c_int64()
        self._chk(self.L.vv_op_softmax_loss(self.h, _dev_ptr(z), int(rows), int(cols), int(pitch), _ptr(lab), loss_weight, _dev_ptr(prob),
                                            _dev_ptr(dz), C.byref(loss), C.byref(correct)))
        return np.float32(loss.value), int(correct.value)

    def op_hinge_loss(self, z, rows, cols, pitch, labels, norm, loss_weight=1.0, dz=None):
        """vv_op_hinge_loss on device logits z [rows][pitch] (DevBuf or device pointer); norm "L1" / "L2" (or VV_NORM_*); dz: a DevBuf
        [rows][pitch], a device pointer or None.  Returns (loss, correct)."""
        lab = np.ascontiguousarray(labels, dtype=np.int32).reshape(-1)
        if lab.shape[0] != int(rows):
            raise VVError("op_hinge_loss: labels must be [rows]")
        loss, correct = C.c_float(), C.c_int64()
        self._chk(self.L.vv_op_hinge_loss(self.h, _dev_ptr(z), int(rows), int(cols), int(pitch), _ptr(lab), int(_NORMS.get(norm, norm)),
                                          loss_weight, _dev_ptr(dz), C.byref(loss), C.byref(correct)))
        return np.float32(loss.value), int(correct.value)

    def op_gemm_tn(self, A, lda, B, ldb, k, m, n, out):
        """vv_op_gemm_tn: out [m][n] = A^T B for device A [k][lda >= m], B [k][ldb >= n] (DevBufs or device pointers)."""
        self._chk(self.L.vv_op_gemm_tn(self.h, _dev_ptr(A), int(lda), _dev_ptr(B), int(ldb), int(k), int(m), int(n), _dev_ptr(out)))

    def _index(self, who, cls, items, centroids, metric, assign, *codebooks):
        """Engine.ivf's and Engine.ivfpq's body: metric, centroids, (ivfpq) codebooks and assign checked in that order, then vv_<who>_create."""
        if isinstance(metric, str):                       # (an integer goes to the library as it is: VV_KMEANS_*)
            if metric not in KMEANS_METRICS:
                raise VVError("%s: metric must be one of %s" % (who, ", ".join(sorted(KMEANS_METRICS))))
            metric = KMEANS_METRICS[metric]
        cent = np.ascontiguousarray(centroids, dtype=np.float32)
        if cent.ndim != 2 or cent.shape[1] != items.dim:
            raise VVError("%s: centroids must be [num_clusters][%d]" % (who, items.dim))
        books = [self._codebooks(who, items, cb) for cb in codebooks]
        a = None
        if assign is not None:
            a = np.ascontiguousarray(assign, dtype=np.int32)
            if a.shape != (items.n_ref,):
                raise VVError("%s: assign must be [n_ref]" % who)
        h = C.c_void_p()
        more = [x for cb in books for x in (_ptr(cb), cb.shape[0], cb.shape[1])]
        self._chk(getattr(self.L, "vv_%s_create" % who)(self.h, items.h, _ptr(cent), cent.shape[0], int(metric), _ptr(a), *more, C.byref(h)))
        return cls(self, h)

    def ivf(self, items, centroids, metric="euclidean", assign=None):
        """An inverted-file index of the Gallery `items` (vv_ivf_create): centroids fp32 [C][dim], metric "euclidean" or "spherical" (the
        probe's key is k-means'), assign int32 [n_ref] -- the list of every item, taken as it is -- or None: the index assigns every
        item to its nearest centroid as Gallery.kmeans(iters=0) does."""
        return self._index("ivf", IVFIndex, items, centroids, metric, assign)

    def _codebooks(self, who, items, codebooks):
        cb = np.ascontiguousarray(codebooks, dtype=np.float32)
        if cb.ndim != 3 or cb.shape[0] < 1 or cb.shape[0] * cb.shape[2] != items.dim:
            raise VVError("%s: codebooks must be [M][ksub][dim / M] with M * (dim / M) = %d" % (who, items.dim))
        return cb

    def pq_train(self, items, M, ksub, iters=20, seed=0):
        """Product-quantisation codebooks of the Gallery `items` (vv_pq_train): (codebooks fp32 [M][ksub][dim / M], objective float64
        [M]) -- sub-space m's are Gallery(items[:, m dsub:(m + 1) dsub]).kmeans(ksub, iters, seed=seed + m)'s centroids and last objective."""
        M, ksub = int(M), int(ksub)
        dsub = items.dim // M if M > 0 and items.dim % M == 0 else 0
        shape = (max(M, 0), max(ksub, 0), dsub)
        cb = np.zeros(max(shape[0] * shape[1] * shape[2], 1), np.float32)     # (never empty: the library names the argument that is wrong)
        obj = np.zeros(max(M, 1), np.float64)
        self._chk(self.L.vv_pq_train(self.h, items.h, M, ksub, int(iters), int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(cb), _ptr(obj)))
        return cb[:shape[0] * shape[1] * shape[2]].reshape(shape).copy(), obj[:M].copy()

    def pq_encode(self, items, codebooks):
        """uint8 [n_ref][M], item order (vv_pq_encode): code m of an item is the codeword Gallery.kmeans(iters=0, init=codebooks[m])
        assigns its sub-vector to."""
        cb = self._codebooks("pq_encode", items, codebooks)
        out = np.zeros((items.n_ref, cb.shape[0]), np.uint8)
        self._chk(self.L.vv_pq_encode(self.h, items.h, _ptr(cb), cb.shape[0], cb.shape[1], _ptr(out)))
        return out

    def ivfpq(self, items, centroids, codebooks, metric="euclidean", assign=None):
        """An inverted-file index of product-quantised codes of the Gallery `items` (vv_ivfpq_create): centroids, metric and assign as
        Engine.ivf takes them, codebooks fp32 [M][ksub][dim / M] (pq_train's)."""
        return self._index("ivfpq", IVFPQIndex, items, centroids, metric, assign, codebooks)

    def gallery(self, feat, ids=None):
        """A fixed reference set on the device (vv_gallery_create): feat fp32 [n_ref][dim], ids [n_ref] or None (top-k only)."""
        feat = np.ascontiguousarray(feat, dtype=np.float32)
        if feat.ndim != 2:
            raise VVError("gallery: feat must be [n_ref][dim]")
        rid = None if ids is None else np.ascontiguousarray(ids, dtype=np.int32)
        if rid is not None and rid.shape != (feat.shape[0],):
            raise VVError("gallery: ids must be [n_ref]")
        h = C.c_void_p()
        self._chk(self.L.vv_gallery_create(self.h, _ptr(feat), feat.shape[0], feat.shape[1], _ptr(rid), C.byref(h)))
        return Gallery(self, h, rid)

    def gallery_from_table(self, rows, ids=None, coeff=None, relu=True, l2norm=True):
        """The same from table rows, embedded as embed_mean does ([n][k] rows; [n] rows and no coeff: as embed); the
        embeddings never leave the device."""
        r = np.ascontiguousarray(rows, dtype=np.int32)
        if r.ndim == 1:
            r = r.reshape(-1, 1)
        n, k = r.shape
        cf = None if coeff is None else np.ascontiguousarray(coeff, dtype=np.float32)
        rid = None if ids is None else np.ascontiguousarray(ids, dtype=np.int32)
        if rid is not None and rid.shape != (n,):
            raise VVError("gallery_from_table: ids must be [n]")
        h = C.c_void_p()
        self._chk(self.L.vv_gallery_from_table(self.h, _ptr(r), n, k, _ptr(cf), int(relu), int(l2norm), _ptr(rid), C.byref(h)))
        return Gallery(self, h, rid)

    # ---- profiling
    def profile_enable(self, on=True):
        self._chk(self.L.vv_profile_enable(self.h, int(on)))

    def profile_select(self, kernels=None):
        """Time only these kernels (iterable of names); None = all."""
        self._chk(self.L.vv_profile_select(self.h, ",".join(kernels).encode() if kernels else None))

    def profile_get(self, kernel):
        ms, n = C.c_double(), C.c_int64()
        self._chk(self.L.vv_profile_get(self.h, kernel.encode(), C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def box_probe(self):
        """vv_box_probe: what this device delivers right now on two fixed probes (the benchmark's forward GEMM instantiation on contiguous
        random rows; a 1 GiB streaming copy) -- the calibration record of a bench line."""
        r = _BoxProbe()
        self._chk(self.L.vv_box_probe(self.h, C.byref(r)))
        return {"gemm_tflops": r.gemm_tflops, "gemm_ms": r.gemm_ms, "gemm_clock_mhz": r.gemm_clock_mhz,
                "copy_tbs": r.copy_tbs, "copy_ms": r.copy_ms,
                "gemm_shape": [r.gemm_rows, r.gemm_k, r.gemm_n], "gemm_launches": r.gemm_launches, "copy_bytes": r.copy_bytes}


class DevBuf:
    """Device memory of an Engine's context (vv_dev_alloc): the GPU side of a Blob."""

    def __init__(self, eng, array_or_shape):
        self.eng = eng
        if isinstance(array_or_shape, np.ndarray):
            a = np.ascontiguousarray(array_or_shape)
            self.shape, self.dtype = a.shape, a.dtype
        else:
            a = None
            self.shape, self.dtype = tuple(np.atleast_1d(array_or_shape)), np.dtype(np.float32)
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        p = C.c_void_p()
        eng._chk(eng.L.vv_dev_alloc(eng.h, max(self.nbytes, 4), C.byref(p)))
        self.ptr = C.c_void_p(p.value)
        if a is not None and self.nbytes:
            eng._chk(eng.L.vv_dev_upload(eng.h, self.ptr, _ptr(a), self.nbytes))

    def get(self):
        out = np.empty(self.shape, self.dtype)
        if self.nbytes:
            self.eng._chk(self.eng.L.vv_dev_download(self.eng.h, _ptr(out), self.ptr, self.nbytes))
        return out

    def set(self, a):
        a = np.ascontiguousarray(a, dtype=self.dtype)
        assert a.shape == self.shape
        self.eng._chk(self.eng.L.vv_dev_upload(self.eng.h, self.ptr, _ptr(a), self.nbytes))

    def free(self):
        if self.ptr is not None and getattr(self.eng, "h", None):
            self.eng.L.vv_dev_free(self.eng.h, self.ptr)
        self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class _SamplerParam(C.Structure):
    _fields_ = [("batch_size", C.c_int32), ("context_size", C.c_int32),
                ("num_negative_samples", C.c_int32), ("max_buffer_size", C.c_int32),
                ("negative_swap_percentage", C.c_int32), ("max_same_video_negs", C.c_int32),
                ("max_tries_for_negs", C.c_int32), ("context_type", C.c_int32), ("initial_cursor", C.c_int32),
                ("output_shot_distance", C.c_int32), ("max_shot_distance", C.c_float), ("rand_seed", C.c_int32)]


CONTEXT_TYPES = {"WINDOW": 0, "PAST": 1, "PAST_CONTINUOUS": 2, "PAST_CONTINUOUS_FIXED": 3, "PAIRWISE": 4}


class Sampler:
    """Host-side triplet sampler of the product library (vv_sampler_*): the reference's
    VideoSampledShotsDataLayer with row indices instead of feature copies.  negatives = (video_id, n_shots,
    row_base[, shot_ids]) of a `negative_dataset` whose rows live in the same feature table."""

    def __init__(self, video_id, n_shots, row_base, *, batch_size, context_size,
                 num_negative_samples, max_buffer_size=5000, negative_swap_percentage=50,
                 max_same_video_negs=0, max_tries_for_negs=100, shot_ids=None, context_type="WINDOW", initial_cursor=0,
                 output_shot_distance=False, max_shot_distance=5.0, negatives=None, rand_seed=1):
        L = load_library()
        L.vv_sampler_create_neg.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.POINTER(C.c_void_p)]
        L.vv_sampler_next.argtypes = [C.c_void_p] * 4
        L.vv_sampler_destroy.argtypes = [C.c_void_p]
        L.vv_sampler_prefetch_start.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_char_p, C.c_int32]
        L.vv_sampler_prefetch_stop.argtypes = [C.c_void_p]
        L.vv_sampler_ring.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        self.L = L
        vid = np.ascontiguousarray(video_id, dtype=np.int32)
        ns = np.ascontiguousarray(n_shots, dtype=np.int32)
        rb = np.ascontiguousarray(row_base, dtype=np.int64)
        sid = None if shot_ids is None else np.ascontiguousarray(shot_ids, dtype=np.int32)
        p = _SamplerParam(batch_size, context_size, num_negative_samples, max_buffer_size,
                          negative_swap_percentage, max_same_video_negs, max_tries_for_negs,
                          CONTEXT_TYPES[context_type], initial_cursor, int(output_shot_distance), max_shot_distance, rand_seed)
        self.h = C.c_void_p()
        nvid = nns = nrb = nsid = None
        if negatives is not None:
            nvid = np.ascontiguousarray(negatives[0], dtype=np.int32)
            nns = np.ascontiguousarray(negatives[1], dtype=np.int32)
            nrb = np.ascontiguousarray(negatives[2], dtype=np.int64)
            nsid = np.ascontiguousarray(negatives[3], dtype=np.int32) if len(negatives) > 3 and negatives[3] is not None else None
        rc = L.vv_sampler_create_neg(C.byref(p), len(vid), _ptr(vid), _ptr(ns), _ptr(rb), _ptr(sid),
                                     0 if nvid is None else len(nvid), _ptr(nvid), _ptr(nns), _ptr(nrb), _ptr(nsid),
                                     C.byref(self.h))
        if rc != 0:
            raise VVError("vv_sampler_create failed (%d): the reference would CHECK-fail on these "
                          "parameters" % rc)
        if context_type == "PAIRWISE":
            context_size = 2
        self.B, self.CN = batch_size, context_size + num_negative_samples

    def next(self, want_last=False, want_label=False):
        idx = np.empty((self.B, self.CN), np.int32)
        last = np.empty((self.B, self.CN), np.int32) if want_last else None
        label = np.empty((self.B,), np.int32) if want_label else None
        rc = self.L.vv_sampler_next(self.h, _ptr(idx), _ptr(last), _ptr(label))
        if rc != 0:
            raise VVError("vv_sampler_next failed (%d)" % rc)
        if want_last or want_label:
            return idx, last, label
        return idx

    def state(self):
        """The state of the reference's one sequential stream after the last batch DELIVERED (by next(), or taken from the ring by its
        single consumer), as opaque bytes; with the pipeline running a private serial sampler is replayed to that position."""
        n = C.c_int64()
        rc = self.L.vv_sampler_state_size(self.h, C.byref(n))
        buf = C.create_string_buffer(max(n.value, 1))
        w = C.c_int64()
        rc = rc or self.L.vv_sampler_state_get(self.h, buf, n.value, C.byref(w))
        if rc != 0:
            raise VVError("vv_sampler_state_get failed (%d): %s" % (rc, self.L.vv_sampler_state_error().decode()), rc)
        return buf.raw[:w.value]

    def set_state(self, blob):
        """Only before prefetch_start() and the first next(); a blob of other parameters or another dataset is refused."""
        blob = bytes(blob)
        rc = self.L.vv_sampler_state_put(self.h, C.create_string_buffer(blob, max(len(blob), 1)), len(blob))
        if rc != 0:
            raise VVError("vv_sampler_state_put failed (%d): %s" % (rc, self.L.vv_sampler_state_error().decode()), rc)

    def prefetch_start(self, depth=4, threads=4, shm_name=None, consumers=1):
        """Background threads keep `depth` batches ahead (BasePrefetchingDataLayer, base_data_layer.cpp:52-95); next()
        then pops finished batches.  shm_name: publish the ring in POSIX shared memory for `consumers` processes
        (BatchRing.attach)."""
        rc = self.L.vv_sampler_prefetch_start(self.h, depth, threads, None if shm_name is None else shm_name.encode(), consumers)
        if rc != 0:
            raise VVError("vv_sampler_prefetch_start failed (%d)" % rc)

    def stat(self, which):
        self.L.vv_sampler_stat.argtypes = [C.c_void_p, C.c_int32]
        self.L.vv_sampler_stat.restype = C.c_int64
        return self.L.vv_sampler_stat(self.h, which)

    def prefetch_stop(self):
        self.L.vv_sampler_prefetch_stop(self.h)

    def ring(self):
        """The producer process's own consumer handle of the prefetch ring."""
        r = C.c_void_p()
        if self.L.vv_sampler_ring(self.h, C.byref(r)) != 0:
            raise VVError("vv_sampler_ring: prefetch is not running")
        return BatchRing(r, owned=False, keep=self)

    def close(self):
        if getattr(self, "h", None) and self.h:
            self.L.vv_sampler_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BatchRing:
    """A consumer's view of a sampler's prefetch ring (vv_batch_ring_*): one sampler per node, every data-parallel
    rank takes its items of the same global batch."""

    def __init__(self, handle, owned, keep=None):
        self.L = load_library()
        self.L.vv_batch_ring_info.argtypes = [C.c_void_p] + [C.POINTER(C.c_int32)] * 4
        self.L.vv_batch_ring_next.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_double]
        self.L.vv_batch_ring_detach.argtypes = [C.c_void_p]
        self.h, self.owned, self._keep = handle, owned, keep
        v = [C.c_int32() for _ in range(4)]
        self.L.vv_batch_ring_info(self.h, *[C.byref(x) for x in v])
        self.batch_size, self.CN, self.consumers, self.depth = [x.value for x in v]

    @classmethod
    def attach(cls, shm_name, timeout_s=60.0):
        L = load_library()
        L.vv_batch_ring_attach.argtypes = [C.c_char_p, C.c_double, C.POINTER(C.c_void_p)]
        h = C.c_void_p()
        rc = L.vv_batch_ring_attach(shm_name.encode(), float(timeout_s), C.byref(h))
        if rc != 0:
            raise VVError("vv_batch_ring_attach(%r) failed (%d)" % (shm_name, rc))
        return cls(h, owned=True)

    def next(self, consumer=0, item_begin=0, item_count=None, want_label=False, timeout_s=0.0, out=None):
        n = self.batch_size - item_begin if item_count is None else item_count
        idx = out if out is not None else np.empty((n, self.CN), np.int32)
        label = np.empty((n,), np.int32) if want_label else None
        rc = self.L.vv_batch_ring_next(self.h, consumer, item_begin, n, _ptr(idx), _ptr(label), float(timeout_s))
        if rc != 0:
            raise VVError("vv_batch_ring_next failed (%d): producer gone or timeout" % rc)
        return (idx, label) if want_label else idx

    def close(self):
        if self.owned and self.h:
            self.L.vv_batch_ring_detach(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
