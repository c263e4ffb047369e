"""ctypes binding of ``libxrl_amd.so`` -- the MI355X counterpart of ``pecos.core.clib`` for the
XR-Linear inference path.

Mirrors, for that path only, the reference's binding layer (pecos/core/base.py):

* struct views ``ScipyCsrF32 / ScipyCscF32 / ScipyDrmF32 / ScipyDcmF32``   base.py:172-354
* ``ScipyCompressedSparseAllocator`` (python-side result allocator)        base.py:357-478
* ``corelib`` methods ``xlinear_load_predict_only``, ``xlinear_destruct_model``,
  ``xlinear_get_int_attr``, ``xlinear_get_layer_type``, ``xlinear_predict``,
  ``xlinear_single_layer_predict``, ``xlinear_single_layer_train`` (with
  ``ScipyCoordinateSparseAllocator``), ``sparse_matmul``,
  ``sparse_inner_products``                                               base.py:978-1405, 1460-1589

with the same names, argument order and meaning, so that code written against
``pecos.core.clib`` reads the same against :data:`clib` here.  There is NO CPU fallback: every
compute call needs a visible HIP device and raises ``RuntimeError`` otherwise.
"""
import contextlib
import ctypes
import sys
import os
from ctypes import (CFUNCTYPE, POINTER, byref, c_bool, c_char_p, c_double, c_float, c_int, c_int32, c_int64,
                    c_uint32, c_uint64, c_void_p, cast)

import numpy as np
import scipy.sparse as smat

XLINEAR_INFERENCE_MODEL_TYPES = {"CSC": 0, "HASH_CHUNKED": 1, "BINARY_SEARCH_CHUNKED": 2}  # base.py:49

# PECOS_XRL_AMD_SO selects another build of the same library (kernel-tuning variants)
_LIB_PATH = os.environ.get("PECOS_XRL_AMD_SO") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libxrl_amd.so")


class ClusteringParam(ctypes.Structure):
    """struct ClusteringParam of include/xrl_abi.h (clustering.hpp:35-72); built from any object with these attributes, or from keywords."""
    _fields_ = [("partition_algo", c_uint64), ("seed", c_int), ("kmeans_max_iter", c_uint64), ("threads", c_int),
                ("max_sample_rate", c_float), ("min_sample_rate", c_float), ("warmup_ratio", c_float)]

    def __init__(self, params=None, **kw):
        super().__init__()
        for name, _ in self._fields_:
            setattr(self, name, kw[name] if name in kw else getattr(params, name))


TFIDF_TOKENIZER_CODES = {"word": 10, "char": 20, "char_wb": 30}  # tfidf.hpp:281-285


class TfidfBaseVectorizerParam(ctypes.Structure):
    """struct TfidfBaseVectorizerParam of include/xrl_abi.h (tfidf.hpp:66-116), filled from a config dict the way the reference's class
    of the same name is (base.py:53-126): ``norm`` / ``analyzer`` / ``truncate_length`` / ``ngram_range`` are aliases of ``norm_p`` /
    ``tok_type`` / ``max_length`` / (``min_ngram``, ``max_ngram``), and the dict is updated in place with the resolved names."""
    _fields_ = [("min_ngram", c_int32), ("max_ngram", c_int32), ("max_length", c_int32), ("max_feature", c_int32),
                ("min_df_ratio", c_float), ("max_df_ratio", c_float), ("min_df_cnt", c_int32), ("max_df_cnt", c_int32),
                ("binary", c_bool), ("use_idf", c_bool), ("smooth_idf", c_bool), ("add_one_idf", c_bool), ("sublinear_tf", c_bool),
                ("keep_frequent_feature", c_bool), ("norm_p", c_int32), ("tok_type", c_int32)]
    DEFAULTS = dict(min_ngram=1, max_ngram=1, max_length=-1, max_feature=0, min_df_ratio=0.0, max_df_ratio=1.0, min_df_cnt=0, max_df_cnt=-1,
                    binary=False, use_idf=True, smooth_idf=True, add_one_idf=False, sublinear_tf=False, keep_frequent_feature=True, norm_p=2,
                    tok_type=TFIDF_TOKENIZER_CODES["word"])

    def __init__(self, config_dict=None):
        super().__init__()
        cfg = {} if config_dict is None else config_dict

        def named(key, alias):
            return cfg.get(key, cfg.get(alias, self.DEFAULTS[key]))

        norm_p = named("norm_p", "norm")
        if isinstance(norm_p, str):                      # "l1" / "l2"
            norm_p = int(norm_p[1:])
        if norm_p not in (1, 2):
            raise NotImplementedError("norm_p only support 1 or 2")
        cfg["norm_p"] = norm_p
        tok_type = named("tok_type", "analyzer")
        cfg["tok_type"] = TFIDF_TOKENIZER_CODES[tok_type] if isinstance(tok_type, str) else tok_type
        cfg["max_length"] = named("max_length", "truncate_length")
        if "ngram_range" in cfg:
            cfg["min_ngram"], cfg["max_ngram"] = cfg["ngram_range"][0], cfg["ngram_range"][1]
        for name, _ in self._fields_:
            setattr(self, name, cfg.get(name, self.DEFAULTS[name]))


class TfidfVectorizerParam(ctypes.Structure):
    """struct TfidfVectorizerParam (tfidf.hpp:194-208): the base parameters side by side and the ensemble's norm."""
    _fields_ = [("base_param_ptr", POINTER(TfidfBaseVectorizerParam)), ("num_base_vect", c_int32), ("norm_p", c_int32)]

    def __init__(self, base_vect_param_list, norm_p):
        super().__init__()
        self.num_base_vect = len(base_vect_param_list)
        self._base = (TfidfBaseVectorizerParam * max(1, self.num_base_vect))(*base_vect_param_list)   # (kept alive with the struct)
        self.base_param_ptr = cast(self._base, POINTER(TfidfBaseVectorizerParam))
        self.norm_p = norm_p

    @classmethod
    def from_config(cls, config):
        """A single base config, or {"base_vect_configs": [...], "norm_p": ...} (base.py:1766-1778)."""
        if "base_vect_configs" not in config:
            bases = [TfidfBaseVectorizerParam(config)]
            return cls(bases, bases[0].norm_p)
        return cls([TfidfBaseVectorizerParam(c) for c in config["base_vect_configs"]], config["norm_p"])


class _MatView(ctypes.Structure):
    """Common behaviour of the zero-copy matrix views (the buffers are kept alive in py_buf)."""

    @classmethod
    def init_from(cls, A):
        if A is None:
            return None
        if isinstance(A, cls):
            return A
        return cls(A)

    @property
    def dtype(self):
        return self.buf.dtype

    @property
    def shape(self):
        return self.buf.shape


class ScipyCscF32(_MatView):
    _fields_ = [("rows", c_uint32), ("cols", c_uint32), ("col_ptr", POINTER(c_uint64)),
                ("row_idx", POINTER(c_uint32)), ("val", POINTER(c_float))]

    def __init__(self, A):
        assert isinstance(A, smat.csc_matrix)
        assert A.dtype == np.float32
        self.py_buf = {"col_ptr": A.indptr.astype(np.uint64, copy=False),
                       "row_idx": A.indices.astype(np.uint32, copy=False),
                       "val": A.data.astype(np.float32, copy=False)}
        self.rows, self.cols = A.shape
        for name, typ in self._fields_[2:]:
            setattr(self, name, self.py_buf[name].ctypes.data_as(typ))
        self.buf = A


class ScipyCsrF32(_MatView):
    _fields_ = [("rows", c_uint32), ("cols", c_uint32), ("row_ptr", POINTER(c_uint64)),
                ("col_idx", POINTER(c_uint32)), ("val", POINTER(c_float))]

    def __init__(self, A):
        assert isinstance(A, smat.csr_matrix)
        assert A.dtype == np.float32
        self.py_buf = {"row_ptr": A.indptr.astype(np.uint64, copy=False),
                       "col_idx": A.indices.astype(np.uint32, copy=False),
                       "val": A.data.astype(np.float32, copy=False)}
        self.rows, self.cols = A.shape
        for name, typ in self._fields_[2:]:
            setattr(self, name, self.py_buf[name].ctypes.data_as(typ))
        self.buf = A


class ScipyDrmF32(_MatView):
    _fields_ = [("rows", c_uint32), ("cols", c_uint32), ("val", POINTER(c_float))]

    def __init__(self, A):
        assert isinstance(A, np.ndarray)
        assert A.dtype == np.float32
        assert A.flags["C_CONTIGUOUS"] is True
        self.py_buf = {"val": A}
        self.rows, self.cols = A.shape
        self.val = A.ctypes.data_as(POINTER(c_float))
        self.buf = A


class ScipyDcmF32(_MatView):
    _fields_ = [("rows", c_uint32), ("cols", c_uint32), ("val", POINTER(c_float))]

    def __init__(self, A):
        assert isinstance(A, np.ndarray)
        assert A.dtype == np.float32
        assert A.flags["F_CONTIGUOUS"] is True
        self.py_buf = {"val": A}
        self.rows, self.cols = A.shape
        self.val = A.ctypes.data_as(POINTER(c_float))
        self.buf = A


class ScipyCompressedSparseAllocator(object):
    """Python-side allocator handed to the native predict call (base.py:357-478): the callee passes
    the addresses of its three pointers, we allocate numpy arrays and write their addresses back."""

    CFUNCTYPE = CFUNCTYPE(None, c_bool, c_uint64, c_uint64, c_uint64, c_void_p, c_void_p, c_void_p)

    def __init__(self, rows=0, cols=0, dtype=np.float32):
        assert dtype == np.float32
        self.rows, self.cols, self.dtype = rows, cols, dtype
        self.indices = self.indptr = self.data = None
        self.is_col_major = None

    def __call__(self, is_col_major, rows, cols, nnz, indices_ptr, indptr_ptr, data_ptr):
        self.rows, self.cols, self.is_col_major = rows, cols, is_col_major
        self.indptr = np.zeros((cols if is_col_major else rows) + 1, dtype=np.uint64)
        self.indices = np.zeros(nnz, dtype=np.uint32)
        self.data = np.zeros(nnz, dtype=self.dtype)
        for dst, arr in ((indices_ptr, self.indices), (indptr_ptr, self.indptr), (data_ptr, self.data)):
            cast(dst, POINTER(c_uint64)).contents.value = arr.ctypes.data_as(c_void_p).value or 0

    def get(self):
        if self.indptr is None:
            raise RuntimeError("native call did not produce a result")
        mat = smat.csc_matrix if self.is_col_major else smat.csr_matrix
        # int64 index arrays (scipy would otherwise up/down-cast unsigned ones); order is preserved
        return mat((self.data, self.indices.astype(np.int64), self.indptr.astype(np.int64)),
                   shape=(self.rows, self.cols))

    @property
    def cfunc(self):
        return self.CFUNCTYPE(self)


class ScipyCoordinateSparseAllocator(object):
    """Python-side allocator of a COO result (base.py:481-540): u64 row and column ids and float32 values, allocated when the native
    training call knows the count."""

    CFUNCTYPE = CFUNCTYPE(None, c_uint64, c_uint64, c_uint64, c_void_p, c_void_p, c_void_p)

    def __init__(self, rows=0, cols=0, dtype=np.float32):
        assert dtype == np.float32
        self.rows, self.cols, self.dtype = rows, cols, dtype
        self.row_ptr = self.col_ptr = self.data = None

    def __call__(self, rows, cols, nnz, row_ptr, col_ptr, val_ptr):
        self.rows, self.cols = rows, cols
        self.row_ptr, self.col_ptr, self.data = np.zeros(nnz, dtype=np.uint64), np.zeros(nnz, dtype=np.uint64), np.zeros(nnz, dtype=self.dtype)
        for dst, arr in ((row_ptr, self.row_ptr), (col_ptr, self.col_ptr), (val_ptr, self.data)):
            cast(dst, POINTER(c_uint64)).contents.value = arr.ctypes.data_as(c_void_p).value or 0

    def _coo(self):
        if self.data is None:
            raise RuntimeError("native call did not produce a result")
        return smat.coo_matrix((self.data, (self.row_ptr.astype(np.int64), self.col_ptr.astype(np.int64))), shape=(self.rows, self.cols))

    def tocsr(self):
        return self._coo().tocsr()

    def tocsc(self):
        return self._coo().tocsc()

    @property
    def cfunc(self):
        return self.CFUNCTYPE(self)


XLINEAR_SOLVERS = {"L2R_L2LOSS_SVC_DUAL": 1, "L2R_L1LOSS_SVC_DUAL": 3, "L2R_LR_DUAL": 7, "L2R_L2LOSS_SVC_PRIMAL": 2}  # base.py:42-47


class ProfileRec(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char * 32), ("layer", c_uint32), ("launches", c_uint32),
                ("ms", c_double), ("reserved", c_double)]


def _preload_torch_hip_runtime():
    """One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64 (same SONAME as /opt/rocm's).  If this library pulls in the
    system copy first and torch is imported LATER, torch finds "No HIP GPUs"; importing torch first avoided that,
    but nothing enforced the order.  When a torch installation is present and not imported yet, its copy of the runtime is loaded here
    (without importing torch), so that libxrl_amd.so binds to the runtime torch will use -- in either import order."""
    if "torch" in sys.modules:
        return
    try:
        import glob
        import importlib.util
        spec = importlib.util.find_spec("torch")
        for d in (spec.submodule_search_locations or []) if spec else []:
            for so in sorted(glob.glob(os.path.join(d, "lib", "libamdhip64.so*"))):
                ctypes.CDLL(so, mode=ctypes.RTLD_GLOBAL)
                return
    except Exception:
        pass                                     # fall back to the system runtime


class corelib(object):
    """The C-ABI library, loaded lazily (so that importing the package works on a CPU-only box)."""

    def __init__(self, so_path=_LIB_PATH):
        self.so_path = so_path
        self._lib = None

    # ------------------------------------------------------------------ loading / errors
    @property
    def clib_float32(self):
        if self._lib is None:
            if not os.path.exists(self.so_path):
                raise RuntimeError(
                    f"{self.so_path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                    "(hipcc --offload-arch=gfx950).  pecos_amd has no CPU fallback.")
            _preload_torch_hip_runtime()
            self._lib = ctypes.CDLL(self.so_path)
            self._link(self._lib)
        return self._lib

    _alloc_t = ScipyCompressedSparseAllocator.CFUNCTYPE
    _coo_alloc_t = ScipyCoordinateSparseAllocator.CFUNCTYPE
    # name -> (result type, argument types) of every function include/xrl_abi.h declares
    SIGNATURES = {
        "xrl_last_error": (c_char_p, []),
        "xrl_clear_error": (None, []),
        "xrl_version": (c_char_p, []),
        "xrl_device_count": (c_int, []),
        "xrl_set_device": (c_int, [c_int]),
        "c_xlinear_load_model_from_disk": (c_void_p, [c_char_p]),
        "c_xlinear_load_model_from_disk_ext": (c_void_p, [c_char_p, c_int]),
        "c_xlinear_load_mmap_model_from_disk": (c_void_p, [c_char_p, c_bool]),
        "c_xlinear_compile_mmap_model": (None, [c_char_p, c_char_p]),
        "c_xlinear_destruct_model": (None, [c_void_p]),
        "c_xlinear_get_int_attr": (c_uint32, [c_void_p, c_char_p]),
        "c_xlinear_get_layer_type": (c_int, [c_void_p, c_int]),
        "c_xlinear_predict_csr_f32": (None, [c_void_p, POINTER(ScipyCsrF32), c_uint32, c_char_p, c_uint32, c_int, _alloc_t]),
        "c_xlinear_predict_drm_f32": (None, [c_void_p, POINTER(ScipyDrmF32), c_uint32, c_char_p, c_uint32, c_int, _alloc_t]),
        "c_xlinear_predict_on_selected_outputs_csr_f32": (None, [c_void_p, POINTER(ScipyCsrF32), POINTER(ScipyCsrF32), c_char_p, c_int, _alloc_t]),
        "c_xlinear_predict_on_selected_outputs_drm_f32": (None, [c_void_p, POINTER(ScipyDrmF32), POINTER(ScipyCsrF32), c_char_p, c_int, _alloc_t]),
        "c_xlinear_single_layer_predict_csr_f32": (None, [POINTER(ScipyCsrF32), POINTER(ScipyCsrF32), POINTER(ScipyCscF32), POINTER(ScipyCscF32), c_char_p, c_uint32, c_int, c_float, _alloc_t]),
        "c_xlinear_single_layer_predict_drm_f32": (None, [POINTER(ScipyDrmF32), POINTER(ScipyCsrF32), POINTER(ScipyCscF32), POINTER(ScipyCscF32), c_char_p, c_uint32, c_int, c_float, _alloc_t]),
        "c_xlinear_single_layer_predict_on_selected_outputs_csr_f32": (None, [POINTER(ScipyCsrF32), POINTER(ScipyCsrF32), POINTER(ScipyCsrF32), POINTER(ScipyCscF32), POINTER(ScipyCscF32), c_char_p, c_int, c_float, _alloc_t]),
        "c_xlinear_single_layer_predict_on_selected_outputs_drm_f32": (None, [POINTER(ScipyDrmF32), POINTER(ScipyCsrF32), POINTER(ScipyCsrF32), POINTER(ScipyCscF32), POINTER(ScipyCscF32), c_char_p, c_int, c_float, _alloc_t]),
        "c_sparse_inner_products_csr2csc_f32": (None, [POINTER(ScipyCsrF32), POINTER(ScipyCscF32), c_uint64, POINTER(c_uint32), POINTER(c_uint32), POINTER(c_float), c_int]),
        "c_sparse_inner_products_drm2csc_f32": (None, [POINTER(ScipyDrmF32), POINTER(ScipyCscF32), c_uint64, POINTER(c_uint32), POINTER(c_uint32), POINTER(c_float), c_int]),
        "c_sparse_inner_products_csr2dcm_f32": (None, [POINTER(ScipyCsrF32), POINTER(ScipyDcmF32), c_uint64, POINTER(c_uint32), POINTER(c_uint32), POINTER(c_float), c_int]),
        "c_sparse_inner_products_drm2dcm_f32": (None, [POINTER(ScipyDrmF32), POINTER(ScipyDcmF32), c_uint64, POINTER(c_uint32), POINTER(c_uint32), POINTER(c_float), c_int]),
        "c_sparse_matmul_csr_f32": (None, [POINTER(ScipyCsrF32), POINTER(ScipyCsrF32), _alloc_t, c_bool, c_bool, c_int]),
        "c_sparse_matmul_csc_f32": (None, [POINTER(ScipyCscF32), POINTER(ScipyCscF32), _alloc_t, c_bool, c_bool, c_int]),
        "xrl_smat_upload_csr": (c_void_p, [c_int, POINTER(ScipyCsrF32)]),
        "xrl_smat_from_device_csr": (c_void_p, [c_int, c_uint32, c_uint32, c_void_p, c_void_p, c_void_p, c_uint64]),
        "xrl_smat_from_device_result": (c_void_p, [c_int, c_uint32, c_uint32, c_void_p, c_void_p, c_void_p, c_uint32, c_void_p]),
        "xrl_smat_info": (c_int, [c_void_p, POINTER(c_uint64), c_uint32]),
        "xrl_smat_download": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
        "xrl_smat_copy_device": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
        "xrl_smat_free": (None, [c_void_p]),
        "xrl_sparse_matmul_device": (c_void_p, [c_void_p, c_void_p, c_int, c_int, c_void_p]),
        "xrl_debug_spgemm_forms": (c_int, [POINTER(c_uint64), c_uint32]),
        "xrl_run_clustering_device": (c_int, [c_void_p, c_uint64, POINTER(ClusteringParam), c_void_p, c_void_p, c_void_p]),
        "xrl_debug_cluster_plan": (c_int, [c_uint64, c_uint64, c_uint64, c_uint64, POINTER(ClusteringParam), c_void_p, c_void_p, c_void_p, c_void_p]),
        "xrl_debug_cluster_forms": (c_int, [POINTER(c_uint64), c_uint32]),
        "xrl_smat_transpose_device": (c_void_p, [c_void_p, c_void_p]),
        "xrl_smat_normalize_rows_device": (c_int, [c_void_p, c_int, POINTER(c_void_p), c_void_p]),
        "xrl_smat_normalize_rows_norm_device": (c_int, [c_void_p, c_int, c_int, POINTER(c_void_p), c_void_p]),
        "xrl_smat_hstack_device": (c_void_p, [POINTER(c_void_p), c_uint32, c_void_p]),
        "xrl_label_embedding_device": (c_void_p, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p]),
        "xrl_debug_embed_forms": (c_int, [POINTER(c_uint64), c_uint32]),
        "xrl_single_layer_train_csr_f32": (None, [POINTER(ScipyCsrF32), POINTER(ScipyCscF32), POINTER(ScipyCscF32), POINTER(ScipyCscF32), POINTER(ScipyCscF32),
                                                        _coo_alloc_t, c_double, c_uint32, c_int, c_double, c_double, c_uint64, c_double, c_double, c_int]),
        "xrl_single_layer_train_drm_f32": (None, [POINTER(ScipyDrmF32), POINTER(ScipyCscF32), POINTER(ScipyCscF32), POINTER(ScipyCscF32), POINTER(ScipyCscF32),
                                                        _coo_alloc_t, c_double, c_uint32, c_int, c_double, c_double, c_uint64, c_double, c_double, c_int]),
        "xrl_train_layer_device": (c_void_p, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_double, c_uint32, c_int, c_double, c_double, c_uint64, c_double,
                                              c_double, c_void_p]),
        "xrl_single_layer_train_newton_csr_f32": (None, [POINTER(ScipyCsrF32), POINTER(ScipyCscF32), POINTER(ScipyCscF32), POINTER(ScipyCscF32), POINTER(ScipyCscF32),
                                                         _coo_alloc_t, c_double, c_uint32, c_int, c_double, c_double, c_uint64, c_double, c_double, c_int]),
        "xrl_single_layer_train_newton_drm_f32": (None, [POINTER(ScipyDrmF32), POINTER(ScipyCscF32), POINTER(ScipyCscF32), POINTER(ScipyCscF32), POINTER(ScipyCscF32),
                                                         _coo_alloc_t, c_double, c_uint32, c_int, c_double, c_double, c_uint64, c_double, c_double, c_int]),
        "xrl_train_layer_newton_device": (c_void_p, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_double, c_uint32, c_int, c_double, c_double, c_uint64,
                                                     c_double, c_double, c_void_p]),
        "xrl_debug_train_counters": (c_int, [POINTER(c_uint64), c_uint32]),
        "xrl_debug_newton_counters": (c_int, [POINTER(c_uint64), c_uint32]),
        "xrl_smat_pattern_union_device": (c_void_p, [POINTER(c_void_p), c_uint32, c_void_p]),
        "xrl_single_layer_predict_device": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_uint32, c_char_p, c_uint32, c_float, c_void_p,
                                                    c_void_p, c_void_p, c_uint32, c_void_p]),
        "xrl_smat_check_relevance_device": (c_int, [c_void_p, c_void_p, POINTER(c_uint64), c_void_p]),
        "xrl_debug_match_forms": (c_int, [POINTER(c_uint64), c_uint32]),
        "xrl_hnsw_load": (c_int, [c_char_p, c_int, POINTER(c_void_p)]),
        "xrl_hnsw_check_folder": (c_int, [c_char_p, POINTER(c_uint64), c_uint32]),
        "xrl_hnsw_destruct": (None, [c_void_p]),
        "xrl_hnsw_info": (c_int, [c_void_p, POINTER(c_uint64), c_uint32]),
        "xrl_hnsw_searchers_create": (c_void_p, [c_void_p, c_uint32]),
        "xrl_hnsw_searchers_destruct": (None, [c_void_p]),
        "xrl_hnsw_predict_csr_f32": (c_int, [c_void_p, POINTER(ScipyCsrF32), POINTER(c_uint32), POINTER(c_float), c_uint32, c_uint32, c_int32, c_void_p]),
        "xrl_hnsw_predict_drm_f32": (c_int, [c_void_p, POINTER(ScipyDrmF32), POINTER(c_uint32), POINTER(c_float), c_uint32, c_uint32, c_int32, c_void_p]),
        "xrl_hnsw_predict_device": (c_int, [c_void_p, c_uint32, c_uint32, c_void_p, c_uint64, c_void_p, c_void_p, c_uint64, c_uint32, c_uint32, c_void_p, c_void_p,
                                            c_void_p, c_uint64, c_void_p, c_void_p]),
        "xrl_debug_hnsw_counters": (c_int, [POINTER(c_uint64), c_uint32, c_int]),
        "xrl_debug_hnsw_caps": (c_int, [POINTER(c_uint64), c_uint32]),
        "xrl_inspect_model": (c_int, [c_char_p, POINTER(c_uint64), c_uint32]),
        "xrl_model_create": (c_void_p, [c_uint32, c_void_p, c_void_p, POINTER(c_float), POINTER(c_uint32), POINTER(c_char_p)]),
        "xrl_queries_upload_csr": (c_void_p, [c_void_p, POINTER(ScipyCsrF32)]),
        "xrl_queries_upload_drm": (c_void_p, [c_void_p, POINTER(ScipyDrmF32)]),
        "xrl_queries_from_device_csr": (c_void_p, [c_void_p, c_uint32, c_uint32, c_void_p, c_void_p, c_void_p, c_uint64]),
        "xrl_queries_from_device_drm": (c_void_p, [c_void_p, c_uint32, c_uint32, c_void_p]),
        "xrl_queries_concat_device": (c_void_p, [c_void_p, c_uint32, c_uint32, c_void_p, c_void_p, c_void_p, c_uint64, c_uint32, c_void_p, c_void_p]),
        "xrl_queries_tfidf_device": (c_void_p, [c_void_p, c_uint32, c_uint32, c_void_p, c_void_p, c_void_p, c_uint64, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
        "xrl_queries_concat_device_ex": (c_void_p, [c_void_p, c_uint32, c_uint32, c_void_p, c_void_p, c_void_p, c_uint64, c_uint32, c_void_p, c_int, c_void_p]),
        "xrl_queries_info": (c_int, [c_void_p, POINTER(c_uint64)]),
        "xrl_queries_download": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
        "xrl_queries_free": (None, [c_void_p]),
        "c_tfidf_load": (c_void_p, [c_char_p]),
        "c_tfidf_destruct": (None, [c_void_p]),
        "c_tfidf_predict": (None, [c_void_p, c_void_p, POINTER(c_uint64), c_uint64, c_int, _alloc_t]),
        "c_tfidf_predict_from_file": (None, [c_void_p, c_void_p, c_uint64, c_uint64, c_int, _alloc_t]),
        "xrl_tfidf_counts": (None, [c_void_p, c_void_p, POINTER(c_uint64), c_uint64, c_int, _alloc_t]),
        "xrl_tfidf_nr_features": (c_uint32, [c_void_p]),
        "xrl_tfidf_predict_device": (c_void_p, [c_void_p, c_void_p, c_void_p, POINTER(c_uint64), c_uint64, c_int]),
        "xrl_tfidf_counts_device": (c_void_p, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_uint64, c_void_p, c_void_p]),
        "xrl_tfidf_predict_device_text": (c_void_p, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_uint64, c_void_p]),
        "xrl_tfidf_predict_device_tok": (c_void_p, [c_void_p, c_void_p, c_void_p, POINTER(c_uint64), c_uint64, c_int, c_int]),
        "xrl_tfidf_device_bytes": (c_uint64, [c_void_p, c_int]),
        "xrl_debug_tfidf_device_forms": (c_int, [c_void_p, POINTER(c_uint64), c_uint32]),
        "xrl_tfidf_train": (c_void_p, [c_void_p, POINTER(c_uint64), c_uint64, POINTER(TfidfVectorizerParam), c_int]),
        "xrl_tfidf_train_device": (c_void_p, [c_int, c_void_p, c_void_p, c_void_p, c_uint64, POINTER(TfidfVectorizerParam), c_void_p]),
        "xrl_tfidf_save": (None, [c_void_p, c_char_p]),
        "xrl_tfidf_transform_device": (c_void_p, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_uint64, c_void_p, c_void_p]),
        "xrl_tfidf_export": (c_int, [c_void_p, c_uint32, POINTER(c_uint64), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
        "xrl_debug_tfidf_train_forms": (c_int, [c_void_p, POINTER(c_uint64), c_uint32]),
        "xrl_queries_concat_handle": (c_void_p, [c_void_p, c_void_p, c_uint32, c_void_p, c_int, c_void_p]),
        "xrl_predict_device": (c_int, [c_void_p, c_void_p, c_uint32, c_char_p, c_uint32, c_void_p, c_void_p, c_void_p, c_uint32, c_void_p, c_int]),
        "xrl_predict_device_rows": (c_int, [c_void_p, c_void_p, c_uint32, c_char_p, c_uint32, c_void_p, c_void_p, c_void_p, c_uint32, c_void_p, c_int, c_uint32, c_uint32]),
        "xrl_ensemble_device": (c_int, [c_int, c_uint32, c_uint32, POINTER(c_void_p), POINTER(c_void_p), POINTER(c_void_p), POINTER(c_uint32), c_int,
                                        POINTER(c_float), c_uint32, c_void_p, c_void_p, c_void_p, c_uint32, c_void_p, c_int]),
        "xrl_ensemble_methods_device": (c_int, [c_int, c_uint32, c_uint32, POINTER(c_void_p), POINTER(c_void_p), POINTER(c_void_p), POINTER(c_uint32), c_int,
                                                c_uint32, c_void_p, c_void_p, c_void_p, c_uint32, c_void_p, c_int]),
        "xrl_metrics_device": (c_int, [c_int, c_uint32, c_void_p, c_void_p, c_void_p, c_uint32, c_void_p, c_void_p, c_uint32, c_void_p, c_void_p, c_void_p, c_int]),
        "xrl_predict_selected_device": (c_int, [c_void_p, c_void_p, c_char_p, c_void_p, c_void_p, c_uint32, c_void_p, c_void_p, c_void_p, c_uint32, c_void_p, c_void_p, c_int]),
        "xrl_set_output_constraint": (c_int, [c_void_p, c_void_p, c_uint64]),
        "xrl_set_output_constraint_device": (c_int, [c_void_p, c_void_p, c_uint64, c_void_p]),
        "xrl_clear_output_constraint": (c_int, [c_void_p]),
        "xrl_output_constraint_info": (c_int, [c_void_p, POINTER(c_uint64), c_uint32]),
        "xrl_debug_output_constraint_view": (c_int, [c_void_p, c_uint32, c_void_p, c_uint64, c_void_p, c_uint64]),
        "xrl_predict_stats": (c_int, [c_void_p, c_void_p, c_uint32, c_char_p, c_uint32, POINTER(c_double), c_uint32]),
        "xrl_effective_topk": (c_uint32, [c_void_p, c_uint32]),
        "xrl_profile_enable": (None, [c_void_p, c_int]),
        "xrl_profile_reset": (None, [c_void_p]),
        "xrl_profile_get": (c_uint32, [c_void_p, POINTER(ProfileRec), c_uint32]),
        "xrl_set_option": (c_int, [c_void_p, c_char_p, c_int64]),
        "xrl_model_device_bytes": (c_uint64, [c_void_p]),
        "xrl_debug_k1_phases": (None, [POINTER(c_uint64), c_int]),
        "xrl_debug_split_chunk": (c_uint32, [POINTER(c_uint64), c_uint32, c_uint64]),
        "xrl_debug_layout_rows": (c_uint64, [POINTER(c_uint32), c_uint32, c_int, POINTER(c_uint32)]),
        "xrl_debug_k2_form": (c_int, [c_uint32, c_uint32, c_int64, c_int, c_uint32, POINTER(c_uint32)]),
        "xrl_debug_host_batches": (c_uint32, [POINTER(c_uint64), c_uint32, c_uint32, c_int, POINTER(c_uint32), c_uint32]),
        "xrl_layer_info": (c_uint32, [c_void_p, c_uint32, POINTER(c_uint64), c_uint32]),
        "xrl_single_layer_cache_clear": (None, []),
        "xrl_single_layer_cache_stats": (None, [POINTER(c_uint64), POINTER(c_uint64), POINTER(c_uint64)]),
    }

    # ... and the two the header declares under the reference's own prefix (base.py:1591-1606 link_clustering)
    CLUSTERING_SIGNATURES = {
        "c_run_clustering_csr_f32": (None, [POINTER(ScipyCsrF32), c_uint64, POINTER(ClusteringParam), POINTER(c_uint32)]),
        "c_run_clustering_drm_f32": (None, [POINTER(ScipyDrmF32), c_uint64, POINTER(ClusteringParam), POINTER(c_uint32)]),
    }

    @classmethod
    def _link(cls, lib):
        for name, (res, args) in list(cls.SIGNATURES.items()) + list(cls.CLUSTERING_SIGNATURES.items()):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args

    @staticmethod
    def _x_view(X, check_sorted=True, not_implemented=None):
        """A caller's query matrix as (zero-copy view, "csr" or "drm": the suffix of the symbol that takes that view)."""
        if isinstance(X, smat.csr_matrix):
            if check_sorted and not X.has_sorted_indices:
                raise ValueError("Query matrix does not have sorted indices!")
            X = ScipyCsrF32.init_from(X)
        elif isinstance(X, np.ndarray):
            X = ScipyDrmF32.init_from(X)
        if isinstance(X, ScipyCsrF32):
            return X, "csr"
        if isinstance(X, ScipyDrmF32):
            return X, "drm"
        raise NotImplementedError(not_implemented or "type(X) = {} not implemented".format(type(X)))

    @staticmethod
    def _cstr(s):
        """An optional string argument: utf-8 bytes, or NULL for None / ""."""
        return s.encode("utf-8") if s else None

    @contextlib.contextmanager
    def freeing(self, *handles):
        """``with clib.freeing(q, q2): ...`` frees the query handles when the block ends, also by an exception; ``None`` is skipped."""
        try:
            yield
        finally:
            for h in handles:
                if h is not None:
                    self.queries_free(h)

    def _check(self):
        err = self.clib_float32.xrl_last_error()
        if err:
            self.clib_float32.xrl_clear_error()
            raise RuntimeError(err.decode("utf-8", "replace"))

    def _checked(self, value):
        """``value``, the result of a native call, once that call is known to have left no error."""
        self._check()
        return value

    # ------------------------------------------------------------------ device management (additive)
    def device_count(self):
        return int(self.clib_float32.xrl_device_count())

    def set_device(self, device):
        self.clib_float32.xrl_set_device(int(device))
        self._check()

    def inspect_model(self, folder):
        """Host-only parse of a model folder (no GPU needed): list of per-layer shape dicts."""
        buf = (c_uint64 * (6 * 64))()
        depth = self.clib_float32.xrl_inspect_model(folder.encode("utf-8"), buf, 6 * 64)
        self._check()
        keys = ("w_rows", "w_cols", "w_nnz", "c_rows", "c_cols", "c_nnz")
        return [dict(zip(keys, [int(buf[6 * d + i]) for i in range(6)])) for d in range(depth)]

    # ------------------------------------------------------------------ xlinear (base.py:978-1405)
    def xlinear_load_predict_only(self, folder, weight_matrix_type="BINARY_SEARCH_CHUNKED"):
        """Load a model folder (``<model>/ranker``) onto the GPU; returns the native handle."""
        type_id = XLINEAR_INFERENCE_MODEL_TYPES[weight_matrix_type]
        cmodel = self.clib_float32.c_xlinear_load_model_from_disk_ext(c_char_p(folder.encode("utf-8")), c_int(int(type_id)))
        self._check()
        return cmodel

    def xlinear_load_mmap(self, folder, lazy_load=False):
        """Load a memory-mapped model folder (base.py:990-1009)."""
        cmodel = self.clib_float32.c_xlinear_load_mmap_model_from_disk(c_char_p(folder.encode("utf-8")), c_bool(lazy_load))
        self._check()
        return cmodel

    def xlinear_compile_mmap_model(self, npz_folder, mmap_folder):
        """npz model folder -> mmap model folder (base.py:978-988); host-only."""
        self.clib_float32.c_xlinear_compile_mmap_model(c_char_p(npz_folder.encode("utf-8")), c_char_p(mmap_folder.encode("utf-8")))
        self._check()

    def xlinear_destruct_model(self, c_model):
        if self._lib is not None and c_model:
            self._lib.c_xlinear_destruct_model(c_void_p(c_model))

    def xlinear_get_int_attr(self, c_model, attr):
        assert attr in {"depth", "nr_features", "nr_labels", "nr_codes", "nr_pred_cols", "nr_bucket_layers", "nr_bitmap64_layers", "nr_dense_layers", "merged01", "device", "nr_devices"}, f"attr {attr} not implemented"
        v = self.clib_float32.c_xlinear_get_int_attr(c_void_p(c_model), c_char_p(attr.encode("utf-8")))
        self._check()
        return v

    def xlinear_get_layer_type(self, c_model, layer_depth):
        v = self.clib_float32.c_xlinear_get_layer_type(c_void_p(c_model), layer_depth)
        self._check()
        return v

    def xlinear_predict(self, c_model, X, overriden_beam_size, overriden_post_processor_str, overriden_only_topk,
                        threads, pred_alloc):
        """Full beam-search prediction (base.py:1041-1095).  ``None``/0 overrides = model defaults."""
        clib = self.clib_float32
        X, fmt = self._x_view(X)
        c_predict = getattr(clib, f"c_xlinear_predict_{fmt}_f32")
        cb = pred_alloc.cfunc
        c_predict(c_void_p(c_model), byref(X), overriden_beam_size if overriden_beam_size else 0,
                  self._cstr(overriden_post_processor_str), overriden_only_topk if overriden_only_topk else 0, threads, cb)
        self._check()

    def xlinear_predict_on_selected_outputs(self, c_model, X, selected_outputs_csr, overriden_post_processor_str, threads,
                                            pred_alloc):
        """Scores for a given (query, label) pattern (base.py:1097-1141)."""
        clib = self.clib_float32
        X, fmt = self._x_view(X)
        if not isinstance(selected_outputs_csr, smat.csr_matrix):
            raise ValueError("type(selected_outputs_csr) = {} not implemented".format(type(selected_outputs_csr)))
        S = ScipyCsrF32.init_from(selected_outputs_csr.astype(np.float32))
        c_predict = getattr(clib, f"c_xlinear_predict_on_selected_outputs_{fmt}_f32")
        cb = pred_alloc.cfunc
        c_predict(c_void_p(c_model), byref(X), byref(S), self._cstr(overriden_post_processor_str), threads, cb)
        self._check()

    def xlinear_single_layer_predict(self, X, csr_codes, W, C, post_processor_str, only_topk, num_threads, bias, pred_alloc):
        """One layer from python-owned W / C (base.py:1143-1207)."""
        clib = self.clib_float32
        post_processor_str = post_processor_str.encode("utf-8")
        W = ScipyCscF32.init_from(W)
        C = ScipyCscF32.init_from(C)
        X, fmt = self._x_view(X)
        c_predict = getattr(clib, f"c_xlinear_single_layer_predict_{fmt}_f32")
        codes = ScipyCsrF32.init_from(csr_codes)
        cb = pred_alloc.cfunc
        c_predict(byref(X), byref(codes) if codes is not None else None, byref(W),
                  byref(C) if C is not None else None, post_processor_str, only_topk, num_threads, bias, cb)
        self._check()

    def xlinear_single_layer_predict_on_selected_outputs(self, X, selected_outputs_csr, csr_codes, W, C, post_processor_str,
                                                         num_threads, bias, pred_alloc):
        """One layer from python-owned W / C on a given output pattern (base.py:1227-1303)."""
        clib = self.clib_float32
        post_processor_str = post_processor_str.encode("utf-8")
        W = ScipyCscF32.init_from(W)
        S = ScipyCsrF32.init_from(selected_outputs_csr.astype(np.float32))
        X, fmt = self._x_view(X)
        fn = getattr(clib, f"c_xlinear_single_layer_predict_on_selected_outputs_{fmt}_f32")
        if C is None:
            C = smat.csc_matrix(np.ones((W.shape[1], 1), dtype=np.float32))
        C = ScipyCscF32.init_from(C)
        if csr_codes is not None:
            if csr_codes.shape[0] != X.shape[0]:
                raise ValueError("Instance dimension of query and csr_codes matrix do not match")
            if csr_codes.shape[1] != C.shape[1]:
                raise ValueError("Label dimension of csr_codes and C matrix do not match")
            csr_codes = ScipyCsrF32.init_from(csr_codes)
        cb = pred_alloc.cfunc
        fn(byref(X), byref(S), byref(csr_codes) if csr_codes is not None else None, byref(W), byref(C), post_processor_str,
           num_threads, bias, cb)
        self._check()

    def sparse_inner_products(self, X, W, X_row_idx, W_col_idx, pred_values=None, threads=-1):
        """val[i] = <X[X_row_idx[i], :], W[:, W_col_idx[i]]>  (base.py:1536-1589)."""
        clib = self.clib_float32
        nnz = len(X_row_idx)
        assert nnz == len(W_col_idx)
        assert X.shape[1] == W.shape[0]
        unknown = "type(X)={} and type(W)={} no implemented".format(type(X), type(W))
        pX, x_fmt = self._x_view(X, check_sorted=False, not_implemented=unknown)      # (unsorted indices are accepted here)
        if isinstance(W, smat.csc_matrix):
            pW, w_fmt = ScipyCscF32.init_from(W), "csc"
        elif isinstance(W, np.ndarray):
            pW, w_fmt = ScipyDcmF32.init_from(W), "dcm"
        else:
            raise NotImplementedError(unknown)
        fn = getattr(clib, f"c_sparse_inner_products_{x_fmt}2{w_fmt}_f32")
        if pred_values is None or len(pred_values) != nnz or pred_values.dtype != np.float32:
            pred_values = np.zeros(nnz, pW.dtype)
        rows = np.ascontiguousarray(X_row_idx, dtype=np.uint32)
        cols = np.ascontiguousarray(W_col_idx, dtype=np.uint32)
        fn(byref(pX), byref(pW), nnz, rows.ctypes.data_as(POINTER(c_uint32)), cols.ctypes.data_as(POINTER(c_uint32)),
           pred_values.ctypes.data_as(POINTER(c_float)), threads)
        self._check()
        return pred_values

    def sparse_matmul(self, X, Y, eliminate_zeros=False, sorted_indices=True, threads=-1):
        """X * Y of two sparse matrices on the device (K10), with the reference's dispatch and result (base.py:1460-1534): CSC x CSC and
        CSR x CSR go to the entry point of their format, a mixed pair converts the operand with the smaller nnz; returns a
        ``csc_matrix`` / ``csr_matrix`` of that format.  ``threads`` is accepted and ignored."""
        if X.shape[1] != Y.shape[0]:
            raise ValueError("X.shape[1]={} != Y.shape[0]={}".format(X.shape[1], Y.shape[0]))
        clib = self.clib_float32
        pred_alloc = ScipyCompressedSparseAllocator()

        def is_col_major(A):
            return isinstance(A, (smat.csc_matrix, ScipyCscF32))

        def is_row_major(A):
            return isinstance(A, (smat.csr_matrix, ScipyCsrF32))

        if is_col_major(X) and is_col_major(Y):
            fmt = "csc"
        elif is_row_major(X) and is_row_major(Y):
            fmt = "csr"
        elif is_col_major(X) and is_row_major(Y):
            fmt = "csc" if X.nnz > Y.nnz else "csr"
        elif is_row_major(X) and is_col_major(Y):
            fmt = "csr" if X.nnz > Y.nnz else "csc"
        else:
            raise ValueError("X and Y should be either csr_matrix/csc_matrix/ScipyCscF32/ScipyCsrF32 !")
        if fmt == "csc":
            view, to_fmt, is_fmt = ScipyCscF32, "tocsc", is_col_major
        else:
            view, to_fmt, is_fmt = ScipyCsrF32, "tocsr", is_row_major
        pX, pY = (view.init_from(A if is_fmt(A) else getattr(A, to_fmt)()) for A in (X, Y))
        getattr(clib, f"c_sparse_matmul_{fmt}_f32")(pX, pY, pred_alloc.cfunc, eliminate_zeros, sorted_indices, threads)
        self._check()
        return pred_alloc.get()

    # ------------------------------------------------------------------ device matrices and their products (additive, K10)
    def smat_upload_csr(self, device, X):
        """A scipy CSR (float32) copied to ``device``: a matrix handle that owns the copy (free it with :meth:`smat_free`)."""
        h = self.clib_float32.xrl_smat_upload_csr(int(device), byref(ScipyCsrF32.init_from(X)))
        self._check()
        return h

    def smat_from_device_csr(self, device, rows, cols, row_ptr_addr, col_idx_addr, val_addr, nnz):
        """Wrap a CSR that already lives in HBM on ``device`` (raw addresses: u64 row_ptr, u32 col_idx, f32 val); non-owning."""
        h = self.clib_float32.xrl_smat_from_device_csr(int(device), int(rows), int(cols), c_void_p(row_ptr_addr), c_void_p(col_idx_addr),
                                                       c_void_p(val_addr), int(nnz))
        self._check()
        return h

    def smat_from_device_result(self, device, rows, cols, d_idx, d_val, d_cnt, stride, stream=None):
        """A fixed-stride result (raw addresses; ``d_cnt`` None = ``stride`` entries in every row) as a rows x cols CSR the handle owns."""
        h = self.clib_float32.xrl_smat_from_device_result(int(device), int(rows), int(cols), c_void_p(d_idx), c_void_p(d_val), c_void_p(d_cnt or 0),
                                                          int(stride), c_void_p(stream or 0))
        self._check()
        return h

    def smat_info(self, h):
        """dict(rows, cols, nnz, device, row_ptr, col_idx, val) of a matrix handle; the last three are device addresses."""
        out = (c_uint64 * 7)()
        self.clib_float32.xrl_smat_info(c_void_p(h), out, 7)
        self._check()
        return dict(zip(("rows", "cols", "nnz", "device", "row_ptr", "col_idx", "val"), (int(v) for v in out)))

    def _download_csr(self, download, h, rows, cols, nnz):
        """``download(h, row_ptr, col_idx, val)`` of a handle's CSR into fresh arrays -> a scipy CSR with the stored order and explicit zeros kept."""
        ptr = np.zeros(rows + 1, dtype=np.uint64); idx = np.zeros(max(nnz, 1), dtype=np.uint32); val = np.zeros(max(nnz, 1), dtype=np.float32)
        download(c_void_p(h), ptr.ctypes.data_as(c_void_p), idx.ctypes.data_as(c_void_p), val.ctypes.data_as(c_void_p)); self._check()
        m = smat.csr_matrix((rows, cols), dtype=np.float32)
        m.indptr, m.indices, m.data = ptr.astype(np.int64), idx[:nnz].astype(np.int64), val[:nnz]      # assigned directly: keeps explicit zeros / order
        return m

    def smat_download(self, h):
        """Copy of a matrix handle back to the host: a scipy CSR with the stored order and explicit zeros kept."""
        info = self.smat_info(h)
        return self._download_csr(self.clib_float32.xrl_smat_download, h, info["rows"], info["cols"], info["nnz"])

    def smat_copy_device(self, h, row_ptr_addr, col_idx_addr, val_addr, stream=None):
        """The handle's arrays into the caller's device buffers (raw addresses, sized from :meth:`smat_info`); synchronises ``stream``."""
        rc = self.clib_float32.xrl_smat_copy_device(c_void_p(h), c_void_p(row_ptr_addr), c_void_p(col_idx_addr or 0), c_void_p(val_addr or 0),
                                                    c_void_p(stream or 0))
        self._check()
        return rc

    def smat_free(self, h):
        if self._lib is not None and h:
            self._lib.xrl_smat_free(c_void_p(h))

    def sparse_matmul_device(self, A, B, eliminate_zeros=False, sorted_indices=True, stream=None):
        """A new matrix handle with A * B of two matrix handles of one device (free it with :meth:`smat_free`)."""
        h = self.clib_float32.xrl_sparse_matmul_device(c_void_p(A), c_void_p(B), 1 if eliminate_zeros else 0, 1 if sorted_indices else 0,
                                                       c_void_p(stream or 0))
        self._check()
        return h

    def debug_spgemm_forms(self):
        """Debug counters of K10 since the load: its CAP, rows served by the LDS form, by the big form, batches of the big form, products."""
        out = (c_uint64 * 5)()
        self.clib_float32.xrl_debug_spgemm_forms(out, 5)
        self._check()
        return dict(zip(("cap", "lds_rows", "big_rows", "batches", "calls"), (int(v) for v in out)))

    # ------------------------------------------------------------------ label embeddings (K12)
    EMBED_METHODS = {"pifa": 0, "pifa_lf_concat": 1, "pii": 2}

    def smat_transpose_device(self, h, stream=None):
        """A new matrix handle with the transpose of a CSR handle in scipy's stable order (free it with :meth:`smat_free`)."""
        t = self.clib_float32.xrl_smat_transpose_device(c_void_p(h), c_void_p(stream or 0))
        self._check()
        return t

    ROW_NORMS = {"l1": 1, "l2": 2, "max": 3}

    def smat_normalize_rows_device(self, h, in_place=False, stream=None, norm="l2"):
        """Row normalisation in sklearn's arithmetic (``norm``: l2, l1 or max): a new matrix handle, or with ``in_place`` None after the
        handle's own values (the caller's array, for a wrapped handle) were rewritten."""
        out = c_void_p()
        if norm == "l2":
            self.clib_float32.xrl_smat_normalize_rows_device(c_void_p(h), 1 if in_place else 0, byref(out), c_void_p(stream or 0))
        else:
            if norm not in self.ROW_NORMS:
                raise ValueError(f"'{norm}' is not a supported norm; supported: {sorted(self.ROW_NORMS)}")
            self.clib_float32.xrl_smat_normalize_rows_norm_device(c_void_p(h), self.ROW_NORMS[norm], 1 if in_place else 0, byref(out), c_void_p(stream or 0))
        self._check()
        return None if in_place else out.value

    def smat_hstack_device(self, handles, stream=None):
        """A new matrix handle ``[M0 M1 ...]`` of matrix handles with one row count on one device."""
        arr = (c_void_p * max(len(handles), 1))(*handles)
        h = self.clib_float32.xrl_smat_hstack_device(arr, len(handles), c_void_p(stream or 0))
        self._check()
        return h

    def label_embedding_device(self, Y, X=None, Z=None, method="pifa", normalized_Y=True, stream=None):
        """A new matrix handle with the label embedding of matrix handles ``Y`` (samples x labels), ``X`` (samples x features) and, for
        ``pifa_lf_concat``, ``Z`` (labels x label-features); ``method`` is a name of :attr:`EMBED_METHODS` or its number."""
        m = self.EMBED_METHODS.get(method, method) if isinstance(method, str) else method
        if not isinstance(m, int):
            raise NotImplementedError(f"label embedding method '{method}' is not served on the device; served: {sorted(self.EMBED_METHODS)}")
        h = self.clib_float32.xrl_label_embedding_device(c_void_p(Y), c_void_p(X or 0), c_void_p(Z or 0), m, 1 if normalized_Y else 0, c_void_p(stream or 0))
        self._check()
        return h

    def debug_embed_forms(self):
        """Debug counters of K12 since the load: its CAP, transposed rows served in LDS and by the big form, normalised rows served one
        per lane and by a wavefront."""
        out = (c_uint64 * 5)()
        self.clib_float32.xrl_debug_embed_forms(out, 5)
        self._check()
        return dict(zip(("cap", "t_lds", "t_big", "n_lane", "n_wave"), (int(v) for v in out)))

    # ------------------------------------------------------------------ ranker training (K13)
    TRAIN_COUNTERS = ("jobs", "batches", "slots", "stride", "iters", "shrinks", "reactivations", "max_iter_stops", "clipped", "lane_rows", "wave_rows",
                      "extensions", "reruns")

    @staticmethod
    def _solver_number(solver_type):
        if isinstance(solver_type, str):
            if solver_type not in XLINEAR_SOLVERS:
                raise ValueError(f"unknown solver_type '{solver_type}'; known: {sorted(XLINEAR_SOLVERS)}")
            return XLINEAR_SOLVERS[solver_type]
        return int(solver_type)

    def _train_symbol(self, solver_type, pattern):
        """The entry point that serves a solver: K16's (``..._newton...``) for L2R_L2LOSS_SVC_PRIMAL, K13's for every other number (which
        refuses what it does not serve)."""
        return getattr(self.clib_float32, pattern.format("_newton" if self._solver_number(solver_type) == XLINEAR_SOLVERS["L2R_L2LOSS_SVC_PRIMAL"] else ""))

    def xlinear_single_layer_train(self, pX, pY, pC, pM, pR, threshold=0.1, max_nonzeros_per_label=None, solver_type="L2R_L2LOSS_SVC_DUAL", Cp=1.0, Cn=1.0,
                                   max_iter=1000, eps=0.1, bias=1.0, threads=-1, verbose=0, **kwargs):
        """One layer's weights trained on the device (K13; ``xrl_single_layer_train_{csr,drm}_f32``, the reference's argument list under this
        library's prefix), with the reference's dispatch and return (base.py:1302-1373): ``pX`` is a
        ScipyCsrF32 or ScipyDrmF32 view, ``pY`` / ``pC`` / ``pM`` / ``pR`` are ScipyCscF32 views (``pC`` / ``pM`` None: pure multi-label,
        ``pR`` None: every positive costs 1).  Returns the float32 ``csc_matrix`` W, (features + (bias > 0)) x labels.  The weights are
        the reference's at threads = 1 bit for bit; ``threads`` and ``verbose`` are accepted and ignored."""
        coo_alloc = ScipyCoordinateSparseAllocator(dtype=np.float32)
        if isinstance(pX, ScipyCsrF32):
            train = self._train_symbol(solver_type, "xrl_single_layer_train{}_csr_f32")
        elif isinstance(pX, ScipyDrmF32):
            train = self._train_symbol(solver_type, "xrl_single_layer_train{}_drm_f32")
        else:
            raise NotImplementedError("type(pX) = {} not implemented".format(type(pX)))
        train(byref(pX), byref(pY), byref(pC) if pC is not None else None, byref(pM) if pM is not None else None, byref(pR) if pR is not None else None,
              coo_alloc.cfunc, threshold, 0 if max_nonzeros_per_label is None else max_nonzeros_per_label, self._solver_number(solver_type), Cp, Cn, max_iter,
              eps, bias, threads)
        self._check()
        return coo_alloc.tocsc().astype(np.float32)

    def train_layer_device(self, X, Yt, Ct=None, Mt=None, Rt=None, threshold=0.1, max_nonzeros_per_label=None, solver_type="L2R_L2LOSS_SVC_DUAL", Cp=1.0,
                           Cn=1.0, max_iter=1000, eps=0.1, bias=1.0, stream=None):
        """A new matrix handle with W^T (labels x (features + (bias > 0)), CSR = the CSC of W) trained from matrix handles: X and the
        TRANSPOSES of Y, C, M and R (free it with :meth:`smat_free`)."""
        h = self._train_symbol(solver_type, "xrl_train_layer{}_device")(c_void_p(X), c_void_p(Yt), c_void_p(Ct or 0), c_void_p(Mt or 0), c_void_p(Rt or 0), threshold,
                                                     0 if max_nonzeros_per_label is None else max_nonzeros_per_label, self._solver_number(solver_type), Cp, Cn,
                                                     max_iter, eps, bias, c_void_p(stream or 0))
        self._check()
        return h

    def debug_train_counters(self):
        """What the last training of this process ran (``xrl_debug_train_counters``), by name."""
        out = (c_uint64 * len(self.TRAIN_COUNTERS))()
        self.clib_float32.xrl_debug_train_counters(out, len(self.TRAIN_COUNTERS))
        self._check()
        return dict(zip(self.TRAIN_COUNTERS, (int(v) for v in out)))

    NEWTON_COUNTERS = ("jobs", "batches", "slots", "stride", "newton_iters", "cg_iters", "hv_calls", "halvings", "end_before_first", "end_gradient",
                       "end_linesearch", "end_actred", "end_cap", "cg_dhd", "cg_q", "cg_positive", "cg_cap", "lane_rows", "wave_rows", "nonfinite_jobs")

    def newton_counters(self):
        """What the last primal training (L2R_L2LOSS_SVC_PRIMAL, K16) of this process ran (``xrl_debug_newton_counters``), by name."""
        out = (c_uint64 * len(self.NEWTON_COUNTERS))()
        self.clib_float32.xrl_debug_newton_counters(out, len(self.NEWTON_COUNTERS))
        self._check()
        return dict(zip(self.NEWTON_COUNTERS, (int(v) for v in out)))

    # ------------------------------------------------------------------ matching matrices and a trained layer's prediction in HBM (K14)
    MATCH_FORMS = ("lds_rows", "big_rows", "read", "written", "last_bound")

    def smat_pattern_union_device(self, handles, stream=None):
        """A new matrix handle that stores a 1 wherever one of the matrix handles (one shape, one device) stores an entry, rows ascending."""
        handles = list(handles)
        arr = (c_void_p * max(len(handles), 1))(*handles)
        h = self.clib_float32.xrl_smat_pattern_union_device(arr, len(handles), c_void_p(stream or 0))
        self._check()
        return h

    def smat_check_relevance_device(self, Y, R, stream=None):
        """``(code, row)`` of ``xrl_smat_check_relevance_device`` over two matrix handles: code 0 when R stores exactly Y's entries and no
        negative value, else 1 (row pointers), 2 (column ids) or 3 (a value below 0) and the first row that offends."""
        status = (c_uint64 * 2)()
        self.clib_float32.xrl_smat_check_relevance_device(c_void_p(Y), c_void_p(R), status, c_void_p(stream or 0))
        self._check()
        return int(status[0]), int(status[1])

    def single_layer_predict_device(self, X, Wt, Ct, codes_idx, codes_val, codes_cnt, codes_stride, post_processor, only_topk, bias, out_idx, out_val, out_cnt,
                                    out_stride, stream=None):
        """One layer predicted from matrix handles (X, W^T, C^T or None) and codes in HBM (raw addresses, all None: no csr_codes) into the
        caller's fixed-stride device buffers; synchronises ``stream``."""
        rc = self.clib_float32.xrl_single_layer_predict_device(c_void_p(X), c_void_p(Wt), c_void_p(Ct or 0), c_void_p(codes_idx or 0), c_void_p(codes_val or 0),
                                                               c_void_p(codes_cnt or 0), int(codes_stride), self._cstr(post_processor), int(only_topk), float(bias),
                                                               c_void_p(out_idx or 0), c_void_p(out_val or 0), c_void_p(out_cnt or 0), int(out_stride),
                                                               c_void_p(stream or 0))
        self._check()
        return rc

    def debug_match_forms(self):
        """Debug counters of K14 since the load (``xrl_debug_match_forms``), by name."""
        out = (c_uint64 * len(self.MATCH_FORMS))()
        self.clib_float32.xrl_debug_match_forms(out, len(self.MATCH_FORMS))
        self._check()
        return dict(zip(self.MATCH_FORMS, (int(v) for v in out)))

    # ------------------------------------------------------------------ HNSW search (K17)
    HNSW_INFO = ("num_node", "feat_dim", "maxM", "maxM0", "efC", "max_level", "init_node", "data_type", "metric_type", "device_bytes")
    HNSW_COUNTERS = ("dist", "pops", "admissions", "passes", "max_cand", "rerun", "lds_queries", "hbm_queries")

    def _hnsw_info(self, out):
        d = dict(zip(self.HNSW_INFO, (int(v) for v in out)))
        d["data_type"], d["metric_type"] = ("csr", "drm")[d["data_type"]], ("ip", "l2")[d["metric_type"]]
        return d

    def hnsw_load(self, c_model_dir, device=0):
        """``xrl_hnsw_load``: the reference's ``c_model`` folder (config.json + index.mmap_store) into HBM -> handle."""
        h = c_void_p()
        self.clib_float32.xrl_hnsw_load(self._cstr(c_model_dir), int(device), ctypes.byref(h))
        self._check()
        return h

    def hnsw_check_folder(self, c_model_dir):
        """The loader's reading and refusals without a GPU (``xrl_hnsw_check_folder``) -> the info dictionary."""
        out = (c_uint64 * 10)()
        self.clib_float32.xrl_hnsw_check_folder(self._cstr(c_model_dir), out, 10)
        self._check()
        return self._hnsw_info(out)

    def hnsw_destruct(self, h):
        self.clib_float32.xrl_hnsw_destruct(h)

    def hnsw_info(self, h):
        out = (c_uint64 * 10)()
        self.clib_float32.xrl_hnsw_info(h, out, 10)
        self._check()
        return self._hnsw_info(out)

    def hnsw_searchers_create(self, h, num_searcher):
        p = self.clib_float32.xrl_hnsw_searchers_create(h, int(num_searcher))
        self._check()
        return c_void_p(p)

    def hnsw_searchers_destruct(self, p):
        self.clib_float32.xrl_hnsw_searchers_destruct(p)

    def hnsw_predict(self, h, pX, data_type, indices, distances, efS, topk, threads=1, searchers=None):
        """``xrl_hnsw_predict_{csr,drm}_f32`` into the caller's ``indices`` uint32 / ``distances`` float32 arrays of rows * topk entries."""
        fn = getattr(self.clib_float32, "xrl_hnsw_predict_%s_f32" % data_type)
        fn(h, ctypes.byref(pX), indices.ctypes.data_as(POINTER(c_uint32)), distances.ctypes.data_as(POINTER(c_float)), efS, topk, threads, searchers)
        self._check()

    def hnsw_predict_device(self, h, rows, cols, val_addr, row_stride, row_ptr_addr, col_idx_addr, nnz, efS, topk, d_idx, d_dist, d_count, out_stride,
                            searchers=None, stream=None):
        self.clib_float32.xrl_hnsw_predict_device(h, rows, cols, c_void_p(val_addr or 0), row_stride, c_void_p(row_ptr_addr or 0), c_void_p(col_idx_addr or 0), nnz,
                                                  efS, topk, c_void_p(d_idx), c_void_p(d_dist), c_void_p(d_count), out_stride, searchers, c_void_p(stream or 0))
        self._check()

    def debug_hnsw_counters(self, reset=False):
        """Counters of K17 since the last reset (``xrl_debug_hnsw_counters``), by name."""
        out = (c_uint64 * len(self.HNSW_COUNTERS))()
        self.clib_float32.xrl_debug_hnsw_counters(out, len(self.HNSW_COUNTERS), 1 if reset else 0)
        return dict(zip(self.HNSW_COUNTERS, (int(v) for v in out)))

    def debug_hnsw_caps(self):
        out = (c_uint64 * 4)()
        self.clib_float32.xrl_debug_hnsw_caps(out, 4)
        return dict(zip(("CAP", "cand_cap", "lds_degree", "max_slots"), (int(v) for v in out)))

    # ------------------------------------------------------------------ label clustering (K11)
    def run_clustering(self, py_feat_mat, train_params, codes=None):
        """Hierarchical 2-means of a label embedding on the device, with the reference's dispatch and return (base.py:1608-1646):
        ``py_feat_mat`` is a ScipyCsrF32 or ScipyDrmF32 view, ``train_params`` carries ``depth`` and the ClusteringParam fields;
        returns the leaf codes (``codes`` when it fits, else a new uint32 array).  The answer is the reference's at threads = 1."""
        clib = self.clib_float32
        if isinstance(py_feat_mat, ScipyCsrF32):
            run = clib.c_run_clustering_csr_f32
        elif isinstance(py_feat_mat, ScipyDrmF32):
            run = clib.c_run_clustering_drm_f32
        else:
            raise NotImplementedError("type(py_feat_mat) = {} is not implemented".format(type(py_feat_mat)))
        if codes is None or len(codes) != py_feat_mat.shape[0] or codes.dtype != np.uint32:
            codes = np.zeros(py_feat_mat.rows, dtype=np.uint32)
        run(byref(py_feat_mat), int(train_params.depth), byref(ClusteringParam(train_params)), codes.ctypes.data_as(POINTER(c_uint32)))
        self._check()
        return codes

    def run_clustering_device(self, smat_handle, depth, param, d_codes, d_scores=None, stream=None):
        """Cluster the rows of a matrix handle; ``d_codes`` (u32 [rows]) and ``d_scores`` (f32 [depth * rows] or None) are device addresses."""
        rc = self.clib_float32.xrl_run_clustering_device(c_void_p(smat_handle), int(depth), byref(param), c_void_p(d_codes), c_void_p(d_scores or 0),
                                                         c_void_p(stream or 0))
        self._check()
        return rc

    def debug_cluster_plan(self, rows, cols, nnz, depth, param):
        """The draws of a clustering, without a GPU: dict(node_seed [2^(depth+1)], level_info [depth, 2] = (sampled, first-touch),
        work [2^depth, 4] by node id = (start, working end, position of r, position of l), perm [depth, rows])."""
        node_seed = np.zeros(2 << depth, dtype=np.uint32); level_info = np.zeros((max(depth, 1), 2), dtype=np.uint32)
        work = np.zeros((1 << depth, 4), dtype=np.uint32); perm = np.zeros((max(depth, 1), rows), dtype=np.uint32)
        self.clib_float32.xrl_debug_cluster_plan(int(rows), int(cols), int(nnz), int(depth), byref(param), *(a.ctypes.data_as(c_void_p) for a in
                                                                                                         (node_seed, level_info, work, perm)))
        self._check()
        return dict(node_seed=node_seed, level_info=level_info[:depth], work=work, perm=perm[:depth])

    def debug_cluster_forms(self, depth=32):
        """Of the last clustering: dict(lane_runs, wave_runs, seg_sorts, switch_level (None: never), iters per level)."""
        out = (c_uint64 * (5 + depth))()
        self.clib_float32.xrl_debug_cluster_forms(out, 5 + depth)
        self._check()
        v = [int(x) for x in out]
        return dict(lane_runs=v[0], wave_runs=v[1], seg_sorts=v[2], switch_level=None if v[3] == 2**64 - 1 else v[3], iters=v[5:5 + min(v[4], depth)])

    # ------------------------------------------------------------------ device-resident path (additive)
    def queries_upload(self, c_model, X):
        lib = self.clib_float32
        X, fmt = self._x_view(X)
        h = getattr(lib, f"xrl_queries_upload_{fmt}")(c_void_p(c_model), byref(X))
        self._check()
        return h

    def queries_from_device_csr(self, c_model, rows, cols, row_ptr_addr, col_idx_addr, val_addr, nnz):
        """Wrap a CSR that already lives in HBM (raw device addresses: u64 row_ptr, u32 col_idx, f32 val); non-owning."""
        h = self.clib_float32.xrl_queries_from_device_csr(c_void_p(c_model), rows, cols, c_void_p(row_ptr_addr), c_void_p(col_idx_addr),
                                                          c_void_p(val_addr), nnz)
        self._check()
        return h

    def queries_from_device_drm(self, c_model, rows, cols, val_addr):
        h = self.clib_float32.xrl_queries_from_device_drm(c_void_p(c_model), rows, cols, c_void_p(val_addr))
        self._check()
        return h

    def queries_tfidf_device(self, c_model, rows, cols, row_ptr_addr, col_idx_addr, count_addr, nnz, idf_addr=None, binary=False,
                             sublinear_tf=False, norm_p=2, stream=None, out_addr=None):
        """Device CSR of term counts -> the reference's tf-idf weighting + normalisation on the device (tfidf.hpp:798-822);
        the handle references row_ptr / col_idx (keep them alive); the weighted values go to out_addr (nnz floats) or a buffer it owns."""
        h = self.clib_float32.xrl_queries_tfidf_device(c_void_p(c_model), rows, cols, c_void_p(row_ptr_addr), c_void_p(col_idx_addr),
                                                       c_void_p(count_addr), nnz, c_void_p(idf_addr or 0), 1 if binary else 0,
                                                       1 if sublinear_tf else 0, int(norm_p), c_void_p(out_addr or 0), c_void_p(stream or 0))
        self._check()
        return h

    def queries_concat_device(self, c_model, rows, sparse_cols, row_ptr_addr, col_idx_addr, val_addr, nnz, dense_cols, emb_addr, stream=None,
                              normalize_emb=False):
        """[X_feat (device CSR) | X_emb (device dense)] -> one device CSR (XR-Transformer concat_model's query form);
        normalize_emb: l2-normalise the rows of X_emb on the device first (the reference's default)."""
        h = self.clib_float32.xrl_queries_concat_device_ex(c_void_p(c_model), rows, sparse_cols, c_void_p(row_ptr_addr), c_void_p(col_idx_addr),
                                                           c_void_p(val_addr), nnz, dense_cols, c_void_p(emb_addr), 1 if normalize_emb else 0,
                                                           c_void_p(stream or 0))
        self._check()
        return h

    # ---- TF-IDF query producer (pecos/core/base.py:1696-1725, 1820-1862: tfidf_load / tfidf_destruct / tfidf_predict)
    def tfidf_load(self, load_dir):
        return self._checked(self.clib_float32.c_tfidf_load(c_char_p(load_dir.encode("utf-8"))))

    def tfidf_destruct(self, model):
        if self._lib is not None and model:
            self._lib.c_tfidf_destruct(c_void_p(model))

    @staticmethod
    def _corpus_joined(corpus):
        """(the documents of a non-empty list of str / bytes joined into ONE bytes object, their byte lengths u64[n]).  Per-document Python work
        is what bounds the producer once the native half runs at millions of documents a second, so an all-ASCII corpus is encoded in one
        go (byte length == len(str))."""
        nr_doc = len(corpus)
        if all(type(d) is str for d in corpus):
            joined = "".join(corpus)
            if joined.isascii():
                buf = joined.encode("ascii")
                lens = np.fromiter(map(len, corpus), dtype=np.uint64, count=nr_doc)
            else:
                enc = [d.encode("utf-8") for d in corpus]
                buf = b"".join(enc)
                lens = np.fromiter(map(len, enc), dtype=np.uint64, count=nr_doc)
        else:
            enc = [d.encode("utf-8") if isinstance(d, str) else bytes(d) for d in corpus]
            buf = b"".join(enc)
            lens = np.fromiter(map(len, enc), dtype=np.uint64, count=nr_doc)
        return buf, lens

    @classmethod
    def _corpus_arrays(cls, corpus):
        """(char** as a ctypes pointer, byte lengths u64[n], n) for a list of str / bytes: the joined buffer of :meth:`_corpus_joined`, the
        pointer table numpy arithmetic on its address."""
        nr_doc = len(corpus)
        if nr_doc == 0:
            return c_void_p(0), np.zeros(1, dtype=np.uint64), 0
        buf, lens = cls._corpus_joined(corpus)
        base = ctypes.cast(c_char_p(buf), c_void_p).value or 0
        ptrs = np.empty(nr_doc, dtype=np.uint64)
        ptrs[0] = base
        if nr_doc > 1:
            np.cumsum(lens[:-1], out=ptrs[1:]); ptrs[1:] += np.uint64(base)
        arr = ptrs.ctypes.data_as(c_void_p)
        arr._keep = (buf, ptrs)               # the table and the text live as long as the pointer object does
        return arr, lens, nr_doc

    @classmethod
    def corpus_packed(cls, corpus):
        """(bytes, offsets u64[n], byte lengths u64[n]) of a list of str / bytes: the device tokenizer's input form (documents back to back
        in the joined buffer ``_corpus_arrays`` points into)."""
        nr_doc = len(corpus)
        if nr_doc == 0:
            return b"", np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint64)
        buf, lens = cls._corpus_joined(corpus)
        off = np.zeros(nr_doc, dtype=np.uint64)
        if nr_doc > 1:
            np.cumsum(lens[:-1], out=off[1:])
        return buf, off, lens

    def tfidf_predict(self, model, corpus, buffer_size=0, threads=-1):
        """Vectorize a list of strings, or -- corpus given as a path -- the lines of a text file (pecos/core/base.py:1820-1863)."""
        pred_alloc = ScipyCompressedSparseAllocator()
        if isinstance(corpus, str):
            assert os.path.isfile(corpus), "Cannot predict from {}!".format(corpus)
            corpus_utf8 = corpus.encode("utf-8")
            self.clib_float32.c_tfidf_predict_from_file(c_void_p(model), ctypes.cast(c_char_p(corpus_utf8), c_void_p), len(corpus_utf8), buffer_size, threads, pred_alloc.cfunc)
            self._check()
            return pred_alloc.get()
        arr, lens, nr_doc = self._corpus_arrays(corpus)
        self.clib_float32.c_tfidf_predict(c_void_p(model), arr, lens.ctypes.data_as(POINTER(c_uint64)), nr_doc, threads, pred_alloc.cfunc)
        self._check()
        return pred_alloc.get()

    def tfidf_counts(self, model, corpus, threads=-1):
        """Host only: the CSR of term COUNTS (hstacked over an ensemble's base vectorizers) the device weighting starts from."""
        pred_alloc = ScipyCompressedSparseAllocator()
        arr, lens, nr_doc = self._corpus_arrays(corpus)
        self.clib_float32.xrl_tfidf_counts(c_void_p(model), arr, lens.ctypes.data_as(POINTER(c_uint64)), nr_doc, threads, pred_alloc.cfunc)
        self._check()
        return pred_alloc.get()

    def tfidf_nr_features(self, model):
        return self._checked(int(self.clib_float32.xrl_tfidf_nr_features(c_void_p(model))))

    TOKENIZERS = {"host": 0, "device": 1}

    def tfidf_predict_device(self, model, c_model, corpus, threads=-1, tokenizer="host"):
        """Texts -> tf-idf X that STAYS on c_model's device: a query handle for predict_device (free it with queries_free).
        tokenizer: "host" (host threads count, the counts are uploaded) or "device" (the text is uploaded, K9 counts)."""
        if tokenizer not in self.TOKENIZERS:
            raise ValueError(f"tokenizer={tokenizer!r}: expected 'host' or 'device'")
        arr, lens, nr_doc = self._corpus_arrays(corpus)
        if tokenizer == "host":
            h = self.clib_float32.xrl_tfidf_predict_device(c_void_p(model), c_void_p(c_model), arr, lens.ctypes.data_as(POINTER(c_uint64)), nr_doc, threads)
        else:
            h = self.clib_float32.xrl_tfidf_predict_device_tok(c_void_p(model), c_void_p(c_model), arr, lens.ctypes.data_as(POINTER(c_uint64)), nr_doc,
                                                              self.TOKENIZERS[tokenizer], threads)
        self._check()
        return h

    def tfidf_counts_device(self, model, c_model, text_addr, off_addr, len_addr, nr_doc, status_addr=None, stream=None):
        """Document bytes in HBM (raw device addresses: u8 text, u64 offsets, u64 lengths) -> the term-count CSR as a query handle (K9);
        ``status_addr`` (u32 [nr_doc]) takes the per-document status instead of an error."""
        return self._checked(self.clib_float32.xrl_tfidf_counts_device(c_void_p(model), c_void_p(c_model), c_void_p(text_addr), c_void_p(off_addr), c_void_p(len_addr), nr_doc,
                                                                       c_void_p(status_addr or 0), c_void_p(stream or 0)))

    def tfidf_predict_device_text(self, model, c_model, text_addr, off_addr, len_addr, nr_doc, stream=None):
        """Document bytes in HBM -> tf-idf X on c_model's device (K9 + the weighting tail): a query handle for predict_device."""
        return self._checked(self.clib_float32.xrl_tfidf_predict_device_text(c_void_p(model), c_void_p(c_model), c_void_p(text_addr), c_void_p(off_addr), c_void_p(len_addr), nr_doc,
                                                                             c_void_p(stream or 0)))

    def tfidf_device_bytes(self, model, device):
        return self._checked(int(self.clib_float32.xrl_tfidf_device_bytes(c_void_p(model), int(device))))

    def tfidf_device_forms(self, model):
        """Debug counters of the device tokenizer since the load: segments served by the LDS form, by the global form, batches, calls."""
        out = (c_uint64 * 4)()
        self.clib_float32.xrl_debug_tfidf_device_forms(c_void_p(model), out, 4)
        self._check()
        return dict(zip(("lds_segments", "global_segments", "batches", "calls"), (int(v) for v in out)))

    # ---- TF-IDF training on the device (K15; pecos/core/base.py:1706-1818: tfidf_save / tfidf_train)
    def tfidf_train(self, trn_corpus, config=None):
        """Train a vectorizer on a list of str / bytes: the reference's ``corelib.tfidf_train`` with the corpus uploaded once and every
        pass over it on the device.  ``config``: one base config or {"base_vect_configs": [...], "norm_p": ...}, with the reference's
        aliases (:class:`TfidfBaseVectorizerParam`).  Returns the handle ``tfidf_load`` returns."""
        if isinstance(trn_corpus, str):
            raise NotImplementedError(f"tfidf_train from a corpus file or folder ({trn_corpus!r}) is not offered by pecos_amd: read the lines and pass a list")
        config = {} if config is None else config
        params = TfidfVectorizerParam.from_config(config)
        arr, lens, nr_doc = self._corpus_arrays(trn_corpus)
        return self._checked(self.clib_float32.xrl_tfidf_train(arr, lens.ctypes.data_as(POINTER(c_uint64)), nr_doc, byref(params), int(config.get("threads", -1))))

    def tfidf_train_device(self, device, text_addr, off_addr, len_addr, nr_doc, config, stream=None):
        """The resident form: document bytes, offsets and lengths in HBM on ``device`` (raw addresses, as for ``tfidf_counts_device``)."""
        params = TfidfVectorizerParam.from_config(config)
        return self._checked(self.clib_float32.xrl_tfidf_train_device(int(device), c_void_p(text_addr), c_void_p(off_addr), c_void_p(len_addr), nr_doc, byref(params), c_void_p(stream or 0)))

    def tfidf_save(self, model, save_dir):
        """The reference's folder layout (``c_tfidf_save``) of a trained or loaded vectorizer handle."""
        self.clib_float32.xrl_tfidf_save(c_void_p(model), c_char_p(save_dir.encode("utf-8")))
        self._check()

    def tfidf_transform_device(self, model, device, text_addr, off_addr, len_addr, nr_doc, status_addr=None, stream=None):
        """Document bytes in HBM -> the weighted X as a matrix handle on ``device`` (K9 + the weighting tail); needs no XR-Linear model."""
        return self._checked(self.clib_float32.xrl_tfidf_transform_device(c_void_p(model), int(device), c_void_p(text_addr), c_void_p(off_addr), c_void_p(len_addr), nr_doc,
                                                                          c_void_p(status_addr or 0), c_void_p(stream or 0)))

    def tfidf_export(self, model, base=0):
        """The content of one base vectorizer: ({token bytes: id}, {tuple of token ids: feature id}, idf float32 [nr_features])."""
        sizes = (c_uint64 * 5)()
        null = c_void_p(0)
        self.clib_float32.xrl_tfidf_export(c_void_p(model), base, sizes, null, null, null, null, null, null, null)
        self._check()
        nt, nbytes, ng, nflat, nidf = (int(v) for v in sizes)
        tok_bytes, tok_off, tok_ids = np.zeros(max(nbytes, 1), np.uint8), np.zeros(nt + 1, np.uint64), np.zeros(max(nt, 1), np.int32)
        ng_flat, ng_off, ng_ids, idf = np.zeros(max(nflat, 1), np.int32), np.zeros(ng + 1, np.uint64), np.zeros(max(ng, 1), np.uint32), np.zeros(max(nidf, 1), np.float32)
        self.clib_float32.xrl_tfidf_export(c_void_p(model), base, sizes, *(c_void_p(a.ctypes.data) for a in (tok_bytes, tok_off, tok_ids, ng_flat, ng_off, ng_ids, idf)))
        self._check()
        raw = tok_bytes.tobytes()
        vocab = {raw[int(tok_off[i]):int(tok_off[i + 1])]: int(tok_ids[i]) for i in range(nt)}
        ngrams = {tuple(int(t) for t in ng_flat[int(ng_off[i]):int(ng_off[i + 1])]): int(ng_ids[i]) for i in range(ng)}
        return vocab, ngrams, idf[:nidf].copy()

    def tfidf_train_forms(self, model):
        """Debug counters of the training that made this handle (zeros for a loaded one)."""
        out = (c_uint64 * 11)()
        self.clib_float32.xrl_debug_tfidf_train_forms(c_void_p(model), out, 11)
        self._check()
        return dict(zip(("vocab_docs", "df_lds_segments", "df_global_segments", "batches", "distinct_tokens", "distinct_ngrams", "long_compares", "table_grows",
                         "us_vocab", "us_df", "us_order"),
                        (int(v) for v in out)))

    def queries_concat_handle(self, c_model, queries, dense_cols, emb_addr, normalize_emb=False, stream=None):
        h = self.clib_float32.xrl_queries_concat_handle(c_void_p(c_model), c_void_p(queries), dense_cols, c_void_p(emb_addr), 1 if normalize_emb else 0, c_void_p(stream or 0))
        self._check()
        return h

    def queries_download(self, h):
        """Copy of a query handle's matrix back to the host (scipy CSR with the stored order, or ndarray)."""
        info = (ctypes.c_uint64 * 4)()
        self.clib_float32.xrl_queries_info(c_void_p(h), info); self._check()
        rows, cols, nnz, dense = (int(v) for v in info)
        dl = self.clib_float32.xrl_queries_download
        if dense:
            out = np.zeros((rows, cols), dtype=np.float32)
            dl(c_void_p(h), None, None, out.ctypes.data_as(c_void_p)); self._check()
            return out
        return self._download_csr(dl, h, rows, cols, nnz)

    def queries_free(self, h):
        if self._lib is not None and h:
            self._lib.xrl_queries_free(c_void_p(h))

    def predict_device(self, c_model, queries, beam_size, post_processor, only_topk, d_idx, d_val, d_cnt, out_stride,
                       stream=None, sync=True):
        """``d_*`` are raw device addresses (e.g. ``tensor.data_ptr()``)."""
        rc = self.clib_float32.xrl_predict_device(
            c_void_p(c_model), c_void_p(queries), beam_size or 0,
            self._cstr(post_processor), only_topk or 0,
            c_void_p(d_idx), c_void_p(d_val), c_void_p(d_cnt), out_stride, c_void_p(stream or 0), 1 if sync else 0)
        self._check()
        return rc

    def predict_device_rows(self, c_model, queries, beam_size, post_processor, only_topk, d_idx, d_val, d_cnt, out_stride,
                            row_begin, row_count, stream=None, sync=True):
        """predict_device for rows [row_begin, row_begin + row_count) only; results land at the same rows of the output buffers."""
        rc = self.clib_float32.xrl_predict_device_rows(
            c_void_p(c_model), c_void_p(queries), beam_size or 0,
            self._cstr(post_processor), only_topk or 0,
            c_void_p(d_idx), c_void_p(d_val), c_void_p(d_cnt), out_stride, c_void_p(stream or 0), 1 if sync else 0,
            int(row_begin), int(row_count))
        self._check()
        return rc

    def predict_selected_device(self, c_model, queries, post_processor, d_sel_idx, d_sel_cnt, sel_stride, d_idx, d_val, d_cnt, out_stride,
                                d_status=None, stream=None, sync=True):
        """K7 + K4: the scores of a given set of labels per query row (``d_sel_idx`` u32 [rows, sel_stride], ``d_sel_cnt`` u32 [rows] or None --
        raw device addresses, the form ``predict_device`` writes) in the reference's order for that set, into ``d_idx`` / ``d_val`` /
        ``d_cnt`` (row stride ``out_stride`` >= ``sel_stride``).  ``d_status``: optional device u32[2] that receives {code, row} of the lowest
        bad row.  ``sync=True`` raises RuntimeError with the host path's message on a bad row; ``sync=False`` returns without synchronising.
        Returns the library's return code."""
        rc = self.clib_float32.xrl_predict_selected_device(
            c_void_p(c_model), c_void_p(queries), self._cstr(post_processor),
            c_void_p(d_sel_idx), c_void_p(d_sel_cnt or 0), int(sel_stride), c_void_p(d_idx), c_void_p(d_val), c_void_p(d_cnt), int(out_stride),
            c_void_p(d_status or 0), c_void_p(stream or 0), 1 if sync else 0)
        self._check()
        return rc

    ENSEMBLE_MODES = {"average": 0, "finish": 1, "rank_average": 2}
    # xrl_ensemble_methods_device's numbers (finish is listed for its number only: that entry point refuses it)
    ENSEMBLE_METHODS = {"average": 0, "finish": 1, "rank_average": 2, "sigmoid_average": 3, "softmax_average": 4, "round_robin": 5}

    def _ensemble_call(self, fn, device, rows, d_idx, d_val, d_cnt, in_stride, middle, d_out_idx, d_out_val, d_out_cnt, out_stride, stream, sync):
        """The pointer tables and the call of either ensemble entry point; ``middle``: its arguments between the strides and the outputs."""
        n = len(d_idx)
        assert len(d_val) == n and len(d_cnt) == n and len(in_stride) == n
        tab = lambda a: (c_void_p * max(n, 1))(*[c_void_p(int(x) if x else 0) for x in a])                   # noqa: E731
        rc = fn(int(device), n, int(rows), tab(d_idx), tab(d_val), tab(d_cnt), (c_uint32 * max(n, 1))(*[int(s) for s in in_stride]), *middle,
                c_void_p(d_out_idx), c_void_p(d_out_val), c_void_p(d_out_cnt), int(out_stride), c_void_p(stream or 0), 1 if sync else 0)
        self._check()
        return rc

    def ensemble_device(self, device, rows, d_idx, d_val, d_cnt, in_stride, mode, threshold, only_topk, d_out_idx, d_out_val, d_out_cnt,
                        out_stride, stream=None, sync=True):
        """K6: merge the fixed-stride results of ``len(d_idx)`` models (lists of raw device addresses, one per model, and their row
        strides) into one, on the device.  ``mode``: a key of ``ENSEMBLE_MODES`` or its number; ``threshold`` / ``only_topk``: mode
        ``finish`` only, ``None`` = none."""
        middle = (self.ENSEMBLE_MODES.get(mode, mode), None if threshold is None else ctypes.byref(c_float(threshold)), only_topk or 0)
        return self._ensemble_call(self.clib_float32.xrl_ensemble_device, device, rows, d_idx, d_val, d_cnt, in_stride, middle,
                                   d_out_idx, d_out_val, d_out_cnt, out_stride, stream, sync)

    def ensemble_methods_device(self, device, rows, d_idx, d_val, d_cnt, in_stride, method, only_topk, d_out_idx, d_out_val, d_out_cnt,
                                out_stride, stream=None, sync=True):
        """K6: like :meth:`ensemble_device` for the methods of ``CsrEnsembler`` -- ``method``: a key of ``ENSEMBLE_METHODS`` (not
        ``finish``) or its number; ``only_topk``: ``None`` / 0 = the method's own rows, else they are ranked again by their fp32 value and
        cut, as ``TransformerMatcher.ensemble_prediction`` does."""
        middle = (self.ENSEMBLE_METHODS.get(method, method), only_topk or 0)
        return self._ensemble_call(self.clib_float32.xrl_ensemble_methods_device, device, rows, d_idx, d_val, d_cnt, in_stride, middle,
                                   d_out_idx, d_out_val, d_out_cnt, out_stride, stream, sync)

    METRICS_MAX = 1024          # capacity of K8 (xrl_metrics_device): entries per result row, and positions

    def metrics_device(self, device, rows, d_idx, d_val, d_cnt, stride, d_true_ptr, d_true_idx, topk, d_matched, d_recall_sum,
                       stream=None, sync=True):
        """K8: the sums behind precision / recall at 1 .. ``topk`` of one fixed-stride result (raw device addresses, row stride ``stride``)
        against the true labels as a device CSR pattern (``d_true_ptr`` u64 [rows+1], ``d_true_idx`` u32), into ``d_matched`` u64 [topk] and
        ``d_recall_sum`` f64 [topk].  A stride or topk outside 1..1024 raises ValueError with the library's message."""
        rc = self.clib_float32.xrl_metrics_device(
            int(device), int(rows), c_void_p(d_idx), c_void_p(d_val), c_void_p(d_cnt), int(stride), c_void_p(d_true_ptr), c_void_p(d_true_idx),
            int(topk), c_void_p(d_matched), c_void_p(d_recall_sum), c_void_p(stream or 0), 1 if sync else 0)
        try:
            self._check()
        except RuntimeError as e:
            if " must be 1.." in str(e):
                raise ValueError(str(e)) from None
            raise
        return rc

    # ------------------------------------------------------------------ output constraint (xmc/base.py:1796-1824, on the device)
    def set_output_constraint(self, c_model, labels):
        """Restrict the handle's beam search to ``labels`` (a contiguous uint32 numpy array on the host); a set that covers every label clears."""
        labels = np.ascontiguousarray(labels, dtype=np.uint32)
        rc = self.clib_float32.xrl_set_output_constraint(c_void_p(c_model), c_void_p(labels.ctypes.data), int(labels.size))
        self._check()
        return rc

    def set_output_constraint_device(self, c_model, d_labels, n, stream=None):
        """... from ``n`` uint32 label ids in HBM on the handle's device (raw address), read on ``stream`` (None: the handle's)."""
        rc = self.clib_float32.xrl_set_output_constraint_device(c_void_p(c_model), c_void_p(d_labels), int(n), c_void_p(stream or 0))
        self._check()
        return rc

    def clear_output_constraint(self, c_model):
        rc = self.clib_float32.xrl_clear_output_constraint(c_void_p(c_model))
        self._check()
        return rc

    def output_constraint_info(self, c_model):
        """(active, [kept children of every layer, top-down])."""
        depth = self.xlinear_get_int_attr(c_model, "depth")
        out = (c_uint64 * (1 + depth))()
        self.clib_float32.xrl_output_constraint_info(c_void_p(c_model), out, 1 + depth)
        self._check()
        return bool(out[0]), [int(out[1 + l]) for l in range(depth)]

    def debug_output_constraint_view(self, c_model, layer, n_parents, kept):
        """Tests: (chunk_col', perm_inv') of one layer's constrained view, or None when the layer runs on its own arrays."""
        cc = np.zeros(n_parents + 1, dtype=np.uint32)
        pi = np.zeros(max(1, kept), dtype=np.uint32)
        rc = self.clib_float32.xrl_debug_output_constraint_view(c_void_p(c_model), int(layer), c_void_p(cc.ctypes.data), cc.size,
                                                                c_void_p(pi.ctypes.data), int(kept))
        self._check()
        return (cc, pi[:kept]) if rc == 1 else None

    def effective_topk(self, c_model, only_topk):
        return int(self.clib_float32.xrl_effective_topk(c_void_p(c_model), only_topk or 0))

    def debug_split_chunk(self, col_nnz, limit):
        """Host-only: number of even column tiles the model compiler cuts a chunk with these column nnz into."""
        cum = np.concatenate([[0], np.cumsum(np.asarray(col_nnz, dtype=np.uint64))]).astype(np.uint64)
        fn = self.clib_float32.xrl_debug_split_chunk
        return int(fn(cum.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), len(col_nnz), int(limit)))

    def debug_layout_rows(self, row_len, align=True):
        """Host-only: (offset, length) of every tile row and the padded entry count, as the model compiler places them."""
        rptr = np.concatenate([[0], np.cumsum(np.asarray(row_len, dtype=np.int64))]).astype(np.uint32)
        ext = np.zeros(len(row_len), dtype=np.uint32)
        fn = self.clib_float32.xrl_debug_layout_rows
        total = int(fn(rptr.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), len(row_len), 1 if align else 0,
                       ext.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))))
        self._check()
        return ext & 0x1FFFFFF, (ext >> 25) + 1, total

    def debug_host_batches(self, indptr, rows, cols, host_batch_mb=12):
        """Host-only: row-batch boundaries of the pipelined host ABI for a CSR X with this row pointer (``None``: dense rows x cols)."""
        ptr = None if indptr is None else np.ascontiguousarray(indptr, dtype=np.uint64)
        fn = self.clib_float32.xrl_debug_host_batches
        rb = np.zeros(34, dtype=np.uint32)          # at most 32 batches
        n = int(fn(None if ptr is None else ptr.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), int(rows), int(cols), int(host_batch_mb),
                   rb.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), len(rb)))
        self._check()
        return rb[:n].copy()

    K2_FORMS = ("wave", "list", "reg", "lds", "big")

    def debug_k2_form(self, k, cand_stride, k2_big_min_k=0, stage=0, limited_cands=0):
        """Host-only: (form, NS) of the per-query top-k launch for a layer that keeps ``k`` of ``cand_stride`` candidates -- a name of
        ``K2_FORMS`` and the candidate registers per lane of the wave / list form (0 otherwise).  ``stage``: 0 = whole row, 1 = a stage of the
        bound pruning (``limited_cands``: what a rank-limited stage looks at), 2 = its last stage on the list of unfinished queries."""
        ns = c_uint32(0)
        f = int(self.clib_float32.xrl_debug_k2_form(int(k), int(cand_stride), int(k2_big_min_k), int(stage), int(limited_cands), byref(ns)))
        self._check()
        return self.K2_FORMS[f], int(ns.value)

    def profile_enable(self, c_model, on=True):
        self.clib_float32.xrl_profile_enable(c_void_p(c_model), 1 if on else 0)

    def profile_reset(self, c_model):
        self.clib_float32.xrl_profile_reset(c_void_p(c_model))

    def profile_get(self, c_model):
        n = self.clib_float32.xrl_profile_get(c_void_p(c_model), None, 0)
        arr = (ProfileRec * max(1, n))()
        n = self.clib_float32.xrl_profile_get(c_void_p(c_model), arr, n)
        return [dict(name=arr[i].name.decode(), layer=arr[i].layer, launches=arr[i].launches, ms=arr[i].ms)
                for i in range(n)]

    def predict_stats(self, c_model, queries, beam_size, post_processor, only_topk):
        """Untimed predict (tile-format kernels) returning per layer a dict of work counters: ref_chunk_bytes (SURVEY.md 8d:
        every active reference chunk streamed whole), candidates, items, probes, hit_rows, hit_entries, item_cols, x_cols."""
        depth = self.xlinear_get_int_attr(c_model, "depth")
        out = (c_double * (8 * depth))()
        self.clib_float32.xrl_predict_stats(c_void_p(c_model), c_void_p(queries), beam_size or 0,
                                            self._cstr(post_processor), only_topk or 0, out, 8 * depth)
        self._check()
        keys = ("ref_chunk_bytes", "candidates", "items", "probes", "hit_rows", "hit_entries", "item_cols", "x_cols")
        return [dict(zip(keys, [out[8 * l + i] for i in range(8)])) for l in range(depth)]

    def set_option(self, c_model, key, value):
        self.clib_float32.xrl_set_option(c_void_p(c_model), key.encode("utf-8"), int(value))
        self._check()

    def debug_k1_phases(self, reset=True):
        out = (c_uint64 * 8)()
        self.clib_float32.xrl_debug_k1_phases(out, 1 if reset else 0)
        self._check()
        return [int(v) for v in out]

    def single_layer_cache_clear(self):
        """Drop every cached single-layer handle (call after modifying W / C in place)."""
        self.clib_float32.xrl_single_layer_cache_clear()

    def single_layer_cache_stats(self):
        h, m, e = c_uint64(0), c_uint64(0), c_uint64(0)
        self.clib_float32.xrl_single_layer_cache_stats(byref(h), byref(m), byref(e))
        return dict(hits=int(h.value), misses=int(m.value), entries=int(e.value))

    def layer_info(self, c_model, layer):
        out = (c_uint64 * 12)()
        self.clib_float32.xrl_layer_info(c_void_p(c_model), layer, out, 12)
        self._check()
        keys = ("lookup", "bucket_levels", "dense", "dense_tile_width", "dense_ld", "tiles", "entries", "dense_bytes", "w_rows",
                "children", "max_tile_cols", "device_bytes")
        return dict(zip(keys, [int(v) for v in out]))

    def model_device_bytes(self, c_model):
        return int(self.clib_float32.xrl_model_device_bytes(c_void_p(c_model)))


clib = corelib()
