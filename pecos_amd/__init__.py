"""pecos_amd -- MI355X-native XR-Linear batch inference (drop-in for the predict path of amzn/pecos).

Only what the hot path needs lives here: ``csrc/`` (HIP kernels + C ABI), :mod:`pecos_amd.core`
(the ctypes binding that mirrors ``pecos.core.clib``), :mod:`pecos_amd.xlinear` (the
``XLinearModel`` surface) and :mod:`pecos_amd.distributed` (query sharding + RCCL all-gather).
"""
from .core import clib  # noqa: F401
from .features import DeviceMatrix, Metrics, metrics_device, metrics_sums_device, result_to_csr_device, sparse_matmul_device  # noqa: F401
from .features import Preprocessor, Tfidf, tfidf_train_device, tfidf_transform_device  # noqa: F401
from .indexer import HierarchicalKMeans, LabelEmbeddingFactory, label_embedding_device, run_clustering_device  # noqa: F401
from .cluster_chain import ClusterChain  # noqa: F401
from .training import matching_chain_device, relevance_chain_device, single_layer_predict_device, train_chain_device, train_layer_device  # noqa: F401
from .ann import HNSW, HNSWProductQuantizer4Bits, PairwiseANN, hnsw_predict_device  # noqa: F401
from .xlinear import HierarchicalMLModel, MLModel, MLProblem, XLinearModel  # noqa: F401

__all__ = ["clib", "XLinearModel", "HierarchicalMLModel", "MLModel", "MLProblem", "Metrics", "metrics_device", "metrics_sums_device",
           "DeviceMatrix", "sparse_matmul_device", "result_to_csr_device", "HierarchicalKMeans", "run_clustering_device",
           "LabelEmbeddingFactory", "label_embedding_device", "train_layer_device", "train_chain_device",
           "single_layer_predict_device", "ClusterChain", "relevance_chain_device", "matching_chain_device", "Tfidf", "Preprocessor", "tfidf_train_device", "tfidf_transform_device",
           "HNSW", "PairwiseANN", "HNSWProductQuantizer4Bits", "hnsw_predict_device"]
