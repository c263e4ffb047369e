"""``ClusterChain`` (pecos/utils/cluster_util.py): a hierarchical clustering as a list of CSC matrices, root first, with the reference's
folder layout and its two chain generators -- the relevance chain of cost-sensitive training and the matching chain of user-supplied
negatives -- computed on the device through :func:`pecos_amd.training.relevance_chain_device` and ``matching_chain_device``."""
import json
import os

import numpy as np
import scipy.sparse as smat

from .indexer import chain_from_partial


class ClusterChain(object):
    """A list of float32 CSC matrices that form a hierarchical clustering chain: ``chain[i].shape[0] == chain[i + 1].shape[1]``."""

    def __init__(self, chain):
        if isinstance(chain, type(self)):
            chain = chain.chain
        elif smat.issparse(chain):
            chain = [chain.tocsc()]
        assert isinstance(chain, list), "clustering chain shall be a list of CSC matrices"
        for i in range(len(chain) - 1):
            assert chain[i].shape[0] == chain[i + 1].shape[1], "matrices do not form a valid hierarchical clustering chain"
        self.chain = chain

    def __delitem__(self, key):
        del self.chain[key]

    def __getitem__(self, key):
        return self.chain[key]

    def __setitem__(self, key, val):
        self.chain[key] = val

    def __iter__(self):
        return iter(self.chain)

    def __len__(self):
        return len(self.chain)

    def __eq__(self, other):
        if len(self) != len(other):
            return False
        return all(A.shape == B.shape and (A != B).nnz == 0 for A, B in zip(self, other))

    def save(self, folder):
        """``folder/config.json`` ({"len": n}) and ``folder/C{i}.npz``, the reference's layout."""
        os.makedirs(folder, exist_ok=True)
        with open(os.path.join(folder, "config.json"), "w", encoding="utf-8") as fout:
            fout.write(json.dumps({"len": len(self)}))
        for i, C in enumerate(self):
            smat.save_npz(os.path.join(folder, f"C{i}.npz"), C, compressed=False)

    @classmethod
    def load(cls, path_to_cluster):
        """A folder written by :meth:`save` (here or by the reference), or one ``.npz`` matrix: the bottom level, completed upwards."""
        if os.path.isfile(path_to_cluster):
            return cls.from_partial_chain(smat.load_npz(path_to_cluster))
        config_path = os.path.join(path_to_cluster, "config.json")
        if not os.path.exists(config_path):
            raise ValueError(f"Cluster config file, {config_path}, does not exist")
        with open(config_path, "r", encoding="utf-8") as fin:
            length = json.loads(fin.read()).get("len", None)
        if length is None:
            raise ValueError(f'Cluster config file, {config_path}, does not have "len" parameter')
        return cls([smat.load_npz(os.path.join(path_to_cluster, f"C{i}.npz")).tocsc().astype(np.float32) for i in range(length)])

    @classmethod
    def from_partial_chain(cls, C, min_codes=None, nr_splits=16):
        """The bottom level(s) ``C`` (one sparse matrix, or a list, root first) completed upwards with all-one levels of out-degree
        ``nr_splits`` until a level has at most ``min_codes`` codes, under a single root (:func:`pecos_amd.indexer.chain_from_partial`)."""
        if smat.issparse(C):
            top, rest = C, []
        else:
            assert isinstance(C, (cls, list, tuple))
            levels = list(C)
            top, rest = levels[0], [smat.csc_matrix(c, dtype=np.float32) for c in levels[1:]]
        return cls(chain_from_partial(top, min_codes=min_codes, nr_splits=nr_splits) + rest)

    def matrix_chain_dimension_check(self, M_dict):
        """The reference's checks of a partial chain keyed by layers above the leaves; ``(nr_insts, nr_labels)``.  A failed check is a
        ``ValueError`` (the reference asserts)."""
        def need(ok, msg):
            if not ok:
                raise ValueError(msg)
        need(isinstance(M_dict, dict), "M_dict must be a dict")
        nr_labels = self.chain[-1].shape[0]
        need(set(M_dict.keys()) <= set(range(len(self) + 1)), "M_dict got invalid key")
        nr_insts = [v.shape[0] for v in M_dict.values() if v is not None]
        need(len(nr_insts) > 0 and nr_insts.count(nr_insts[0]) == len(nr_insts), "M_dict first dim do not match")
        if M_dict.get(0, None) is not None:
            need(M_dict[0].shape[1] == nr_labels, f"0: {tuple(M_dict[0].shape)}!={self.chain[-1].shape}")
        for i in range(1, len(self) + 1):
            if M_dict.get(i, None) is not None:
                need(M_dict[i].shape[1] == self.chain[-i].shape[1], f"{i}: {tuple(M_dict[i].shape)}!={self.chain[-i].shape}")
        return nr_insts[0], nr_labels

    def generate_matching_chain(self, M_dict):
        """The matching chain of user-supplied negatives (cluster_util.py:206-238) as a list of scipy CSC matrices of ones (None where
        nothing is given), computed on the device."""
        from .training import matching_chain_device
        return [None if m is None else smat.csc_matrix(m.download()) for m in matching_chain_device(M_dict, self)]

    def generate_relevance_chain(self, R_dict, norm_type=None, induce=True):
        """The relevance chain of cost-sensitive training (cluster_util.py:240-281) as a list of scipy matrices (CSR, as the reference's
        normalised ones; None where a level has none), computed on the device."""
        from .training import relevance_chain_device
        return [None if r is None else r.download() for r in relevance_chain_device(R_dict, self, norm_type, induce)]
