"""pyhgt_amd -- MI355X (gfx950) native forward pass of pyHGT's HGTConv.

Drop-in for the reference layers pyHGT/conv.py::HGTConv / DenseHGTConv (same constructor, parameter
names, forward signature) backed by hand-written HIP kernels behind a C ABI (include/hgt_hip.h).
"""
from .conv import HGTConv, DenseHGTConv, GeneralConv, RelTemporalEncoding, GraphPlan, install_into  # noqa: F401
from .model import GNN, Classifier, Matcher  # noqa: F401
from .autograd import set_deterministic, set_recompute  # noqa: F401
from .sampler import (DeviceHeteroGraph, sample_subgraph_device, sample_subgraph_host, sample_subgraphs_device,  # noqa: F401
                      sample_subgraphs_host)
from .sampler import LabelSpace, seed_edge_mask, np_label_distribution, np_label_index, np_label_counts, np_label_columns  # noqa: F401
from .sampler import candidate_pairs  # noqa: F401
from .metrics import Segments, rank_metrics, pair_rank_loss, class_loss, np_rank_metrics, np_pair_rank_loss, np_class_loss  # noqa: F401
from .metrics import class_predict, VoteTable, np_class_predict, np_vote_add  # noqa: F401
from .metrics import np_matcher_scores, np_matcher_topk, np_matcher_rank, matcher_scale, matcher_topk, matcher_rank  # noqa: F401
from .optim import AdamW, np_adamw_step  # noqa: F401
from .graph_build import np_edge_lists_to_csr, neighbour_mean, np_neighbour_mean  # noqa: F401
from .trim import np_trim_to_seeds, np_trim_graph, trim_to_seeds, TrimmedGraph  # noqa: F401
from .view import np_whole_graph, label_edge_flags  # noqa: F401
from .neighbourhood import np_neighbourhood, NeighbourhoodGraph, NeighbourhoodArrays  # noqa: F401

__all__ = ["HGTConv", "DenseHGTConv", "GeneralConv", "RelTemporalEncoding", "GraphPlan", "install_into", "GNN", "Classifier", "Matcher",
           "set_deterministic", "set_recompute", "DeviceHeteroGraph", "sample_subgraph_device", "sample_subgraph_host", "sample_subgraphs_device",
           "sample_subgraphs_host"]
