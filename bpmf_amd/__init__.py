"""bpmf_amd -- MI355X-native drop-in for the per-column Gibbs sampler of ExaScience/bpmf.

The compute path is libbpmf_hip.so (hand-written HIP for gfx950 behind the C ABI
of include/bpmf_hip.h); this package is the thin host-side mirror of the
reference's `struct Sys` interface (c++/bpmf.h:112-239) on top of it.  There is
no CPU fallback: without the library and a HIP device the sampler raises.
"""
from ._lib import load_library, library_path, BpmfHipError  # noqa: F401
from .engine import HipEngine, auc, hyper_sample, link_lambda_sample  # noqa: F401
from .sys import Sys, HyperParams, gibbs, fold_in  # noqa: F401
from .censor import censor_flags  # noqa: F401
from .weights import rating_weights  # noqa: F401
from .rank import held_out_lists, rank_metrics  # noqa: F401
from .io import read_tns, write_tns  # noqa: F401
from .tensor import tensor_gibbs  # noqa: F401
from .model import pool_models, run_chains, save_model, load_model, predict_cells, read_model, write_model, diagnose, diag_summary, score_cells, score_summary, score_compare, predict_intervals, calibration_summary, loo_cells, loo_summary  # noqa: F401

__all__ = ["load_library", "library_path", "BpmfHipError", "HipEngine", "auc", "hyper_sample", "Sys", "HyperParams", "gibbs", "fold_in", "censor_flags", "rating_weights", "held_out_lists", "rank_metrics", "read_tns", "write_tns", "tensor_gibbs"]
