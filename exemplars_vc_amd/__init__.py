"""exemplars_vc_amd - MI355X-native exemplar-NMF activation solver.

One hot path of entn-at/exemplars_vc, rebuilt for gfx950: given a fixed parallel exemplar
dictionary (A source, B target) and non-negative source frames X, run the Frobenius
multiplicative update  H <- H (.) A^T X (/) (A^T A H + eps)  and synthesise Y = B H.
Hand-written HIP kernels behind a C ABI (include/evc.h); this package is the host-side
mirror of the reference's three Python call surfaces (see `compat`).
"""
from .solver import (PreparedDictionary, cached_dictionary, compact_dictionary, convert, dtw_align, dtw_dictionary, frame_residuals, griffin_lim,
                     griffin_lim_batch, learn_dictionary, learn_dictionary_beta, learn_dictionary_cd, learn_dictionary_online, mfcc, mfcc_batch, prepare_dictionary, release_workspaces, require_device, solve_activations, solve_activations_beta, solve_activations_cd, stft, transform_online,
                     synthesize, workspace_bytes, solve_activations_deconv, synthesize_deconv, convert_deconv, multiframe_dictionary, learn_dictionary_deconv,
                     compact_dictionary_deconv, solve_activations_semi, convert_semi, solve_activations_prox, convert_prox,
                     learn_dictionary_sparse, compact_dictionary_sparse, learn_dictionary_convex, compact_dictionary_convex, solve_activations_masked,
                     convert_masked, learn_dictionary_masked, learn_dictionary_stochastic, kmeans, vq, compact_dictionary_kmeans)
from . import compat, shard  # noqa: F401

__all__ = ["prepare_dictionary", "cached_dictionary", "PreparedDictionary", "solve_activations", "solve_activations_cd", "solve_activations_beta", "learn_dictionary", "learn_dictionary_beta", "learn_dictionary_cd", "learn_dictionary_online", "transform_online", "solve_activations_deconv", "synthesize_deconv", "convert_deconv", "multiframe_dictionary", "learn_dictionary_deconv", "compact_dictionary_deconv", "solve_activations_semi", "convert_semi", "solve_activations_prox", "convert_prox", "solve_activations_masked", "convert_masked", "learn_dictionary_masked", "learn_dictionary_stochastic", "learn_dictionary_sparse", "compact_dictionary_sparse", "learn_dictionary_convex", "compact_dictionary_convex", "kmeans", "vq", "compact_dictionary_kmeans", "compact_dictionary", "convert", "synthesize", "griffin_lim", "griffin_lim_batch", "stft", "mfcc", "mfcc_batch", "dtw_align", "dtw_dictionary", "frame_residuals", "workspace_bytes",
           "require_device", "release_workspaces", "compat", "shard"]
__version__ = "0.1.0"
