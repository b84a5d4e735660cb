"""MI355X-native node2vec2rank fit-and-rank engine (HIP on gfx950 behind a C-ABI).

Public surface mirrors the reference package for the fit-and-rank path:
``node2vec2rank_amd.model.N2V2R`` (reference ``node2vec2rank/model.py``),
``node2vec2rank_amd.model_utils`` (reference ``node2vec2rank/model_utils.py``),
``node2vec2rank_amd.spectral.UASE`` (the ``spectral_embedding.UASE`` seam).
``node2vec2rank_amd.Coexpression`` has no reference counterpart: a graph layer given by its
expression matrix, whose co-expression network the engine builds on the GPU;
``node2vec2rank_amd.pick_soft_threshold`` chooses its power (WGCNA's ``pickSoftThreshold``) from
connectivities the GPU sums without building the network.
"""
from .coexpression import Coexpression
from .soft_threshold import pick_soft_threshold, scale_free_fit

__version__ = "0.1.0"
__all__ = ["Coexpression", "pick_soft_threshold", "scale_free_fit"]
