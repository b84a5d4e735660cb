"""ctypes binding of libn2v2r_hip.so (the C-ABI in include/n2v2r.h).

There is no CPU fallback: if the library is missing, or no GPU is visible, every entry point
raises.  Status codes map onto the exception types the reference raises for the same
conditions (model_utils.py:64-65, model.py:182-183, model.py:199).
"""
from __future__ import annotations

import atexit
import ctypes
import os
import threading
import warnings
import weakref

import numpy as np

from .coexpression import KINDS, METHODS, Coexpression, method_name

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("N2V2R_LIB", os.path.join(_HERE, "lib", "libn2v2r_hip.so"))

OK = 0
ERR_BAD_ARG = 1
ERR_UNSUPPORTED_METRIC = 2
ERR_NO_CONVERGENCE = 3
ERR_HIP = 4
ERR_OUT_OF_MEMORY = 5
ERR_NOT_READY = 6
ERR_UNSUPPORTED_AGG = 7
ERR_INTERNAL = 8
ERR_RCCL = 9
AGG_BORDA, AGG_NONE = 0, -1
EIG_TIME_SPMM = 16
EIG_TEST_NO_STAGNATION = 64
EIG_TEST_FAIL_ALONE = 128

STRATEGY = {"sequential": 0, "one_vs_before": 1, "one_vs_rest": 2}
METRIC = {"cosine": 0, "euclidean": 1, "correlation": 2}
SYM_DETECT, SYM_NO, SYM_YES = -1, 0, 1

# every symbol include/n2v2r.h and include/n2v2r_diag.h declare (checked by tests/test_capi.py)
EXPORTED = [
    "n2v2r_create", "n2v2r_destroy", "n2v2r_last_error", "n2v2r_version",
    "n2v2r_set_num_layers", "n2v2r_set_layer_csr", "n2v2r_uase", "n2v2r_get_embedding",
    "n2v2r_get_left_embedding", "n2v2r_get_singular_values", "n2v2r_set_embedding",
    "n2v2r_rank", "n2v2r_get_distances", "n2v2r_get_borda", "n2v2r_rank_timing",
    "n2v2r_pairwise_distances", "n2v2r_borda_columns", "n2v2r_borda_columns_ex",
    "n2v2r_column_sums",
    "n2v2r_synchronize", "n2v2r_bench_spmm", "n2v2r_bench_spmm_tiled", "n2v2r_spmm_col_blocks",
    "n2v2r_comm_unique_id", "n2v2r_create_rccl", "n2v2r_simgroup_create",
    "n2v2r_simgroup_destroy", "n2v2r_create_sim", "n2v2r_dist_info", "n2v2r_set_layer_csr_rows",
    "n2v2r_rr_top", "n2v2r_rr_band_top", "n2v2r_set_layer_dense", "n2v2r_project",
    "n2v2r_create_multi", "n2v2r_multi_devices", "n2v2r_h2d_layer_bytes",
    "n2v2r_set_layer_corr", "n2v2r_get_layer_dense", "n2v2r_transform_layer",
    "n2v2r_bench_transform_pass", "n2v2r_tom_layer", "n2v2r_bench_tom_tiles", "n2v2r_pip_pass",
    "n2v2r_gram_apply", "n2v2r_ritz_step", "n2v2r_layers_to_csr", "n2v2r_count_layer_nonzeros",
    "n2v2r_get_layer_csr_nnz", "n2v2r_get_layer_csr", "n2v2r_bench_sparsify_pass",
    "n2v2r_block_gram", "n2v2r_ortho_pass", "n2v2r_soft_connectivity",
    "n2v2r_soft_connectivity_chunks", "n2v2r_set_layer_corr_method",
    "n2v2r_soft_connectivity_method", "n2v2r_corr_ranks", "n2v2r_corr_standardise",
    "n2v2r_bench_corr_rows", "n2v2r_rr_stage", "n2v2r_embed_step",
]
UNIQUE_ID_BYTES = 128


class ArpackNoConvergence(RuntimeError):
    """UASE eigensolver did not reach the residual tolerance (scipy raises
    ``ArpackNoConvergence`` in the reference's svds path)."""


class EigOpts(ctypes.Structure):
    _fields_ = [("block", ctypes.c_int), ("max_basis", ctypes.c_int), ("keep", ctypes.c_int),
                ("max_restarts", ctypes.c_int), ("tol", ctypes.c_double),
                ("seed", ctypes.c_uint64), ("solver_flags", ctypes.c_int)]


class EigStats(ctypes.Structure):
    _fields_ = [("restarts", ctypes.c_int), ("block_applications", ctypes.c_int),
                ("converged", ctypes.c_int), ("basis", ctypes.c_int),
                ("max_residual", ctypes.c_double), ("ms_total", ctypes.c_double),
                ("ms_spmm", ctypes.c_double), ("ms_ortho", ctypes.c_double),
                ("ms_rr_host", ctypes.c_double), ("spmm_launches", ctypes.c_int64),
                ("spmm_algo_bytes", ctypes.c_double), ("stagnated", ctypes.c_int),
                ("rr_fallbacks", ctypes.c_int), ("gpu_ms_spmm", ctypes.c_double * 2),
                ("spmm_timed_launches", ctypes.c_int64 * 2),
                ("spmm_stage_bytes", ctypes.c_double * 2), ("est_scale", ctypes.c_double),
                ("lean_checks", ctypes.c_int), ("pool_blocks", ctypes.c_int),
                ("spmm_form", ctypes.c_int), ("stag_cap", ctypes.c_double),
                ("y_captured", ctypes.c_int), ("tri_fallbacks", ctypes.c_int)]

    def as_dict(self):
        out = {}
        for k, _ in self._fields_:
            v = getattr(self, k)
            out[k] = list(v) if isinstance(v, ctypes.Array) else v
        return out


class GramInfo(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int) for k in ("form", "rs_form", "rs_chunks", "split2", "tile_nb",
                                            "tile_wb", "tile_rows", "rpw1", "rpw2")]


class EmbedInfo(ctypes.Structure):
    _fields_ = [("form", ctypes.c_int), ("launches", ctypes.c_int), ("ldu", ctypes.c_int),
                ("rpw", ctypes.c_int), ("colmax_chunks", ctypes.c_int64),
                ("colmax_rows", ctypes.c_int64)]


class RitzInfo(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int) for k in ("fused", "launches", "lds_bytes")]


class PassInfo(ctypes.Structure):
    _fields_ = [("gram_form", ctypes.c_int), ("gram_flush", ctypes.c_int),
                ("nchunks", ctypes.c_int64), ("rows_per_chunk", ctypes.c_int64),
                ("stage", ctypes.c_int), ("nwg", ctypes.c_int), ("apply_kernel", ctypes.c_int),
                ("reserved", ctypes.c_int), ("fill_seed", ctypes.c_uint64)]


class RrInfo(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int) for k in ("form_ran", "sturm_err", "second_solves",
                                            "reduce_err", "tri_coop", "msect_points",
                                            "msect_rounds", "reserved")]


# n2v2r_rr_stage's form / n2v2r_rr_info.form_ran
RR_AS_FIT, RR_STURM, RR_BAND_REDUCE, RR_DENSE_FROM_BAND, RR_DENSE = -1, 0, 1, 2, 3

# n2v2r_pass_info.gram_form
GRAM_STREAM, GRAM_LINES, GRAM_NARROW, GRAM_MFMA = 0, 1, 2, 3


class TransformStats(ctypes.Structure):
    _fields_ = [("nonzero", ctypes.c_int64), ("kept", ctypes.c_int64), ("cut", ctypes.c_double)]


# n2v2r_transform_layer flags (include/n2v2r.h)
TF_ABSOLUTE, TF_BINARIZE, TF_THRESHOLD = 1, 2, 4
# n2v2r_tom_layer types: N2V2R_TOM_*
TOM_KINDS = {"unsigned": 0, "signed": 1}


def _warn_zero_mad(what, fallback):
    """The RuntimeWarning of a bicor build in which rows took the Pearson fallback."""
    if int(fallback[0]) > 0:
        warnings.warn(f"{what}: {int(fallback[0])} rows have zero MAD (first: row "
                      f"{int(fallback[1])}); Pearson standardisation used for them",
                      RuntimeWarning, stacklevel=3)


_lib = None
_lock = threading.RLock()  # re-entered: acquire_engine -> Engine() -> load()

_vp = ctypes.c_void_p
_i = ctypes.c_int
_i64 = ctypes.c_int64


def _p(dtype):
    return np.ctypeslib.ndpointer(dtype=dtype, flags="C_CONTIGUOUS")


def load(path: str | None = None):
    """Load (once) and return the ctypes library.  Raises if the .so is absent."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        p = path or LIB_PATH
        if not os.path.exists(p):
            raise RuntimeError(
                f"n2v2r HIP library not found at {p}; build it with "
                "`python -m node2vec2rank_amd.build` (there is no CPU fallback)")
        lib = ctypes.CDLL(p)
        # (registered after the library's own load-time registrations -- HIP's fat-binary
        # module constructor -- and after torch's, so it runs before their teardown)
        atexit.register(_teardown)
        sig = {
            "n2v2r_create": (_i, [_i, ctypes.POINTER(_vp)]),
            "n2v2r_destroy": (None, [_vp]),
            "n2v2r_last_error": (_i, [_vp, ctypes.c_char_p, ctypes.c_size_t]),
            "n2v2r_version": (ctypes.c_char_p, []),
            "n2v2r_set_num_layers": (_i, [_vp, _i, _i64]),
            "n2v2r_set_layer_csr": (_i, [_vp, _i, _i64, _i64, _p(np.int64), _p(np.int32),
                                         _p(np.float32), _i]),
            "n2v2r_uase": (_i, [_vp, _i, ctypes.POINTER(EigOpts), ctypes.POINTER(EigStats)]),
            "n2v2r_get_embedding": (_i, [_vp, _p(np.float32)]),
            "n2v2r_get_left_embedding": (_i, [_vp, _p(np.float32)]),
            "n2v2r_get_singular_values": (_i, [_vp, _p(np.float64)]),
            "n2v2r_set_embedding": (_i, [_vp, _i, _i64, _i, _p(np.float32)]),
            "n2v2r_rank": (_i, [_vp, _i, _p(np.int32), _i, _p(np.int32), _i, _i,
                                ctypes.POINTER(_i), ctypes.POINTER(_i)]),
            "n2v2r_get_distances": (_i, [_vp, _i, _p(np.float64)]),
            "n2v2r_get_borda": (_i, [_vp, _i, _p(np.int64)]),
            "n2v2r_rank_timing": (_i, [_vp, ctypes.POINTER(ctypes.c_double),
                                       ctypes.POINTER(ctypes.c_double)]),
            "n2v2r_pairwise_distances": (_i, [_vp, _p(np.float64), _p(np.float64), _i64, _i, _i,
                                              _p(np.float64)]),
            "n2v2r_borda_columns": (_i, [_vp, _p(np.float64), _i64, _i, _p(np.int64)]),
            "n2v2r_borda_columns_ex": (_i, [_vp, _p(np.float64), _i64, _i, _vp, _i, _vp,
                                            _p(np.int64), _p(np.int32)]),
            "n2v2r_column_sums": (_i, [_vp, _i, _p(np.float32)]),
            "n2v2r_synchronize": (_i, [_vp]),
            "n2v2r_bench_spmm": (_i, [_vp, _i, _i, _i, _i, _p(np.float32), _vp,
                                      ctypes.POINTER(ctypes.c_double),
                                      ctypes.POINTER(ctypes.c_double)]),
            "n2v2r_bench_spmm_tiled": (_i, [_vp, _i, _i, _i, _i, _i, _p(np.float32), _vp,
                                            ctypes.POINTER(ctypes.c_double)]),
            "n2v2r_spmm_col_blocks": (_i, [_vp, _i]),
            "n2v2r_rr_top": (_i, [_vp, _i, _p(np.float64), _i, _p(np.float64), _p(np.float32)]),
            "n2v2r_pip_pass": (_i, [_vp, _i64, _i, _p(np.float32), _p(np.float32), _vp,
                                    ctypes.c_float, _i, _i, ctypes.c_uint64, _p(np.float64), _vp,
                                    _p(np.int32), _p(np.int32), _p(np.int32)]),
            "n2v2r_gram_apply": (_i, [_vp, _i, _p(np.float32), _vp, _p(np.float32),
                                      ctypes.POINTER(GramInfo)]),
            "n2v2r_embed_step": (_i, [_vp, _i, _i, _vp, _vp, ctypes.POINTER(EmbedInfo)]),
            "n2v2r_ritz_step": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                     ctypes.POINTER(RitzInfo)]),
            "n2v2r_block_gram": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, ctypes.POINTER(PassInfo)]),
            "n2v2r_ortho_pass": (_i, [_vp, _i, _i, _vp, _vp, _i, _i, _i, ctypes.c_uint64, _vp,
                                      _vp, _vp, _vp, _vp, ctypes.POINTER(PassInfo)]),
            "n2v2r_rr_band_top": (_i, [_vp, _i, _i, _p(np.float64), ctypes.c_int64, _vp, _i,
                                       _p(np.float64), _p(np.float32)]),
            "n2v2r_rr_stage": (_i, [_vp, _i, _i, _vp, ctypes.c_int64, _vp, _i, _i, _vp, _vp, _vp,
                                    ctypes.POINTER(RrInfo)]),
            "n2v2r_set_layer_dense": (_i, [_vp, _i, _i64, _p(np.float32), _i]),
            "n2v2r_project": (_i, [_vp, _i64, _i64, _p(np.float64), _i, _p(np.float64)]),
            "n2v2r_comm_unique_id": (_i, [ctypes.c_char_p, ctypes.c_size_t]),
            "n2v2r_create_rccl": (_i, [_i, _i, _i, ctypes.c_char_p, ctypes.POINTER(_vp)]),
            "n2v2r_simgroup_create": (_i, [_i, ctypes.POINTER(_vp)]),
            "n2v2r_simgroup_destroy": (None, [_vp]),
            "n2v2r_create_sim": (_i, [_i, _vp, _i, ctypes.POINTER(_vp)]),
            "n2v2r_dist_info": (_i, [_vp, ctypes.POINTER(_i), ctypes.POINTER(_i),
                                     ctypes.POINTER(_i64), ctypes.POINTER(_i64)]),
            "n2v2r_set_layer_csr_rows": (_i, [_vp, _i, _i64, _i64, _i64, _i64, _p(np.int64),
                                              _p(np.int32), _p(np.float32)]),
            "n2v2r_create_multi": (_i, [_p(np.int32), _i, ctypes.POINTER(_vp)]),
            "n2v2r_multi_devices": (_i, [_vp, _vp, _i]),
            "n2v2r_h2d_layer_bytes": (_i, [_vp, _vp, _i]),
            "n2v2r_set_layer_corr": (_i, [_vp, _i, _i64, _i64, _p(np.float64), _i,
                                          ctypes.c_double]),
            "n2v2r_get_layer_dense": (_i, [_vp, _i, _p(np.float32)]),
            "n2v2r_transform_layer": (_i, [_vp, _i, _i, ctypes.c_double, ctypes.c_double,
                                           ctypes.POINTER(TransformStats)]),
            "n2v2r_bench_transform_pass": (_i, [_vp, _i, _i, _i, ctypes.c_double, _i,
                                                ctypes.POINTER(ctypes.c_double),
                                                ctypes.POINTER(ctypes.c_double)]),
            "n2v2r_tom_layer": (_i, [_vp, _i, _i]),
            "n2v2r_bench_tom_tiles": (_i, [_vp, _i, _i, _i, _p(np.float64),
                                           ctypes.POINTER(ctypes.c_double)]),
            "n2v2r_layers_to_csr": (_i, [_vp, _vp]),
            "n2v2r_count_layer_nonzeros": (_i, [_vp, _p(np.int64)]),
            "n2v2r_get_layer_csr_nnz": (_i, [_vp, _i, _i, ctypes.POINTER(_i64)]),
            "n2v2r_get_layer_csr": (_i, [_vp, _i, _i, _p(np.int64), _p(np.int32),
                                         _p(np.float32)]),
            "n2v2r_bench_sparsify_pass": (_i, [_vp, _i, _i, _i, ctypes.POINTER(ctypes.c_double),
                                               ctypes.POINTER(ctypes.c_double)]),
            "n2v2r_soft_connectivity": (_i, [_vp, _i64, _i64, _p(np.float64), _i, _p(np.float64),
                                             _i, _p(np.float64)]),
            "n2v2r_soft_connectivity_chunks": (_i, [_vp, _i64, _i64, _p(np.float64), _i,
                                                    _p(np.float64), _i, _i, _p(np.float64),
                                                    ctypes.POINTER(_i),
                                                    ctypes.POINTER(ctypes.c_double)]),
            "n2v2r_set_layer_corr_method": (_i, [_vp, _i, _i64, _i64, _p(np.float64), _i,
                                                 ctypes.c_double, _i, _vp]),
            "n2v2r_soft_connectivity_method": (_i, [_vp, _i64, _i64, _p(np.float64), _i,
                                                    _p(np.float64), _i, _i, _p(np.float64),
                                                    _vp]),
            "n2v2r_corr_ranks": (_i, [_vp, _i64, _i64, _p(np.float64), _p(np.float64)]),
            "n2v2r_corr_standardise": (_i, [_vp, _i64, _i64, _p(np.float64), _i, _p(np.float64),
                                            ctypes.POINTER(_i64)]),
            "n2v2r_bench_corr_rows": (_i, [_vp, _i64, _i64, _p(np.float64), _i, _i,
                                           _p(np.float64)]),
        }
        for name, (res, args) in sig.items():
            f = getattr(lib, name)
            f.restype = res
            f.argtypes = args
        _lib = lib
        return lib


def comm_unique_id() -> bytes:
    """RCCL unique id (rank 0 creates it and broadcasts the bytes over its control plane)."""
    lib = load()
    buf = ctypes.create_string_buffer(UNIQUE_ID_BYTES)
    st = lib.n2v2r_comm_unique_id(buf, UNIQUE_ID_BYTES)
    if st != OK:
        raise RuntimeError(f"n2v2r_comm_unique_id failed with status {st}")
    return buf.raw


class SimGroup:
    """W ranks as threads of one process on one GPU (the row-partitioned algorithm without W
    devices).  Create one, then one thread per rank builds ``Engine.sim(device, group, r)``."""

    def __init__(self, world: int):
        self.lib = load()
        g = _vp()
        st = self.lib.n2v2r_simgroup_create(int(world), ctypes.byref(g))
        if st != OK:
            raise RuntimeError(f"n2v2r_simgroup_create failed with status {st}")
        self.g = g
        self.world = int(world)

    def close(self):
        if getattr(self, "g", None):
            self.lib.n2v2r_simgroup_destroy(self.g)
            self.g = None


_live = weakref.WeakSet()  # every open Engine (closed by _teardown at interpreter exit)


def _teardown():
    """At interpreter exit, while the HIP runtime (and a profiler tool, under rocprofv3) is
    still up: destroy every open handle -- its device allocations, streams, events and RCCL
    communicators -- before the C exit handlers unregister the library's kernels and tear the
    runtime down, so no library object outlives the runtime.  N2V2R_EXIT_MAPS=path also writes
    /proc/self/maps there (to map the PCs of a crash trace printed later in exit to libraries)."""
    for eng in list(_live):
        try:
            eng.close()
        except Exception:
            pass
    path = os.environ.get("N2V2R_EXIT_MAPS")
    if path:
        try:
            with open("/proc/self/maps") as src, open(path, "w") as dst:
                dst.write(src.read())
        except OSError:
            pass


class Engine:
    """One GPU, one handle.  Thin, typed wrapper over the C-ABI.

    Distributed handles (``Engine.rccl`` / ``Engine.sim``) own rows [row0, row0 + n_local) of
    the node set: ``embedding()`` / ``left_embedding()`` return those rows; distances, Borda,
    singular values and column sums are global on every rank."""

    def __init__(self, device: int = 0, _handle=None):
        self.lib = load()
        if _handle is None:
            h = _vp()
            st = self.lib.n2v2r_create(int(device), ctypes.byref(h))
            if st != OK:
                raise RuntimeError(
                    f"n2v2r_create(device={device}) failed with status {st}: no usable HIP GPU "
                    "(the engine has no CPU fallback)")
        else:
            h = _handle
        self.h = h
        self.device = device
        _live.add(self)

    @classmethod
    def rccl(cls, device: int, rank: int, world: int, unique_id: bytes) -> "Engine":
        lib = load()
        h = _vp()
        st = lib.n2v2r_create_rccl(int(device), int(rank), int(world), bytes(unique_id),
                                   ctypes.byref(h))
        if st != OK:
            raise RuntimeError(f"n2v2r_create_rccl(rank={rank}, world={world}) failed: {st}")
        return cls(device, _handle=h)

    @classmethod
    def multi(cls, devices) -> "Engine":
        """One process, len(devices) GPUs (n2v2r_create_multi): the row-partitioned fit with one
        host thread per GPU inside the library, RCCL over distinct devices (a repeated device:
        the in-process thread group, W ranks sharing it).  Used exactly like a one-GPU engine;
        embeddings, distances and Borda come back global."""
        lib = load()
        devs = np.ascontiguousarray([int(d) for d in devices], dtype=np.int32)
        h = _vp()
        st = lib.n2v2r_create_multi(devs, int(devs.size), ctypes.byref(h))
        if st != OK:
            raise RuntimeError(f"n2v2r_create_multi(devices={devs.tolist()}) failed with status "
                               f"{st}" + (" (RCCL)" if st == ERR_RCCL else ""))
        eng = cls(int(devs[0]), _handle=h)
        eng.devices = tuple(int(d) for d in devs)
        return eng

    @classmethod
    def sim(cls, device: int, group: SimGroup, rank: int) -> "Engine":
        lib = load()
        h = _vp()
        st = lib.n2v2r_create_sim(int(device), group.g, int(rank), ctypes.byref(h))
        if st != OK:
            raise RuntimeError(f"n2v2r_create_sim(rank={rank}) failed with status {st}")
        return cls(device, _handle=h)

    def h2d_layer_bytes(self):
        """Layer bytes each rank of this handle copied host -> device (a list, one per rank)."""
        out = np.zeros(64, dtype=np.int64)
        w = self.lib.n2v2r_h2d_layer_bytes(self.h, out.ctypes.data_as(ctypes.c_void_p), 64)
        if w < 0:
            self._check(w, "h2d_layer_bytes")
        return [int(x) for x in out[:w]]

    def dist_info(self):
        """(rank, world, row0, n_local) of this handle's row block."""
        r, w, r0, nl = _i(), _i(), _i64(), _i64()
        self._check(self.lib.n2v2r_dist_info(self.h, ctypes.byref(r), ctypes.byref(w),
                                             ctypes.byref(r0), ctypes.byref(nl)), "dist_info")
        return r.value, w.value, r0.value, nl.value

    def close(self):
        if getattr(self, "h", None):
            self.lib.n2v2r_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- errors --------------------------------------------------------------------------
    def _err(self) -> str:
        buf = ctypes.create_string_buffer(1024)
        self.lib.n2v2r_last_error(self.h, buf, len(buf))
        return buf.value.decode(errors="replace")

    def _check(self, st: int, what: str):
        if st == OK:
            return
        msg = f"{what}: {self._err()}"
        if st == ERR_UNSUPPORTED_METRIC:
            raise NotImplementedError("Unsupported metric")
        if st == ERR_UNSUPPORTED_AGG:
            raise NotImplementedError("Aggregation method not found. Available methods: Borda")
        if st == ERR_NOT_READY:
            raise ValueError("No n2v2r embeddings found")
        if st == ERR_NO_CONVERGENCE:
            raise ArpackNoConvergence(msg)
        if st == ERR_OUT_OF_MEMORY:
            raise MemoryError(msg)
        if st == ERR_BAD_ARG:
            raise ValueError(msg)
        if st == ERR_RCCL:
            raise RuntimeError(f"RCCL failure: {msg}")
        raise RuntimeError(msg)

    # -- layers ----------------------------------------------------------------------------
    def set_layers(self, layers, symmetric=SYM_DETECT, storage="auto", sparsify=False):
        """layers: list of scipy.sparse matrices (any format) or dense arrays, N x N, or
        ``Coexpression`` layers (an N x samples expression matrix each: the engine builds the
        N x N co-expression layer on the GPU, n2v2r_set_layer_corr; a layer whose ``method`` is
        not Pearson goes through n2v2r_set_layer_corr_method, and a bicor layer in which rows
        have zero MAD raises a ``RuntimeWarning`` with their count and the first of them).

        storage: "csr", "dense" (fp32 N x N in HBM, MFMA GEMMs) or "auto" (dense when every
        layer is a dense array with more than 1/4 of its entries non-zero).  A list that holds a
        ``Coexpression`` is dense storage: its other layers must be dense arrays.

        sparsify: what becomes of dense-storage layers once the last one is built and
        transformed.  ``False``: they stay dense.  ``True``: ``to_csr()``, the conversion to CSR
        in HBM (the sparse fit of a thresholded network).  ``"auto"``: ``to_csr()`` when every
        layer ends at most 1/4 non-zero, counted on the GPU (the rule ``storage="auto"`` applies
        to host arrays; with ``sparsify`` set, dense arrays under ``storage="auto"`` are loaded
        dense and counted there, never scanned on the host).  ``ValueError`` with
        ``storage="csr"`` or sparse inputs: there is nothing to convert."""
        import scipy.sparse as sp
        if not (sparsify is False or sparsify is True or
                (isinstance(sparsify, str) and sparsify == "auto")):
            raise ValueError(f"sparsify must be False, True or 'auto', got {sparsify!r}")
        if sparsify is not False:
            # (as every refusal of this method: before the first library call)
            if any(sp.issparse(a) for a in layers):
                raise ValueError("sparsify converts dense-storage layers: a sparse layer is "
                                 "stored as CSR already, there is nothing to convert")
            if storage == "csr":
                raise ValueError("sparsify converts dense-storage layers: with storage='csr' "
                                 "there is nothing to convert")
            if storage == "auto":
                storage = "dense"
        corr = [isinstance(a, Coexpression) for a in layers]
        if any(corr):
            # (every check before the first library call: a refused list leaves the handle as is)
            if storage == "csr":
                raise ValueError("Coexpression layers are stored dense: storage='csr' does not "
                                 "apply")
            if any(sp.issparse(a) for a in layers):
                raise ValueError("a sparse layer cannot share a handle with Coexpression layers "
                                 "(all layers of a handle are CSR or all dense): pass it as a "
                                 "dense array")
            arrs = [a if c else np.ascontiguousarray(np.asarray(a), dtype=np.float32)
                    for a, c in zip(layers, corr)]
            n = arrs[0].shape[0]
            for a in arrs:
                if a.shape != (n, n):
                    raise ValueError("all layers must be square and share the node set")
            self._check(self.lib.n2v2r_set_num_layers(self.h, len(arrs), n), "set_num_layers")
            for k, a in enumerate(arrs):
                fallback = np.array([0, -1], dtype=np.int64)
                if isinstance(a, Coexpression) and a.method != "pearson":
                    st = self.lib.n2v2r_set_layer_corr_method(
                        self.h, k, n, a.expression.shape[1], a.expression, a.kind_id, a.power,
                        a.method_id, fallback.ctypes.data_as(_vp))
                elif isinstance(a, Coexpression):
                    st = self.lib.n2v2r_set_layer_corr(self.h, k, n, a.expression.shape[1],
                                                       a.expression, a.kind_id, a.power)
                else:
                    st = self.lib.n2v2r_set_layer_dense(self.h, k, n, a, int(symmetric))
                self._check(st, f"layer {k}")
                _warn_zero_mad(f"layer {k}", fallback)
                # WGCNA's order (adjacency, then its topological overlap), then the reference's
                # network_transform
                if isinstance(a, Coexpression) and a.tom is not None:
                    self.tom_layer(k, kind=a.tom)
                if isinstance(a, Coexpression) and a.filters:
                    self.transform_layer(k, threshold=a.threshold,
                                         top_percent_keep=a.top_percent_keep,
                                         binarize=a.binarize)
            self.n = n
            self.num_layers = len(arrs)
            self.storage = "dense"
            self._sparsify(sparsify)
            return
        if storage == "auto":
            storage = "csr"
            if all(not sp.issparse(a) for a in layers):
                arrs = [np.asarray(a) for a in layers]
                if all(_denser_than_quarter(a) for a in arrs):
                    storage = "dense"
        if storage == "dense":
            arrs = [np.ascontiguousarray(np.asarray(a.todense() if sp.issparse(a) else a),
                                         dtype=np.float32) for a in layers]
            n = arrs[0].shape[0]
            for a in arrs:
                if a.shape != (n, n):
                    raise ValueError("all layers must be square and share the node set")
            self._check(self.lib.n2v2r_set_num_layers(self.h, len(arrs), n), "set_num_layers")
            for k, a in enumerate(arrs):
                self._check(self.lib.n2v2r_set_layer_dense(self.h, k, n, a, int(symmetric)),
                            f"layer {k}")
            self.n = n
            self.num_layers = len(arrs)
            self.storage = "dense"
            self._sparsify(sparsify)
            return
        mats = [sp.csr_matrix(a, dtype=np.float32) for a in layers]
        n = mats[0].shape[0]
        for m in mats:
            if m.shape != (n, n):
                raise ValueError("all layers must be square and share the node set")
        self._check(self.lib.n2v2r_set_num_layers(self.h, len(mats), n), "set_num_layers")
        for k, m in enumerate(mats):
            # no sum_duplicates / sort_indices here (an O(nnz) host pass each): the engine
            # checks row order on the GPU and compares unsorted layers through (A^T)^T, and a
            # duplicate entry adds into every product exactly as its summed value would
            indptr = np.ascontiguousarray(m.indptr, dtype=np.int64)
            indices = np.ascontiguousarray(m.indices, dtype=np.int32)
            data = np.ascontiguousarray(m.data, dtype=np.float32)
            self._check(self.lib.n2v2r_set_layer_csr(self.h, k, n, int(m.nnz), indptr, indices,
                                                     data, int(symmetric)), f"layer {k}")
        self.n = n
        self.num_layers = len(mats)
        self.storage = "csr"

    def set_layer_rows(self, n: int, num_layers: int, local_layers):
        """Distributed ingest of symmetric layers from this rank's own rows only:
        ``local_layers[k]`` is the (n_local x n) CSR block of rows [row0, row0 + n_local)."""
        import scipy.sparse as sp
        self._check(self.lib.n2v2r_set_num_layers(self.h, int(num_layers), int(n)),
                    "set_num_layers")
        _, _, row0, nl = self.dist_info()
        for k, blk in enumerate(local_layers):
            m = sp.csr_matrix(blk, dtype=np.float32)
            m.sum_duplicates()
            m.sort_indices()
            if m.shape != (nl, n):
                raise ValueError(f"layer {k}: local block must be {nl} x {n}, got {m.shape}")
            self._check(self.lib.n2v2r_set_layer_csr_rows(
                self.h, k, int(n), int(row0), int(nl), int(m.nnz),
                np.ascontiguousarray(m.indptr, dtype=np.int64),
                np.ascontiguousarray(m.indices, dtype=np.int32),
                np.ascontiguousarray(m.data, dtype=np.float32)), f"layer {k} rows")
        self.n = int(n)
        self.num_layers = int(num_layers)

    # -- UASE ------------------------------------------------------------------------------
    def uase(self, d: int, block=0, max_basis=0, keep=0, max_restarts=0, tol=0.0, seed=0,
             solver_flags=0, raise_on_no_convergence=True):
        o = EigOpts(int(block), int(max_basis), int(keep), int(max_restarts), float(tol),
                    int(seed) & 0xFFFFFFFFFFFFFFFF, int(solver_flags))
        s = EigStats()
        st = self.lib.n2v2r_uase(self.h, int(d), ctypes.byref(o), ctypes.byref(s))
        if st == ERR_NO_CONVERGENCE and not raise_on_no_convergence:
            pass
        else:
            self._check(st, "uase")
        self.d = int(d)
        return s.as_dict()

    def _n_local(self):
        return self.dist_info()[3]

    def embedding(self):
        Y = np.empty((self.num_layers, self._n_local(), self.d), dtype=np.float32)
        self._check(self.lib.n2v2r_get_embedding(self.h, Y), "get_embedding")
        return Y

    def left_embedding(self):
        X = np.empty((self._n_local(), self.d), dtype=np.float32)
        self._check(self.lib.n2v2r_get_left_embedding(self.h, X), "get_left_embedding")
        return X

    def singular_values(self):
        s = np.empty(self.d, dtype=np.float64)
        self._check(self.lib.n2v2r_get_singular_values(self.h, s), "get_singular_values")
        return s

    def set_embedding(self, Y):
        Y = np.ascontiguousarray(Y, dtype=np.float32)
        K, n, d = Y.shape
        self._check(self.lib.n2v2r_set_embedding(self.h, K, n, d, Y), "set_embedding")
        self.num_layers, self.n, self.d = K, n, d

    # -- rank --------------------------------------------------------------------------------
    def rank(self, strategy: str, dims, metrics, method: int = AGG_BORDA):
        """Distances for every (comparison, dim, metric) column on the GPU; their Borda aggregate
        too unless ``method=AGG_NONE``."""
        if strategy not in STRATEGY:
            raise ValueError(f"unknown comp_strategy {strategy!r}")
        mids = []
        for m in metrics:
            if m not in METRIC:
                raise NotImplementedError("Unsupported metric")
            mids.append(METRIC[m])
        dims_a = np.ascontiguousarray(dims, dtype=np.int32)
        met_a = np.ascontiguousarray(mids, dtype=np.int32)
        ncmp = ctypes.c_int()
        ncol = ctypes.c_int()
        self._check(self.lib.n2v2r_rank(self.h, STRATEGY[strategy], dims_a, len(dims_a), met_a,
                                        len(met_a), int(method), ctypes.byref(ncmp),
                                        ctypes.byref(ncol)), "rank")
        self.ncmp, self.ncols = ncmp.value, ncol.value
        return self.ncmp, self.ncols

    def distances(self, comparison: int):
        D = np.empty((self.ncols, self.n), dtype=np.float64)
        self._check(self.lib.n2v2r_get_distances(self.h, int(comparison), D), "get_distances")
        return D.T  # N x C view (column-major on device)

    def borda(self, comparison: int):
        b = np.empty(self.n, dtype=np.int64)
        self._check(self.lib.n2v2r_get_borda(self.h, int(comparison), b), "get_borda")
        return b

    def rank_timing(self):
        a, b = ctypes.c_double(), ctypes.c_double()
        self.lib.n2v2r_rank_timing(self.h, ctypes.byref(a), ctypes.byref(b))
        return a.value, b.value

    # -- seams ------------------------------------------------------------------------------
    def pairwise_distances(self, m1, m2, metric: str):
        if metric not in METRIC:
            raise NotImplementedError("Unsupported metric")
        a = np.ascontiguousarray(m1, dtype=np.float64)
        b = np.ascontiguousarray(m2, dtype=np.float64)
        if a.ndim == 1:
            a = a[:, None]
            b = b[:, None]
        n, dim = a.shape
        out = np.empty(n, dtype=np.float64)
        self._check(self.lib.n2v2r_pairwise_distances(self.h, a, b, n, dim, METRIC[metric], out),
                    "pairwise_distances")
        return out

    def borda_columns(self, D, tie_order: str = "stable", return_tied: bool = False):
        """D: N x C float64 (one ranking column per column) -> int64 Borda in row order.

        tie_order "stable": every column sorted on the GPU, equal values by ascending row.
        "reference": columns holding exact ties (flagged by the GPU) are ordered as the
        reference orders them, pandas ``Series.sort_values(ascending=False)`` (numpy quicksort,
        ``model.py:173-174``), whose order of equal values is implementation-defined, and their
        positions go into the same GPU Borda; tie-free columns (every ER graph of BASELINE) are
        never touched on the host.  return_tied: also return the per-column tie flags."""
        if tie_order not in ("stable", "reference"):
            raise ValueError(f"unknown tie_order {tie_order!r}")
        Dc = np.ascontiguousarray(np.asarray(D, dtype=np.float64).T)
        c, n = Dc.shape
        out = np.empty(n, dtype=np.int64)
        tied = np.zeros(c, dtype=np.int32)
        self._check(self.lib.n2v2r_borda_columns_ex(self.h, Dc, n, c, None, 0, None, out, tied),
                    "borda_columns")
        cols = np.flatnonzero(tied)
        if tie_order == "reference" and cols.size:
            orders = np.empty((cols.size, n), dtype=np.int32)
            for g, j in enumerate(cols):
                orders[g] = reference_descending_order(Dc[j])
            gc = np.ascontiguousarray(cols, dtype=np.int32)
            self._check(self.lib.n2v2r_borda_columns_ex(
                self.h, Dc, n, c, gc.ctypes.data_as(_vp), int(cols.size),
                orders.ctypes.data_as(_vp), out, tied), "borda_columns")
        return (out, tied.astype(bool)) if return_tied else out

    def column_sums(self, k: int):
        out = np.empty(self.n, dtype=np.float32)
        self._check(self.lib.n2v2r_column_sums(self.h, int(k), out), "column_sums")
        return out

    def layer_dense(self, k: int):
        """Dense layer k back on the host (n2v2r_get_layer_dense): N x N float32.  A rank handle
        fills its own rows [row0, row0 + n_local) and leaves the others zero."""
        A = np.zeros((self.n, self.n), dtype=np.float32)
        self._check(self.lib.n2v2r_get_layer_dense(self.h, int(k), A), "layer_dense")
        return A

    def _sparsify(self, sparsify):
        """The ``sparsify`` option of ``set_layers`` on the dense-storage layers just loaded."""
        if sparsify is False:
            return
        if sparsify == "auto" and any(4 * c > self.n * self.n for c in self.count_nonzeros()):
            return
        self.to_csr()

    def count_nonzeros(self) -> list:
        """Stored entries (non-zero, a NaN included, -0 not) of every dense-storage layer, counted
        on the GPU over all ranks (n2v2r_count_layer_nonzeros); nothing changes."""
        out = np.zeros(max(int(getattr(self, "num_layers", 0)), 8), dtype=np.int64)
        self._check(self.lib.n2v2r_count_layer_nonzeros(self.h, out), "count_nonzeros")
        return [int(x) for x in out[:self.num_layers]]

    def to_csr(self) -> list:
        """Every dense-storage layer of the handle to CSR storage, in HBM (n2v2r_layers_to_csr):
        afterwards the handle is what ``set_layers`` with the same matrices as scipy CSR would
        have left, the fit is the sparse one and ``storage == "csr"``.  Returns the stored entries
        per layer (over all ranks).  ``ValueError`` (handle untouched): no layers, a layer not
        loaded, layers that are CSR already; ``MemoryError`` leaves the dense layers in place too."""
        out = np.zeros(max(int(getattr(self, "num_layers", 0)), 8), dtype=np.int64)
        self._check(self.lib.n2v2r_layers_to_csr(self.h, out.ctypes.data_as(ctypes.c_void_p)),
                    "to_csr")
        self.storage = "csr"
        return [int(x) for x in out[:self.num_layers]]

    def layer_csr(self, k: int, transpose: bool = False):
        """CSR layer k back on the host as a ``scipy.sparse.csr_matrix`` of shape (n_local, n)
        (n2v2r_get_layer_csr): this handle's rows, global columns; all N rows on a multi-GPU
        handle.  ``transpose=True``: the A^T copy of a directed layer (``ValueError`` for a
        symmetric one)."""
        import scipy.sparse as sp
        nnz = _i64()
        self._check(self.lib.n2v2r_get_layer_csr_nnz(self.h, int(k), int(bool(transpose)),
                                                     ctypes.byref(nnz)), "layer_csr")
        nl, m = self._n_local(), int(nnz.value)
        indptr = np.zeros(nl + 1, dtype=np.int64)
        indices = np.zeros(max(m, 1), dtype=np.int32)
        data = np.zeros(max(m, 1), dtype=np.float32)
        self._check(self.lib.n2v2r_get_layer_csr(self.h, int(k), int(bool(transpose)), indptr,
                                                 indices, data), "layer_csr")
        return sp.csr_matrix((data[:m], indices[:m], indptr), shape=(nl, self.n))

    def bench_sparsify_pass(self, k: int, which: int, reps: int = 20):
        """Time one kernel of ``to_csr`` alone on dense layer k (n2v2r_bench_sparsify_pass):
        ``which`` 0 the count pass, 1 the compaction.  Returns (ms, layer bytes read)."""
        ms, by = ctypes.c_double(), ctypes.c_double()
        self._check(self.lib.n2v2r_bench_sparsify_pass(self.h, int(k), int(which), int(reps),
                                                       ctypes.byref(ms), ctypes.byref(by)),
                    "bench_sparsify_pass")
        return ms.value, by.value

    def transform_layer(self, k: int, threshold=None, top_percent_keep=100, binarize=False,
                        absolute=False) -> dict:
        """``network_transform`` of the loaded dense-storage layer k, in place on the GPU
        (n2v2r_transform_layer): what ``ingest.transform`` gives on the layer's stored values, bit
        for bit.  Returns ``{"nonzero", "kept", "cut"}``: the entries alive before the
        percentile cut, the survivors and the cut.  ``ValueError`` (layer untouched): an
        argument out of range, a CSR-storage layer, a NaN in the layer, or a layer with no
        non-zero entry left."""
        try:
            thr = 0.0 if threshold is None else float(threshold)
            top = float(top_percent_keep)
        except (TypeError, ValueError):
            raise ValueError("threshold and top_percent_keep must be numbers, got "
                             f"{threshold!r} and {top_percent_keep!r}") from None
        flags = ((TF_ABSOLUTE if absolute else 0) | (TF_BINARIZE if binarize else 0) |
                 (0 if threshold is None else TF_THRESHOLD))
        st = TransformStats()
        self._check(self.lib.n2v2r_transform_layer(self.h, int(k), flags, thr, top,
                                                   ctypes.byref(st)), f"transform_layer {k}")
        return {"nonzero": int(st.nonzero), "kept": int(st.kept), "cut": float(st.cut)}

    def tom_layer(self, k: int, kind: str = "unsigned"):
        """Replace the loaded symmetric dense-storage layer k by its topological overlap matrix
        on the GPU (n2v2r_tom_layer): WGCNA's ``TOMsimilarity`` with ``TOMDenom="min"``, fp64
        rounded once to fp32, the layer's diagonal ignored and the result's set to 1.  kind:
        ``"unsigned"`` (entries in [0, 1]) or ``"signed"`` (entries in [-1, 1], a ``"raw"``
        co-expression layer).  ``ValueError`` (layer untouched): an unknown kind, a layer that
        is not loaded, CSR-stored or directed, a NaN or a value outside the kind's range."""
        if not isinstance(kind, str) or kind.casefold() not in TOM_KINDS:
            raise ValueError(f"unknown TOM kind {kind!r}; options are {sorted(TOM_KINDS)}")
        self._check(self.lib.n2v2r_tom_layer(self.h, int(k), TOM_KINDS[kind.casefold()]),
                    f"tom_layer {k}")

    def bench_tom_tiles(self, k: int, kind: str = "unsigned", reps: int = 5):
        """Time the tile kernel of ``tom_layer`` alone (n2v2r_bench_tom_tiles; the layer stays as
        it is).  Returns (the launches' ms as an array, the flop of one launch)."""
        ms = np.zeros(int(reps), dtype=np.float64)
        flop = ctypes.c_double()
        self._check(self.lib.n2v2r_bench_tom_tiles(self.h, int(k), TOM_KINDS[kind], int(reps), ms,
                                                   ctypes.byref(flop)), "bench_tom_tiles")
        return ms, flop.value

    def bench_transform_pass(self, k: int, which: int, threshold=None, absolute=False,
                             reps: int = 20):
        """Time one kernel of ``transform_layer`` alone (n2v2r_bench_transform_pass): ``which``
        0..3 a histogram pass, 4 the min pass, 5 the apply pass.  Returns (ms, bytes read)."""
        flags = (TF_ABSOLUTE if absolute else 0) | (0 if threshold is None else TF_THRESHOLD)
        ms, by = ctypes.c_double(), ctypes.c_double()
        self._check(self.lib.n2v2r_bench_transform_pass(
            self.h, int(k), int(which), flags, 0.0 if threshold is None else float(threshold),
            int(reps), ctypes.byref(ms), ctypes.byref(by)), "bench_transform_pass")
        return ms.value, by.value

    def bench_spmm(self, k: int, X, transpose: bool = False, reps: int = 20, want_y=True):
        """Time the SpMM kernel alone (HIP events on the engine stream)."""
        X = np.ascontiguousarray(X, dtype=np.float32)
        n, b = X.shape
        Y = np.empty((self._n_local(), b), dtype=np.float32) if want_y else None
        ms, by = ctypes.c_double(), ctypes.c_double()
        yp = Y.ctypes.data_as(ctypes.c_void_p) if want_y else None
        self._check(self.lib.n2v2r_bench_spmm(self.h, int(k), int(bool(transpose)), int(b),
                                              int(reps), X, yp, ctypes.byref(ms),
                                              ctypes.byref(by)), "bench_spmm")
        return Y, ms.value, by.value

    def bench_spmm_tiled(self, k: int, X, transpose: bool = False, nb: int = 0, reps: int = 20,
                         want_y=True):
        """Time the flat-window tiled SpMM (panel width 8) of layer k alone."""
        X = np.ascontiguousarray(X, dtype=np.float32)
        n, b = X.shape
        Y = np.empty((self._n_local(), b), dtype=np.float32) if want_y else None
        ms = ctypes.c_double()
        yp = Y.ctypes.data_as(ctypes.c_void_p) if want_y else None
        self._check(self.lib.n2v2r_bench_spmm_tiled(self.h, int(k), int(bool(transpose)), int(b),
                                                    int(nb), int(reps), X, yp, ctypes.byref(ms)),
                    "bench_spmm_tiled")
        return Y, ms.value

    def spmm_col_blocks(self, b: int = 8) -> bool:
        """True when the SpMM at panel width b runs the XCD-local column-block form."""
        r = self.lib.n2v2r_spmm_col_blocks(self.h, int(b))
        if r < 0 or r > 1:
            self._check(r, "spmm_col_blocks")
        return r == 1

    def project(self, W, on: str = "columns"):
        """W^T W (on="columns") or W W^T (on="rows") of a dense m x n matrix, fp64 on the GPU
        (the reference's float64 ``np.matmul``, ``preprocessing_utils.py:22-24``)."""
        W = np.ascontiguousarray(np.asarray(W), dtype=np.float64)
        m, n = W.shape
        oc = on.casefold() == "columns"
        if not oc and on.casefold() != "rows":
            raise ValueError("Unknown projection type, options are columns or rows")
        k = n if oc else m
        out = np.empty((k, k), dtype=np.float64)
        self._check(self.lib.n2v2r_project(self.h, m, n, W, int(oc), out), "project")
        return out

    def _soft_args(self, E, kind, powers):
        values = getattr(E, "values", E)  # (a DataFrame's array)
        try:
            e = np.ascontiguousarray(np.asarray(values), dtype=np.float64)
            pw = np.ascontiguousarray(np.asarray(powers), dtype=np.float64).reshape(-1)
        except (TypeError, ValueError) as err:
            raise ValueError(f"expression and powers must be real arrays: {err}") from None
        if e.ndim != 2:
            raise ValueError(f"expression must be 2-D (n x samples), got {e.ndim}-D")
        if not isinstance(kind, str) or kind.replace("_", " ").casefold() not in KINDS:
            raise ValueError(f"unknown kind {kind!r}; options are {sorted(KINDS)}")
        return e, KINDS[kind.replace("_", " ").casefold()], pw

    def soft_connectivity(self, E, kind: str = "unsigned", powers=(6.0,),
                          method: str = "pearson"):
        """Connectivities for a soft-threshold scan (n2v2r_soft_connectivity): for the
        ``n x samples`` expression matrix E and each candidate power p, ``k_i(p) = sum_{j != i}
        t(r_ij) ** p`` with r and t as a ``Coexpression`` layer of that kind evaluates them, summed
        in fp64 on the GPU without an n x n array anywhere.  Returns ``(len(powers), n)`` float64.
        The loaded layers, the embedding and ``storage`` stay as they are.  ``ValueError``: fewer
        than 2 samples, more than 32 powers, a power not finite or < 1, kind ``"raw"`` or
        unknown, a row of E that is constant or holds a non-finite value (named by index).

        method: ``"pearson"``, ``"spearman"`` or ``"bicor"`` (n2v2r_soft_connectivity_method), the
        correlation r as a ``Coexpression`` layer of that method evaluates it; a bicor scan in
        which rows have zero MAD raises the ``RuntimeWarning`` ``set_layers`` raises."""
        e, kid, pw = self._soft_args(E, kind, powers)
        mid = METHODS[method_name(method)]
        out = np.empty((pw.size, e.shape[0]), dtype=np.float64)
        if mid == 0:
            self._check(self.lib.n2v2r_soft_connectivity(self.h, e.shape[0], e.shape[1], e, kid,
                                                         pw, int(pw.size), out),
                        "soft_connectivity")
            return out
        fallback = np.array([0, -1], dtype=np.int64)
        self._check(self.lib.n2v2r_soft_connectivity_method(
            self.h, e.shape[0], e.shape[1], e, kid, pw, int(pw.size), mid, out,
            fallback.ctypes.data_as(_vp)), "soft_connectivity")
        _warn_zero_mad("soft_connectivity", fallback)
        return out

    def _rows_arg(self, E):
        values = getattr(E, "values", E)  # (a DataFrame's array)
        try:
            e = np.ascontiguousarray(np.asarray(values), dtype=np.float64)
        except (TypeError, ValueError) as err:
            raise ValueError(f"expression must be a real n x samples array: {err}") from None
        if e.ndim != 2:
            raise ValueError(f"expression must be 2-D (n x samples), got {e.ndim}-D")
        return e

    def corr_ranks(self, E):
        """The per-row average ranks of E (n x samples) as the Spearman path computes them on the
        GPU (n2v2r_corr_ranks): ``scipy.stats.rankdata(E, axis=1)``, exact half-integers in
        float64; a row that holds a non-finite value comes back as NaNs."""
        e = self._rows_arg(E)
        out = np.empty_like(e)
        self._check(self.lib.n2v2r_corr_ranks(self.h, e.shape[0], e.shape[1], e, out),
                    "corr_ranks")
        return out

    def corr_standardise(self, E, method: str = "pearson", return_bad_row: bool = False):
        """The standardised rows Z (n x samples float64) whose products Z Z^T are the
        correlations of ``method`` (n2v2r_corr_standardise).  A row that is constant or holds a
        non-finite value is zeros, not an error; with ``return_bad_row`` the result is
        ``(Z, the smallest such row or -1)``."""
        e = self._rows_arg(E)
        out = np.empty_like(e)
        bad = _i64()
        self._check(self.lib.n2v2r_corr_standardise(self.h, e.shape[0], e.shape[1], e,
                                                    METHODS[method_name(method)], out,
                                                    ctypes.byref(bad)), "corr_standardise")
        return (out, int(bad.value)) if return_bad_row else out

    def bench_corr_rows(self, E, method: str = "pearson", reps: int = 10):
        """The row kernel of ``method`` alone (Pearson: the standardisation, Spearman: the
        ranking, bicor: its standardisation), ``reps`` launches after a warm-up, one HIP event
        pair each (n2v2r_bench_corr_rows).  Returns the times in ms."""
        e = self._rows_arg(E)
        ms = np.empty(int(reps), dtype=np.float64)
        self._check(self.lib.n2v2r_bench_corr_rows(self.h, e.shape[0], e.shape[1], e,
                                                   METHODS[method_name(method)], int(reps), ms),
                    "bench_corr_rows")
        return ms

    def soft_connectivity_chunks(self, E, kind: str = "unsigned", powers=(6.0,), chunks: int = 0):
        """``soft_connectivity`` with the chunk count of the scan given (0: the call's own) and
        the scan kernel timed (n2v2r_soft_connectivity_chunks).  Returns (the connectivities, the
        chunk count that ran, the scan kernel's ms from one HIP event pair)."""
        e, kid, pw = self._soft_args(E, kind, powers)
        out = np.empty((pw.size, e.shape[0]), dtype=np.float64)
        used, ms = _i(), ctypes.c_double()
        self._check(self.lib.n2v2r_soft_connectivity_chunks(
            self.h, e.shape[0], e.shape[1], e, kid, pw, int(pw.size), int(chunks), out,
            ctypes.byref(used), ctypes.byref(ms)), "soft_connectivity_chunks")
        return out, used.value, ms.value

    def rr_top(self, H, p: int):
        """Rayleigh-Ritz stage alone: top-p eigenpairs of symmetric H (GPU tridiagonalisation,
        bisection + inverse iteration, back-transform).  Returns (w, S)."""
        H = np.ascontiguousarray(H, dtype=np.float64)
        c = H.shape[0]
        w = np.empty(p, dtype=np.float64)
        S = np.empty((c, p), dtype=np.float32)
        self._check(self.lib.n2v2r_rr_top(self.h, c, H, int(p), w, S), "rr_top")
        return w, S

    def pip_pass(self, Q, Za, Zb=None, tau: float = 0.0, first: int = 0, form: int = 0,
                 seed: int = 1):
        """One orthogonalisation pass at block width 8 alone (see n2v2r_pip_pass).  Q: (nq, n, 8)
        fp32; Za, Zb: (n, 8) fp32 (Zb given: the paired full pass, form 0 its three launches,
        form 1 the paired apply).  Returns a dict: the block(s) after the pass, the fp64 Gram the
        pass used ((nq + 1, 8, 8), or (2, nq + 2, 8, 8)), R (single pass), flags, any_flag and
        the skip counters."""
        Q = np.ascontiguousarray(Q, dtype=np.float32)
        nq, n = Q.shape[0], Q.shape[1]
        za = np.array(Za, dtype=np.float32, order="C")
        zb = None if Zb is None else np.array(Zb, dtype=np.float32, order="C")
        if Q.shape != (nq, n, 8) or za.shape != (n, 8) or (zb is not None and zb.shape != (n, 8)):
            raise ValueError("pip_pass: Q is (nq, n, 8), Za and Zb are (n, 8)")
        nz = 1 if zb is None else 2
        gram = np.empty((nq + 1, 8, 8) if zb is None else (2, nq + 2, 8, 8), dtype=np.float64)
        R = np.empty((8, 8), dtype=np.float64) if zb is None else None
        flags = np.empty(8, dtype=np.int32)
        any_flag = np.empty(1, dtype=np.int32)
        skipped = np.empty(nq + nz, dtype=np.int32)
        self._check(self.lib.n2v2r_pip_pass(
            self.h, n, nq, Q, za, None if zb is None else zb.ctypes.data_as(ctypes.c_void_p),
            float(tau), int(first), int(form), int(seed), gram,
            None if R is None else R.ctypes.data_as(ctypes.c_void_p), flags, any_flag, skipped),
            "pip_pass")
        return {"Za": za, "Zb": zb, "gram": gram, "R": R, "flags": flags,
                "any_flag": int(any_flag[0]), "skipped": skipped}

    def gram_apply(self, X, want_z: bool = True):
        """One application W = sum_k A_k (A_k^T X) through the solver's own launches (see
        n2v2r_gram_apply).  X: the global (N, b) fp32 panel, b = 8, 16, 32 or 64; on a rank handle
        every rank calls with the same X.  Returns (W, Z, info): this handle's (n_local, b) rows
        of M X, the stage-1 panels (K, n_local, b) (None without want_z) and a dict naming the form
        that ran (the fields of n2v2r_gram_info)."""
        X = np.ascontiguousarray(X, dtype=np.float32)
        if X.ndim != 2 or X.shape[0] != self.n:
            raise ValueError(f"gram_apply: X must be ({self.n}, b), got {X.shape}")
        b, nl = X.shape[1], self._n_local()
        W = np.empty((nl, b), dtype=np.float32)
        Z = np.empty((self.num_layers, nl, b), dtype=np.float32) if want_z else None
        info = GramInfo()
        self._check(self.lib.n2v2r_gram_apply(
            self.h, int(b), X, Z.ctypes.data_as(ctypes.c_void_p) if want_z else None, W,
            ctypes.byref(info)), "gram_apply")
        return W, Z, {k: getattr(info, k) for k, _ in GramInfo._fields_}

    def embed_step(self, U, theta, b: int = 8):
        """The step from a converged fit's left vectors to the embedding alone (see
        n2v2r_embed_step): signs, sigma = sqrt(theta) and Y_k = A_k^T U sigma^(-1/2) in the form a
        fit at block width b takes on this handle.  U: the global (N, d) fp32 matrix (on a rank
        handle every rank calls with the same U); theta: d fp64.  The result is installed as the
        handle's embedding: read it with embedding(), left_embedding() and singular_values().
        Returns a dict of n2v2r_embed_info's fields."""
        if U is None or theta is None:
            raise ValueError("embed_step: U and theta are required")
        U = np.ascontiguousarray(U, dtype=np.float32)
        theta = np.ascontiguousarray(theta, dtype=np.float64)
        if U.ndim != 2 or U.shape[0] != self.n or theta.shape != (U.shape[1],):
            raise ValueError(f"embed_step: U must be ({self.n}, d) and theta (d,), got "
                             f"{U.shape} and {theta.shape}")
        info = EmbedInfo()
        self._check(self.lib.n2v2r_embed_step(
            self.h, int(b), int(U.shape[1]), U.ctypes.data_as(ctypes.c_void_p),
            theta.ctypes.data_as(ctypes.c_void_p), ctypes.byref(info)), "embed_step")
        self.d = int(U.shape[1])
        return {k: getattr(info, k) for k, _ in EmbedInfo._fields_}

    def ritz_step(self, Q, W, S, theta, lean: bool = False):
        """The step between Rayleigh-Ritz and the next cycle alone (see n2v2r_ritz_step).  Q, W:
        (nq, n_local, b) fp32 basis blocks and images (W None when lean); S: (nq b, keep) fp32;
        theta: keep fp64.  Returns (X, MX, res, info): (keep / b, n_local, b) fp32 blocks (MX and
        res None when lean), keep fp64 squared residuals and a dict of n2v2r_ritz_info's fields."""
        Q = np.ascontiguousarray(Q, dtype=np.float32)
        S = np.ascontiguousarray(S, dtype=np.float32)
        theta = np.ascontiguousarray(theta, dtype=np.float64)
        W = None if W is None else np.ascontiguousarray(W, dtype=np.float32)
        nl = self._n_local()
        if Q.ndim != 3 or Q.shape[1] != nl or (W is not None and W.shape != Q.shape):
            raise ValueError(f"ritz_step: Q and W must be (nq, {nl}, b), got {Q.shape}")
        nq, b = Q.shape[0], Q.shape[2]
        if S.ndim != 2 or S.shape[0] != nq * b or theta.shape != (S.shape[1],):
            raise ValueError("ritz_step: S must be (nq b, keep) and theta (keep,)")
        keep = S.shape[1]
        pb = max(1, keep // max(b, 1))
        X = np.empty((pb, nl, b), dtype=np.float32)
        MX = None if lean else np.empty((pb, nl, b), dtype=np.float32)
        res = None if lean else np.empty(keep, dtype=np.float64)
        info = RitzInfo()

        def ptr(a):
            return None if a is None else a.ctypes.data_as(ctypes.c_void_p)

        self._check(self.lib.n2v2r_ritz_step(
            self.h, int(b), int(nq), int(keep), int(bool(lean)), ptr(Q), ptr(W), ptr(S),
            ptr(theta), ptr(X), ptr(MX), ptr(res), ctypes.byref(info)), "ritz_step")
        return X, MX, res, {k: getattr(info, k) for k, _ in RitzInfo._fields_}

    def block_gram(self, A, B):
        """G = [A]^T [B] through the solver's own Gram method (see n2v2r_block_gram).  A, B:
        (na, n_local, b) and (nb, n_local, b) fp32 blocks.  Returns (G, info): (na b, nb b) fp64
        and a dict of n2v2r_pass_info's fields."""
        A = np.ascontiguousarray(A, dtype=np.float32)
        B = np.ascontiguousarray(B, dtype=np.float32)
        nl = self._n_local()
        if A.ndim != 3 or B.ndim != 3 or A.shape[1:] != B.shape[1:] or A.shape[1] != nl:
            raise ValueError(f"block_gram: A and B must be (blocks, {nl}, b), got {A.shape}, "
                             f"{B.shape}")
        na, nb, b = A.shape[0], B.shape[0], A.shape[2]
        G = np.empty((na * b, nb * b), dtype=np.float64)
        info = PassInfo()
        vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        self._check(self.lib.n2v2r_block_gram(self.h, int(b), int(na), int(nb), vp(A), vp(B),
                                              vp(G), ctypes.byref(info)), "block_gram")
        return G, {k: getattr(info, k) for k, _ in PassInfo._fields_}

    def ortho_pass(self, Q, Z, in_place: bool = True, first: int = 0, cond: int = -1,
                   seed: int = 1):
        """One orthogonalisation pass at block width b alone (see n2v2r_ortho_pass).  Q:
        (nq, n_local, b) fp32, nq >= 0; Z: (n_local, b) fp32.  Returns a dict: Z after the pass,
        the fp64 Gram ((nq + 1) b, b), xinv (b, b) and F ((nq + 1) b, b) (both None at b = 8),
        flags, any_flag and info (n2v2r_pass_info's fields)."""
        z = np.array(Z, dtype=np.float32, order="C")
        nl = self._n_local()
        if z.ndim != 2 or z.shape[0] != nl:
            raise ValueError(f"ortho_pass: Z must be ({nl}, b), got {z.shape}")
        b = z.shape[1]
        Q = np.ascontiguousarray(Q, dtype=np.float32).reshape(-1, nl, b)
        nq = Q.shape[0]
        gram = np.empty(((nq + 1) * b, b), dtype=np.float64)
        xinv = None if b == 8 else np.empty((b, b), dtype=np.float64)
        F = None if b == 8 else np.empty(((nq + 1) * b, b), dtype=np.float32)
        flags = np.empty(b, dtype=np.int32)
        any_flag = np.empty(1, dtype=np.int32)
        info = PassInfo()
        vp = lambda a: None if a is None or a.size == 0 else a.ctypes.data_as(ctypes.c_void_p)
        self._check(self.lib.n2v2r_ortho_pass(
            self.h, int(b), int(nq), vp(Q), vp(z), int(bool(in_place)), int(first), int(cond),
            int(seed), vp(gram), vp(xinv), vp(F), vp(flags), vp(any_flag), ctypes.byref(info)),
            "ortho_pass")
        return {"Z": z, "gram": gram, "xinv": xinv, "F": F, "flags": flags,
                "any_flag": int(any_flag[0]),
                "info": {k: getattr(info, k) for k, _ in PassInfo._fields_}}

    def rr_band_top(self, hband, c: int, kp: int, theta_prev, p: int):
        """Banded Rayleigh-Ritz stage alone (see n2v2r_rr_band_top).  Returns (w, S)."""
        hband = np.ascontiguousarray(hband, dtype=np.float64).ravel()
        tp = None
        if kp > 0:
            tp = np.ascontiguousarray(theta_prev, dtype=np.float64)
        w = np.empty(p, dtype=np.float64)
        S = np.empty((c, p), dtype=np.float32)
        self._check(self.lib.n2v2r_rr_band_top(
            self.h, int(c), int(kp), hband, int(hband.size),
            None if tp is None else tp.ctypes.data_as(ctypes.c_void_p), int(p), w, S),
            "rr_band_top")
        return w, S

    def rr_stage(self, hband, c: int, kp: int, theta_prev, p: int, form: int = RR_AS_FIT):
        """One Rayleigh-Ritz of a Krylov-Schur projected matrix in one chosen form (see
        n2v2r_rr_stage; form: RR_AS_FIT, RR_STURM, RR_BAND_REDUCE or RR_DENSE_FROM_BAND).
        Returns (w, S, Y, info): p fp64 values, (c, p) fp32 and fp64 vectors (Y is NaN from the
        forms that hold no fp64 vectors in H's basis) and a dict of n2v2r_rr_info's fields."""
        hband = np.ascontiguousarray(hband, dtype=np.float64).ravel()
        tp = None if theta_prev is None else np.ascontiguousarray(theta_prev, dtype=np.float64)
        w = np.empty(max(int(p), 0), dtype=np.float64)
        S = np.empty((max(int(c), 0), w.size), dtype=np.float32)
        Y = np.empty(S.shape, dtype=np.float64)
        info = RrInfo()
        vp = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
        self._check(self.lib.n2v2r_rr_stage(
            self.h, int(c), int(kp), vp(hband), int(hband.size), vp(tp), int(p), int(form),
            vp(w), vp(S), vp(Y), ctypes.byref(info)), "rr_stage")
        return w, S, Y, {k: getattr(info, k) for k, _ in RrInfo._fields_}

    def synchronize(self):
        self._check(self.lib.n2v2r_synchronize(self.h), "synchronize")


def reference_descending_order(col) -> np.ndarray:
    """Row indices of one ranking column best first, exactly as the reference sorts it:
    ``pd.Series(col, index=node_names).sort_values(ascending=False)`` (``model.py:173-174``),
    i.e. pandas ``nargsort``: reverse, ``argsort(kind='quicksort')``, reverse, NaNs last in row
    order.  The order of equal values is whatever this host's numpy quicksort gives, as in the
    reference; only columns the GPU flags as tied come here."""
    import pandas as pd
    return pd.Series(np.asarray(col, dtype=np.float64)).sort_values(
        ascending=False).index.to_numpy(dtype=np.int64)


_default = {}


def new_engine(device) -> Engine:
    """An engine on one device (int) or on several (a tuple of devices: Engine.multi)."""
    if isinstance(device, tuple):
        return Engine.multi(device)
    return Engine(device)


def default_engine(device: int = 0) -> Engine:
    """Process-wide engine per device (the handle is not thread-safe)."""
    e = _default.get(device)
    if e is None or e.h is None:
        e = Engine(device)
        _default[device] = e
    return e


def _denser_than_quarter(a) -> bool:
    """More than a quarter of the entries non-zero (the storage choice of ``set_layers``; dense
    and CSR storage give the same products).  A strided sample of ~2M entries decides when its
    density is clearly on one side of 1/4 (a dense co-expression layer: one pass over 1/200 of
    it instead of a quarter of it, 0.12 s per 20k x 20k layer); otherwise the exact count, in row
    blocks that stop as soon as the answer is known."""
    if a.size == 0:
        return False
    a2 = a.reshape(a.shape[0], -1) if a.ndim > 1 else a.reshape(1, -1)
    rows, cols = a2.shape
    stride = max(1, rows // max(1, (1 << 21) // max(1, cols)))
    if stride > 1:
        sample = a2[::stride]
        p = np.count_nonzero(sample) / sample.size
        if p > 0.3:
            return True
        if p < 0.2:
            return False
    need = a.size // 4
    step = max(1, (1 << 24) // max(1, cols))
    nz = 0
    for r in range(0, rows, step):
        nz += int(np.count_nonzero(a2[r:r + step]))
        if nz > need:
            return True
        if nz + (rows - r - step) * cols <= need:
            return False
    return nz > need


# Handles per device for the drop-in N2V2R models: a handle whose owner model is gone (or has
# none) is reused with its device allocations; a new one is made while every handle is owned,
# up to POOL_MAX, beyond which the least recently acquired handle is taken over (its owner's
# ``_hand_over()`` first copies what it still needs to the host).
POOL_MAX = 4
_pool = {}
_pool_tick = [0]


def engine_owner(eng: Engine):
    ref = getattr(eng, "_owner", None)
    return ref() if ref is not None else None


def acquire_engine(device: int, owner) -> Engine:
    import weakref
    with _lock:
        handles = _pool.setdefault(device, [])
        handles[:] = [e for e in handles if e.h is not None]
        free = [e for e in handles if engine_owner(e) is None]
        if free:
            eng = free[0]
        elif len(handles) < POOL_MAX:
            eng = new_engine(device)
            handles.append(eng)
        else:
            eng = min(handles, key=lambda e: getattr(e, "_tick", 0))
            prev = engine_owner(eng)
            if prev is not None and hasattr(prev, "_hand_over"):
                prev._hand_over()
        _pool_tick[0] += 1
        eng._tick = _pool_tick[0]
        eng._owner = weakref.ref(owner)
        return eng
