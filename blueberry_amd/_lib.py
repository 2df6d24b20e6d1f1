"""ctypes binding of libblueberry_hip.so (C-ABI: include/blueberry_hip.h).

There is deliberately NO fallback here: if the shared library is missing, or
there is no usable MI355X, every compute call raises.  The CPU oracle under
oracle/ is test infrastructure and is never imported from this package.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# BB_LIB: load another build of the same library (kernel-tuning experiments only)
LIB_PATH = os.environ.get("BB_LIB") or os.path.join(_HERE, "libblueberry_hip.so")

BB_OK, BB_ERR_INVALID, BB_ERR_HIP, BB_ERR_STATE, BB_ERR_NOMEM = 0, 1, 2, 3, 4
BB_F32, BB_F64 = 0, 1
BB_KIND_WISH, BB_KIND_COUNTS = 0, 1
BB_PEER_HANDLE_BYTES = 128
BB_CMP_SPEARMAN = 1
BB_COARSEN_SUM, BB_COARSEN_MEAN = 0, 1

c_i32, c_i64, c_dbl = ctypes.c_int32, ctypes.c_int64, ctypes.c_double
p_i32, p_i64, p_dbl = (ctypes.POINTER(c_i32), ctypes.POINTER(c_i64), ctypes.POINTER(c_dbl))
c_int, c_void_p = ctypes.c_int, ctypes.c_void_p
p_u8 = ctypes.POINTER(ctypes.c_ubyte)       # uint8_t: masks and flags


class LayoutInfo(ctypes.Structure):
    """struct bb_layout_info (include/blueberry_hip.h)."""
    _fields_ = [(name, c_i64) for name in (
        "n_bins", "n_pad", "vw", "rows_per_unit", "units_per_tile", "n_blocks", "n_tiles",
        "n_units")]

    def as_dict(self):
        return {name: int(getattr(self, name)) for name, _ in self._fields_}


class SweepKnobs(ctypes.Structure):
    """struct bb_sweep_knobs (include/blueberry_hip.h)."""
    _fields_ = [(name, c_i32) for name in ("waves_per_cu", "pair", "reduce_slices", "row_owner")]


class SweepPlan(ctypes.Structure):
    """struct bb_sweep_plan (include/blueberry_hip.h)."""
    _fields_ = [(name, c_i64) for name in (
        "n_local", "t_first", "n_local_tiles", "n_waves", "wpb", "chunk_q", "chunk_r", "n_slots",
        "rowpart_elems", "colpart_elems", "zero_off", "part_total", "red_slices", "red_stride",
        "red_blocks", "defer_cap_units", "lds_wave_floats", "defer_lds_bytes", "nontemporal",
        "full_ld", "ro_wpr", "ro_blocks")]
    as_dict = LayoutInfo.as_dict


# name -> (restype, argtypes); every symbol include/blueberry_hip.h declares
SIGNATURES = {
    "bb_version": (c_int, []),
    "bb_last_error": (ctypes.c_char_p, []),
    "bb_device_count": (c_int, [ctypes.POINTER(c_int)]),
    "bb_band_count": (c_int, [p_dbl, c_i64, c_i32, c_i32, c_int, p_i64]),
    "bb_band_count_rows": (c_int, [p_dbl, c_i64, c_i32, c_i32, c_i64, c_i64, c_int, p_i64]),
    "bb_layout_dense_info": (c_int, [c_i64, c_int, ctypes.POINTER(LayoutInfo)]),
    "bb_layout_dense_tiles": (c_int, [c_i64, c_int, p_i32, p_i32, c_i64]),
    "bb_layout_rank_units": (c_int, [c_i64, c_int, c_int, p_i64, p_i64]),
    "bb_layout_sweep_plan": (c_int, [c_i64, c_int, p_i32, p_i32, c_i64, c_i64, c_i64, c_int,
                                     ctypes.POINTER(SweepKnobs), ctypes.POINTER(SweepPlan), p_i32,
                                     p_i32, p_i32, p_i32, p_i64]),
    "bb_layout_pk24_table": (c_int, [ctypes.POINTER(ctypes.c_uint32), p_i32, c_i64, c_i64, c_int,
                                     p_i32, p_i64, p_i64, p_i64, ctypes.POINTER(c_int)]),
    "bb_solver_create": (c_int, [ctypes.POINTER(c_void_p), c_i64, c_int, c_int, c_int, c_int,
                                 p_i32, p_i32, c_i64]),
    "bb_solver_destroy": (c_int, [c_void_p]),
    "bb_solver_set_stream": (c_int, [c_void_p, c_void_p]),
    "bb_solver_layout": (c_int, [c_void_p, ctypes.POINTER(LayoutInfo), p_i64, p_i64]),
    "bb_solver_set_wish_dense": (c_int, [c_void_p, p_dbl, c_i64, c_int, c_dbl]),
    "bb_solver_set_wish_sparse": (c_int, [c_void_p, p_i64, p_i64, p_dbl, c_i64, c_int, c_dbl,
                                          p_dbl, p_dbl]),
    "bb_triples_create": (c_int, [ctypes.POINTER(c_void_p), p_dbl, c_i64, c_i32, c_i32, c_int]),
    "bb_triples_destroy": (c_int, [c_void_p]),
    "bb_triples_tiles": (c_int, [c_void_p, c_i64, c_int, p_u8, c_i64]),
    "bb_solver_set_wish_triples": (c_int, [c_void_p, c_void_p, c_int, c_dbl, p_dbl, p_dbl]),
    "bb_solver_set_wish_from_coords": (c_int, [c_void_p, p_dbl]),
    "bb_solver_set_coords": (c_int, [c_void_p, p_dbl]),
    "bb_solver_get_coords": (c_int, [c_void_p, p_dbl]),
    "bb_solver_set_momentum": (c_int, [c_void_p, c_dbl]),
    "bb_solver_iterate": (c_int, [c_void_p, c_i64, c_dbl]),
    "bb_solver_grad": (c_int, [c_void_p]),
    "bb_solver_apply": (c_int, [c_void_p, c_dbl]),
    "bb_comm_unique_id": (c_int, [c_void_p]),
    "bb_solver_comm_init": (c_int, [c_void_p, c_void_p]),
    "bb_solver_allreduce": (c_int, [c_void_p]),
    "bb_solver_iterate_dist": (c_int, [c_void_p, c_i64, c_dbl]),
    "bb_solver_peer_export": (c_int, [c_void_p, c_void_p]),
    "bb_solver_peer_connect": (c_int, [c_void_p, c_void_p]),
    "bb_solver_iterate_peer": (c_int, [c_void_p, c_i64, c_dbl]),
    "bb_solver_peer_status": (c_int, [c_void_p, ctypes.POINTER(c_int)]),
    "bb_solver_peer_set_timeout": (c_int, [c_void_p, c_i64]),
    "bb_solver_peer_form": (c_int, [c_void_p, ctypes.POINTER(c_int)]),
    "bb_solver_peer_set_form": (c_int, [c_void_p, c_int]),
    "bb_group_create": (c_int, [ctypes.POINTER(c_void_p), ctypes.POINTER(c_void_p), c_int]),
    "bb_group_iterate": (c_int, [c_void_p, c_i64, c_dbl]),
    "bb_group_destroy": (c_int, [c_void_p]),
    "bb_solver_comm_world": (c_int, [c_void_p, ctypes.POINTER(c_int)]),
    "bb_solver_comm_abort": (c_int, [c_void_p]),
    "bb_comm_cached": (c_int, [c_int, c_int, c_int, ctypes.POINTER(c_int)]),
    "bb_comm_cached_generation": (c_int, [c_int, c_int, c_int, ctypes.POINTER(c_int),
                                          ctypes.POINTER(ctypes.c_uint64)]),
    "bb_solver_comm_attach": (c_int, [c_void_p]),
    "bb_solver_comm_detach": (c_int, [c_void_p]),
    "bb_comm_cache_clear": (c_int, []),
    "bb_solver_sync_timeout": (c_int, [c_void_p, c_i64]),
    "bb_solver_exchange_size": (c_int, [c_void_p, p_i64]),
    "bb_solver_get_exchange_buffer": (c_int, [c_void_p, ctypes.POINTER(c_void_p)]),
    "bb_solver_set_exchange_buffer": (c_int, [c_void_p, c_void_p]),
    "bb_solver_read_exchange": (c_int, [c_void_p, p_dbl, c_i64]),
    "bb_solver_write_exchange": (c_int, [c_void_p, p_dbl, c_i64]),
    "bb_solver_matvec_sq": (c_int, [c_void_p, p_dbl, p_dbl]),
    "bb_solver_spectral_init": (c_int, [c_void_p, c_int, p_dbl]),
    "bb_solver_spectral_init_tol": (c_int, [c_void_p, c_int, c_dbl, p_dbl, ctypes.POINTER(c_int), p_dbl]),
    "bb_solver_stress": (c_int, [c_void_p, p_dbl]),
    "bb_solver_get_stress_history": (c_int, [c_void_p, p_dbl, c_i64, p_i64]),
    "bb_solver_sync": (c_int, [c_void_p]),
    "bb_solver_set_timing": (c_int, [c_void_p, c_int]),
    "bb_solver_get_timing": (c_int, [c_void_p, p_dbl, p_dbl, p_i64]),
    "bb_solver_get_step_timing": (c_int, [c_void_p, p_dbl]),
    "bb_solver_measure_event_gap": (c_int, [c_void_p, c_int, p_dbl]),
    "bb_solver_measure_stream_read": (c_int, [c_void_p, c_int, p_dbl]),
    "bb_solver_iteration_path": (c_int, [c_void_p, ctypes.POINTER(c_int), ctypes.POINTER(c_int)]),
    "bb_solver_traffic": (c_int, [c_void_p, p_i64, p_i64]),
    "bb_solver_stream_info": (c_int, [c_void_p, p_i64, p_i64, p_i64, p_i64]),
    "bb_cm_create": (c_int, [ctypes.POINTER(c_void_p), c_i64, c_int]),
    "bb_cm_destroy": (c_int, [c_void_p]),
    "bb_cm_dim": (c_int, [c_void_p, p_i64]),
    "bb_cm_device_ptr": (c_int, [c_void_p, ctypes.POINTER(c_void_p), p_i64, ctypes.POINTER(c_int)]),
    "bb_cm_upload": (c_int, [c_void_p, p_dbl, c_i64]),
    "bb_cm_download": (c_int, [c_void_p, p_dbl, c_i64]),
    "bb_cm_scatter": (c_int, [c_void_p, p_dbl, c_i64, c_i32]),
    "bb_cm_scatter_ex": (c_int, [c_void_p, p_dbl, c_i64, c_i32, c_i32, p_u8,
                                 ctypes.POINTER(c_i32)]),
    "bb_cm_normalize": (c_int, [c_void_p, c_i64, p_dbl, p_dbl]),
    "bb_cm_marginals": (c_int, [c_void_p, p_dbl]),
    "bb_cm_filter": (c_int, [c_void_p, c_dbl, p_i64, p_u8]),
    "bb_cm_symv": (c_int, [c_void_p, p_dbl, p_dbl]),
    "bb_cm_eigenvector": (c_int, [c_void_p, p_dbl, p_dbl, c_dbl, c_i64, p_i64, p_dbl]),
    "bb_cm_correlation": (c_int, [c_void_p, p_dbl]),
    "bb_cm_release_scratch": (c_int, [c_int]),
    "bb_cm_shortest_paths": (c_int, [c_void_p, c_void_p, c_int, c_dbl, p_i64]),
    "bb_cm_balance": (c_int, [c_void_p, c_i64, c_i64, c_i64, c_dbl, c_i64, c_dbl, p_dbl,
                              p_u8, p_i64, p_dbl]),
    "bb_cm_expected": (c_int, [c_void_p, c_i64, p_dbl, p_dbl, p_i64]),
    "bb_triples_balance": (c_int, [c_void_p, c_i64, c_i64, c_i64, c_dbl, c_i64, c_dbl, p_dbl,
                                   p_u8, p_i64, p_dbl]),
    "bb_triples_expected": (c_int, [c_void_p, c_i64, p_dbl, p_dbl, p_i64]),
    "bb_triples_pairs": (c_int, [c_void_p, c_i64, p_i64]),
    "bb_triples_edge_degrees": (c_int, [c_void_p, c_i64, c_int, c_dbl, p_dbl, p_dbl, p_i64]),
    "bb_triples_paths": (c_int, [c_void_p, c_i64, c_int, c_dbl, p_dbl, p_dbl, p_i64, c_i64,
                                 ctypes.POINTER(c_void_p)]),
    "bb_paths_info": (c_int, [c_void_p, p_i64, p_i64, p_i64, p_i64]),
    "bb_paths_reached": (c_int, [c_void_p, p_i64]),
    "bb_paths_read": (c_int, [c_void_p, p_dbl]),
    "bb_paths_read_columns": (c_int, [c_void_p, p_i64, c_i64, p_dbl]),
    "bb_paths_place": (c_int, [c_void_p, p_dbl, p_dbl, p_dbl, p_u8]),
    "bb_paths_timing": (c_int, [c_void_p, p_dbl, p_dbl]),
    "bb_paths_destroy": (c_int, [c_void_p]),
    "bb_solver_set_anchors": (c_int, [c_void_p, c_void_p, p_u8, c_dbl]),
    "bb_solver_anchor_sums": (c_int, [c_void_p, p_dbl, c_i64]),
    "bb_solver_anchor_stress": (c_int, [c_void_p, p_dbl]),
    "bb_solver_anchor_info": (c_int, [c_void_p, p_i64, p_i64, p_i64]),
    "bb_solver_measure_anchors": (c_int, [c_void_p, c_int, p_dbl]),
    "bb_binomial_sf": (c_int, [p_i64, c_dbl, p_dbl, p_dbl, c_i64, c_int]),
    "bb_cm_significance": (c_int, [c_void_p, c_i64, c_i64, c_i64, p_dbl, c_dbl, c_dbl, p_dbl, c_dbl,
                                   ctypes.POINTER(c_void_p)]),
    "bb_triples_significance": (c_int, [c_void_p, c_i64, c_i64, c_i64, p_dbl, c_dbl, c_dbl, p_dbl,
                                        c_dbl, ctypes.POINTER(c_void_p)]),
    "bb_sig_size": (c_int, [c_void_p, p_i64, p_i64]),
    "bb_sig_read": (c_int, [c_void_p, p_i32, p_i32, p_dbl, p_dbl]),
    "bb_sig_timing": (c_int, [c_void_p, p_dbl, p_dbl]),
    "bb_sig_q_values": (c_int, [c_void_p, c_i64, p_dbl, p_dbl]),
    "bb_sig_read_q": (c_int, [c_void_p, p_dbl]),
    "bb_sig_select": (c_int, [c_void_p, c_dbl, ctypes.POINTER(c_void_p)]),
    "bb_sig_destroy": (c_int, [c_void_p]),
    "bb_cm_coarsen": (c_int, [c_void_p, c_i64, c_i64, c_int, c_void_p]),
    "bb_cm_coarsen_timing": (c_int, [c_void_p, p_dbl]),
    "bb_triples_coarsen": (c_int, [c_void_p, c_i64, c_i64, c_int, ctypes.POINTER(c_void_p)]),
    "bb_triples_coarsen_timing": (c_int, [c_void_p, p_dbl]),
    "bb_triples_size": (c_int, [c_void_p, p_i64]),
    "bb_triples_download": (c_int, [c_void_p, p_dbl]),
    "bb_cm_insulation": (c_int, [c_void_p, c_i64, c_i64, c_i64, p_dbl, p_dbl, p_i64]),
    "bb_cm_insulation_timing": (c_int, [c_void_p, p_dbl]),
    "bb_triples_insulation": (c_int, [c_void_p, c_i64, c_i64, c_i64, p_dbl, p_dbl, p_i64]),
    "bb_triples_insulation_timing": (c_int, [c_void_p, p_dbl]),
    "bb_solver_set_wish_from_cm": (c_int, [c_void_p, c_void_p, c_int, c_dbl]),
    "bb_solver_set_wish_from_cm_block": (c_int, [c_void_p, c_void_p, c_i64, c_int, c_dbl]),
    "bb_solver_set_maps": (c_int, [c_void_p, c_int, p_i64, p_dbl]),
    "bb_solver_set_wish_dense_block": (c_int, [c_void_p, p_dbl, c_i64, c_i64, c_i64, c_int, c_dbl]),
    "bb_solver_stress_maps": (c_int, [c_void_p, p_dbl, c_int]),
    "bb_solver_set_block_steps": (c_int, [c_void_p, p_dbl, c_i64]),
    "bb_solver_set_bin_steps": (c_int, [c_void_p, p_dbl, c_i64]),
    "bb_solver_degrees": (c_int, [c_void_p, p_i64, c_i64]),
    "bb_solver_set_weight_power": (c_int, [c_void_p, c_int]),
    "bb_solver_weight_sums": (c_int, [c_void_p, p_dbl, c_i64]),
    "bb_solver_score": (c_int, [c_void_p, p_dbl, p_dbl, p_dbl]),
    "bb_solver_get_score_timing": (c_int, [c_void_p, p_dbl, p_dbl, p_dbl]),
    "bb_solver_loglog": (c_int, [c_void_p, p_dbl, p_dbl]),
    "bb_solver_repower": (c_int, [c_void_p, c_dbl]),
    "bb_contactmap_scatter": (c_int, [p_dbl, c_i64, c_i32, p_dbl, c_i64, c_int]),
    "bb_contactmap_normalize": (c_int, [p_dbl, c_i64, p_dbl, p_dbl, c_int]),
    "bb_benjamini_hochberg": (c_int, [p_dbl, c_i64, c_i64, p_dbl, c_int]),
    "bb_q_values": (c_int, [p_dbl, c_i64, c_i64, p_dbl, p_i64, c_int]),
    "bb_downsample": (c_int, [ctypes.POINTER(ctypes.c_float), c_i64,
                              ctypes.POINTER(ctypes.c_float), c_i64, c_int]),
    "bb_structures_moments": (c_int, [p_dbl, p_dbl, p_u8, c_i64, c_int, p_dbl]),
    "bb_structures_compare": (c_int, [p_dbl, p_dbl, p_u8, c_i64, p_dbl, c_int,
                                      c_int, p_dbl, p_dbl, p_dbl, p_dbl, p_dbl, p_dbl]),
}

_lib = None


def load():
    """Load the shared library once; raise loudly if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "blueberry_amd: %s is missing -- build it with `python -c 'import __graft_entry__ as "
            "g; g.build()'` (or ./build.sh) at the repository root. There is no CPU fallback."
            % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)   # AttributeError here = header/library mismatch
        fn.restype = restype
        fn.argtypes = argtypes
    _lib = lib
    return lib


def hip_runtimes_loaded():
    """Paths of the libamdhip64 images mapped into this process.  More than one
    means torch's bundled HIP runtime and the system one are both live, and
    stream / event handles cannot cross between them (see solver.exchange_tensor)."""
    paths = set()
    try:
        with open("/proc/self/maps") as fh:
            for line in fh:
                if "libamdhip64" in line:
                    paths.add(line.split()[-1])
    except OSError:
        pass
    return sorted(paths)


def last_error():
    msg = load().bb_last_error()
    return msg.decode("utf-8", "replace") if msg else ""


def check(rc, what=""):
    """Turn a BB_ERR_* status into the Python exception the host API documents."""
    if rc == BB_OK:
        return
    msg = last_error() or ("%s failed (status %d)" % (what, rc))
    if rc == BB_ERR_INVALID:
        raise ValueError(msg)
    if rc == BB_ERR_NOMEM:
        raise MemoryError(msg)
    raise RuntimeError(msg)


def as_f64_ptr(arr):
    return arr.ctypes.data_as(p_dbl)


class Handle(object):
    """Owner of one library handle (`_h`, a c_void_p) whose entry points are `prefix` + name.
    The subclass names `prefix` and makes the handle with `_create`, or adopts one that another
    call returned.  `close()` (or leaving the `with` block, or the last reference going) destroys
    it; any call after that is a ValueError raised here, before C sees the NULL."""
    prefix = None                       # "bb_solver_", "bb_cm_", ...

    def __init__(self, handle=None):
        self._lib = load()
        self._h = c_void_p() if handle is None else handle

    def _create(self, *args):
        """<prefix>create(&handle, *args)."""
        name = self.prefix + "create"
        check(getattr(self._lib, name)(self._h, *args), name)

    def _open(self):
        if not self._h:
            raise ValueError("this %s handle is closed" % self.prefix[:-1])
        return self._h

    def _status(self, name, *args):
        """The status of <prefix><name>(handle, *args), for the few calls where a status other
        than BB_OK is an outcome the caller handles and not an error."""
        return getattr(self._lib, self.prefix + name)(self._open(), *args)

    def _call(self, name, *args):
        """<prefix><name>(handle, *args); any status but BB_OK raises (`check`)."""
        check(self._status(name, *args), self.prefix + name)

    def _get(self, ctype, name, *args):
        """The one scalar <prefix><name>(handle, *args, &out) writes: ctype is c_int, c_dbl
        or c_i64."""
        out = ctype()
        self._call(name, *args, out)
        return out.value

    def close(self):
        """Destroy the handle; again, or on an object whose create failed: nothing."""
        if getattr(self, "_h", None):
            getattr(self._lib, self.prefix + "destroy")(self._h)
            self._h = c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
