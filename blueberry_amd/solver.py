"""StructureSolver -- contact matrix -> 3D coordinates on MI355X.

Host side of the hot path BASELINE.json names.  The reference has no solver
(SURVEY.md section 0); the estimator shape follows the only estimator the
reference has, `FitHiC(hyper-parameters).fit_transform(data)`
(`blueberry/fithic.py:76-108`), and the input is the dense float64 matrix a
`ContactMap` holds (`blueberry/datatypes.pyx:78-86`).  The algorithm is
specified in docs/SPEC.md and runs entirely in libblueberry_hip.so
(include/blueberry_hip.h); this module is the estimator: it validates arguments,
runs the fit on an engine (engine.py) and, for world_size > 1, has exchange.py drive
one sum over the ranks per iteration (backend "nccl" = RCCL over xGMI) -- or, with
`StructureSolver(devices=[...])`, drives several GPUs from this one process without
torch (`GroupEngine`: one solver per device, one host thread each, the sum over them
ordered by HIP events, `bb_group_*`).
"""
import contextlib
import math
import os    # noqa: F401
import sys   # noqa: F401

import numpy

from . import _lib
# what this module uses, and every name it has ever had, which stays importable from it
from .compare import compare_structures
from .datatypes import (ContactMap, _nan_to_num, check_balance_args, check_coarsen_args,  # noqa: F401
                        complete_map, triples_buffer)
from .engine import (_DTYPES, _KINDS, GroupEngine, HipEngine, RankDeficient,  # noqa: F401
                     _check_coords, _square_bins)
from .exchange import (_exchange_state, allreduce_exchange, allreduce_exchange_host,  # noqa: F401
                       comm_reuse, run_iterations, select_exchange)
from .landmark import (LandmarkInfo, _check_landmark_weight, _check_n_landmarks,  # noqa: F401
                       landmark_choice, landmark_coefficients, landmark_start)
from .plan import (ALPHA_MAX, ALPHA_MIN, _check_alpha, block_degrees,  # noqa: F401
                   block_step_factors, degree_step_factors, layout_info, loglog_slope,
                   loglog_totals, max_degree, next_alpha, tiles_from_blocks, tiles_from_entries,
                   weighted_steps)
from .ranks import (all_ranks as _all_ranks, dist_state as _dist_state, gather_objects,
                    pick_device, running_job, sum_over_ranks as _sum_over_ranks)
from .triples import (DeviceTriples, GeodesicRows, TriplesBalance, _balance_options,  # noqa: F401
                      _check_triples, _resident_triples, balance_triples, coarsen_triples)


def _check_devices(devices, n_gpus, device, distributed):
    """The device list of StructureSolver(devices=, n_gpus=), validated without a GPU, or
    None when neither is given."""
    if devices is None and n_gpus is None:
        return None
    if devices is not None and n_gpus is not None:
        raise ValueError("give devices or n_gpus, not both")
    if device is not None:
        raise ValueError("give device or devices / n_gpus, not both")
    if distributed:
        raise ValueError("devices / n_gpus drive several GPUs from one process; distributed=True "
                         "runs one GPU per process")
    if n_gpus is not None:
        if isinstance(n_gpus, bool) or int(n_gpus) != n_gpus or int(n_gpus) < 1:
            raise ValueError("n_gpus must be a positive integer")
        devices = list(range(int(n_gpus)))
    devices = list(devices)
    if not devices:
        raise ValueError("devices must name at least one device")
    for d in devices:
        if isinstance(d, bool) or not isinstance(d, (int, numpy.integer)) or d < 0:
            raise ValueError("devices must be non-negative device indices, got %r" % (d,))
    if len(devices) > 16:
        raise ValueError("devices: at most 16 members")
    return [int(d) for d in devices]


def _check_complete(complete):
    """The `complete=` argument of fit / fit_many / fit_triples, checked before any device call."""
    if complete is not None and complete != "shortest_path":
        raise ValueError("complete must be None or 'shortest_path', got %r" % (complete,))


@contextlib.contextmanager
def _teardown(eng):
    """Close the engine when the fit ends, however it ends."""
    try:
        yield
    except BaseException:
        # this rank leaves a multi-rank job in the middle: its peers may sit in a collective
        # on the library's communicator, which must then not go back into the cache for the
        # next fit() to borrow (close() would return it as free)
        if _exchange_state(eng) == "rccl" and hasattr(eng, "comm_abort"):
            try:
                eng.comm_abort()
            except Exception:                  # noqa: BLE001 -- the first error is the one to report
                pass
        raise
    finally:
        eng.close()


class FitScore(object):
    """How well a structure fits a map, from the device's sums (SPEC 2.8, `StructureSolver.score`).

    sums : (n_bins, 9) float64, row k = the constrained pairs of separation j - i = k: pairs,
        sum d, sum delta, sum d^2, sum delta^2, sum d delta, sum (d - delta)^2,
        sum (d - delta)^2 / delta, sum ((d - delta) / delta)^2
    bin_sums : (n_bins, 3) float64, row i = the pairs that hold bin i: pairs, sum (d - delta)^2,
        sum ((d - delta) / delta)^2

    Derived on the host in float64:
    n_pairs : the constrained pairs
    stress : array of 3, S_q of SPEC 2.3.1 for q = 0, 1, 2 -- comparable between fits made
        with different weight_power
    normalized_stress : stress[0] / sum delta^2
    pearson : Pearson r of (d, delta) over the pairs; NaN with fewer than 2 pairs or no variance
    pairs, mean_distance, mean_wish, rms_relative_error : per separation k (int64; the others
        NaN where pairs == 0); rms_relative_error = sqrt(mean ((d - delta) / delta)^2)
    bin_pairs, bin_stress, bin_relative : per bin: its pairs (int64), its sum (d - delta)^2
        (every pair counts at both of its bins: the bins add up to 2 stress[0]) and the rms
        relative error of its pairs (NaN for a bin without pairs)
    """

    def __init__(self, sums, bin_sums):
        self.sums = numpy.ascontiguousarray(sums, dtype=numpy.float64)
        self.bin_sums = numpy.ascontiguousarray(bin_sums, dtype=numpy.float64)
        if self.sums.ndim != 2 or self.sums.shape[1] != 9 or self.bin_sums.shape != (self.sums.shape[0], 3):
            raise ValueError("FitScore: sums must be (n_bins, 9) and bin_sums (n_bins, 3)")
        tot = self.sums.sum(axis=0)
        n, sd, sw, sdd, sww, sdw = (float(v) for v in tot[:6])
        self.n_pairs = int(round(n))
        self.stress = tot[6:9].copy()
        self.normalized_stress = float(tot[6] / sww) if sww > 0 else float("nan")
        # (a variance the rounding of its own sums could have made counts as none: each of the
        # moments is good to n 2^-53 of itself)
        var_d, var_w, noise = n * sdd - sd * sd, n * sww - sw * sw, 8.0 * n * n * 2.0 ** -53
        self.pearson = (float((n * sdw - sd * sw) / numpy.sqrt(var_d * var_w))
                        if self.n_pairs >= 2 and var_d > noise * sdd and var_w > noise * sww
                        else float("nan"))

        def per(total, count):
            return numpy.where(count > 0, total / numpy.where(count > 0, count, 1.0), numpy.nan)
        cnt = self.sums[:, 0]
        self.pairs = numpy.rint(cnt).astype(numpy.int64)
        self.mean_distance = per(self.sums[:, 1], cnt)
        self.mean_wish = per(self.sums[:, 2], cnt)
        self.rms_relative_error = numpy.sqrt(per(self.sums[:, 8], cnt))
        self.bin_pairs = numpy.rint(self.bin_sums[:, 0]).astype(numpy.int64)
        self.bin_stress = self.bin_sums[:, 1].copy()
        self.bin_relative = numpy.sqrt(per(self.bin_sums[:, 2], self.bin_sums[:, 0]))

    def __repr__(self):
        return ("FitScore(n_pairs=%d, stress=%s, normalized_stress=%.6g, pearson=%.6g)"
                % (self.n_pairs, numpy.array2string(self.stress, precision=6),
                   self.normalized_stress, self.pearson))


class StructureSolver(object):
    """Infer 3D bin coordinates from a Hi-C contact matrix (metric MDS).

    Minimises  S(X) = sum_{i<j, c_ij>0} (|x_i - x_j| - delta_ij)^2  with
    delta_ij = c_ij^(-1/alpha), by `n_iter` gradient steps  X <- X - lr * grad S
    (docs/SPEC.md).  With lr = 1/(2 N) and a complete matrix each step equals a
    SMACOF / Guttman-transform step, so the stress never increases.

    Parameters
    ----------
    n_iter : int
        Number of iterations (fixed; there is no convergence test on the device).
    lr : float or 'auto'
        Step size; 'auto' = 1 / (2 * n_bins).
    dtype : 'float32' or 'float64'
        Arithmetic type on the GPU.
    alpha : float, 'auto', ('auto', alpha0), ('auto', alpha0, max_rounds) or
            ('auto', alpha0, max_rounds, tol)
        Count-to-distance exponent, delta = c^(-1/alpha).  'auto' infers it in the fit (SPEC
        2.11): after `n_iter` iterations at alpha0 (3.0) the log-log slope p of fitted on wish
        distance is taken on the device; while |p - 1| > tol (1e-3) and fewer than max_rounds
        (8) rounds have run, the next exponent comes from a secant step on (ln alpha, ln p),
        the resident wish distances are re-exponentiated in place, the structure is rescaled
        and `n_iter` iterations run again.  Then the map is packed once more at `alpha_` and
        `n_iter` iterations run from `alpha_init_`: `structure_` and `stress_` are bit for bit
        those of StructureSolver(alpha=alpha_, ...).fit(X, init=alpha_init_).  The options ride
        in `alpha` (stored normalised; `alpha_start`, `alpha_rounds`, `alpha_tol` read them
        back) so that clones carry them.  For every input of `fit` and `fit_triples`
        (`balance=`, `devices=`, a distributed world: every rank takes the same alpha); `score`
        then uses `alpha_` (ValueError before a fit).  ValueError with kind='wish' (no counts),
        complete='shortest_path' and init='landmark' (distances that are sums along paths
        cannot be re-exponentiated) and for `fit_many`; ValueError for a map with fewer than 3
        usable pairs or whose counts do not vary; RuntimeError when a slope is <= 0 or a round's
        coordinates are not finite (the fit diverged).  Exact on
        noise-free maps; on Poisson-sampled counts whose zero cells are dropped the estimate is
        biased upwards (3.27 for a true 3; 3.58 with weight_power=2): the zeros are truncated
        and the estimator has no model for them.
    kind : 'counts' or 'wish'
        Whether the input matrix holds contact counts or wish distances.
    seed : int
        Seed of the default initial coordinates (numpy default_rng standard normal).
    tol : float or None
        None: exactly n_iter steps.  Otherwise stop as soon as the relative stress
        decrease of one step is <= tol, checked every `check_every` steps (n_iter is
        then the maximum); `n_iter_` tells how many were run.
    init : 'random', 'spectral', 'landmark', ('landmark', n_landmarks) or
           ('landmark', n_landmarks, landmark_weight)
        Start used when `fit()` gets no `init=` array: seeded standard normal, or
        classical MDS computed on the device (`spectral_init`), or -- for the sparse inputs,
        `fit_triples` and `fit(scipy.sparse)` -- landmark MDS over shortest paths on the stored
        pairs (`landmark_start`, SPEC 2.5.4), which gives a map with counts only between nearby
        bins its global fold without the dense matrix.  'landmark' takes 64 landmarks; the
        tuple form another number, an int in [4, 1024] (`n_landmarks` reads it back; it is part
        of `init` and not a constructor argument of its own, so that clones carry it).  The
        start is computed once, on devices[0] of `devices=` or on the rank's own device, under
        this solver's kind and alpha and the bias the fit uses (KR vectors, `balance=`), and
        handed to the unchanged fit as `init=`; `landmarks_` and `landmark_placed_` tell which
        bins were landmarks and which were placed.  Not for dense inputs or a ContactMap
        (`complete='shortest_path'` is their route, or init='spectral'), not with
        `complete='shortest_path'`, `fit_many`, or an engine without a device: ValueError.
        The stored pairs alone do not hold the fold for ever (SPEC 2.5.4): few iterations, or
        ('landmark', n_landmarks, landmark_weight) with landmark_weight > 0 (SPEC 2.5.5): the
        kept landmarks' geodesic rows stay in the fit as constraints, every term weighted
        landmark_weight * D^-weight_power, and hold the fold over any number of iterations
        (`landmark_weight` reads it back; 0, the default, is the fit without them bit for bit).
        It needs degree_steps=True (a landmark touches about N terms: ValueError otherwise) and
        ONE device (`devices=` / `n_gpus` of several, a distributed world > 1: ValueError);
        `stress_` is then the total of stored pairs and landmark terms, `anchor_stress_` the
        latter's share at the end, `landmark_terms_` their number.  An `init=` array given to
        the call replaces the start only; the constraints stay.  The anchored fit reduces the
        stress of the stored pairs less than the free one.
    degree_steps : bool
        A step per bin from the map itself (SPEC 2.4.1): bin i steps by 1 / (2 (deg_i + 1)),
        deg_i = the number of pairs that constrain it (counted on the device, summed over
        the ranks), instead of one step for all (`lr='auto'`: 1 / (2 N), the step of a
        COMPLETE map).  For incomplete maps -- blocked-sparse input, a whole genome whose
        chromosomes differ in size, real maps whose long-range pairs have no contact -- that
        is each bin's own Guttman-like step: a genome-like map converges in about a third
        of the iterations.  A float `lr` is then the step of the bin with the most partners.
        A complete map: no effect.  With weight_power > 0 the weighted degree
        s_i = sum_j delta_ij^-q takes the place of deg_i: bin i steps by 1 / (2 s_i).
    weight_power : 0, 1 or 2
        Weight w = delta^-q of each pair's squared residual (SPEC 2.3.1).  0: raw stress, where
        the long-range pairs (largest, noisiest delta) dominate.  1: Sammon stress, a middle
        ground.  2: relative stress, sum ((d - delta) / delta)^2, every pair's relative error
        counts alike -- the local structure, the best-measured part of a Hi-C map, gets its
        share.  With q > 0, lr='auto' is 1 / (2 max_i s_i), s_i the weighted degree; `stress_`
        reports the weighted stress.  float32 refuses (ValueError) a map whose largest s_i
        exceeds 2^60.
    spectral_iter, spectral_tol : int, float
        The spectral start's block power iteration makes at most `spectral_iter` products
        and ends once B V lies within `spectral_tol` (relative) of span(V); 0 = always
        `spectral_iter` products.  `spectral_iterations_` tells how many were made.
    momentum : float in [0, 1)
        Heavy-ball coefficient mu: V <- mu V - lr g, X <- X + V.  0 = plain steps.
    device : int or None
        HIP device index; None = LOCAL_RANK (distributed) or 0.
    devices : list of int or None
        Several GPUs driven from THIS process, no torch.distributed job needed: member r of
        the group plays rank r of world len(devices) on devices[r], packs only its own units
        from the one input, and a host thread per member enqueues its iterations; the
        partials are summed in rank order by an exchange ordered with HIP events
        (`GroupEngine`, `bb_group_*`), bit-identical to the process-per-rank peer exchange
        (two-launch form) at the same world size.  One entry: as `device=`.  A device may
        repeat -- members then take turns on it: a rehearsal, the one form a one-GPU box can
        run.  Not with `device`, `n_gpus`, `distributed=True` or inside a torch.distributed
        job; not for `fit_many`.
    n_gpus : int or None
        Shorthand for devices=list(range(n_gpus)).
    distributed : bool or None
        None: shard over the ranks of an initialised torch.distributed job if
        there is one.  Every rank passes the same matrix and gets the same result.

    Attributes
    ----------
    structure_ : numpy.ndarray, shape (n_bins, 3), float64
    stress_ : numpy.ndarray, shape (n_iter,) -- stress BEFORE each step
    n_bins_, lr_ : the problem size and the step actually used
    exchange_ : how the ranks summed their partial gradients ('rccl', 'peer', 'torch',
        'host', 'group' for devices=), None on one rank.  Results are reproducible bit for
        bit for a given transport; fit() never picks one by timing (that is bench.py's trial).
    devices_ : the devices of a `devices=` / `n_gpus=` fit, member by member; else None.
    alpha_ : the exponent of the fit: the inferred one under alpha='auto', else `alpha`.
    alpha_rounds_ : (rounds, 5) float64, per round of the search alpha_r, the slope p_r, the
        intercept a_r, the log-log correlation, the iterations run; (0, 5) for a float alpha.
    alpha_converged_ : whether the search ended by |p - 1| <= tol (True for a float alpha).
    alpha_init_ : (n_bins, 3), the start of the last fit under 'auto'; None for a float alpha.

    Failure on several ranks.  A rank that fails mid-fit raises, and takes the library's
    communicator out of the cache (its peers may still sit in a collective on it).  With
    the peer exchange ('peer', BB_COMM=peer or a trial) in its one-launch form every wave
    decides for its own 64 coordinates, so a rank that dies IN THE MIDDLE of an exchange can
    leave its peers with part of a step applied: their fit() then raises too
    (`peer_status`), and the coordinates of a solver that raised are not a result.  Nothing
    of a rank that is late or gone ever arrives, so nothing is applied; the two-launch form
    (ranks sharing a GPU, BB_PEER_FUSED=0) applies a step whole or not at all.
    """

    def __init__(self, n_iter=100, lr="auto", dtype="float32", alpha=3.0, kind="counts",
                 seed=0, device=None, distributed=None, engine=None, momentum=0.0,
                 init="random", tol=None, check_every=10, spectral_iter=40, spectral_tol=1e-3,
                 degree_steps=False, weight_power=0, devices=None, n_gpus=None):
        if dtype not in _DTYPES:
            raise ValueError("dtype must be 'float32' or 'float64'")
        if kind not in _KINDS:
            raise ValueError("kind must be 'counts' or 'wish'")
        if int(n_iter) < 0:
            raise ValueError("n_iter must be >= 0")
        if int(n_iter) > (1 << 20):
            raise ValueError("n_iter is limited to 2**20: the per-iteration stress history "
                             "lives on the device (include/blueberry_hip.h, bb_solver_iterate)")
        if not (lr == "auto" or float(lr) > 0):
            raise ValueError("lr must be positive or 'auto'")
        alpha = _check_alpha(alpha)
        if isinstance(alpha, tuple):
            if kind == "wish":
                raise self._auto_refusal("infers the exponent of counts: kind='wish' holds wish "
                                         "distances, which have none")
            if init == "landmark" or (isinstance(init, tuple) and init[:1] == ("landmark",)):
                raise self._auto_refusal("does not go with init='landmark': the landmark start and "
                                         "its geodesic rows are made of the wish distances of one "
                                         "alpha, which the search changes")
        if not 0.0 <= float(momentum) < 1.0:
            raise ValueError("momentum must be in [0, 1)")
        self.momentum = float(momentum)
        if tol is not None and not float(tol) > 0:
            raise ValueError("tol must be positive or None")
        if int(check_every) < 1:
            raise ValueError("check_every must be >= 1")
        self.tol, self.check_every = (None if tol is None else float(tol)), int(check_every)
        if isinstance(init, tuple) and len(init) in (2, 3) and init[0] == "landmark":
            init = ("landmark", _check_n_landmarks(init[1])) + tuple(
                _check_landmark_weight(w) for w in init[2:])
        elif not (isinstance(init, str) and init in ("random", "spectral", "landmark")):
            raise ValueError("init must be 'random', 'spectral', 'landmark', ('landmark', "
                             "n_landmarks) or ('landmark', n_landmarks, landmark_weight) (or pass "
                             "init= to fit())")
        self.init = init
        if int(spectral_iter) < 0 or not 0.0 <= float(spectral_tol) < 1.0:
            raise ValueError("need spectral_iter >= 0 and 0 <= spectral_tol < 1")
        self.spectral_iter, self.spectral_tol = int(spectral_iter), float(spectral_tol)
        self.degree_steps = bool(degree_steps)
        if isinstance(weight_power, bool) or weight_power not in (0, 1, 2):
            raise ValueError("weight_power must be 0, 1 or 2")
        self.weight_power = int(weight_power)
        self.n_iter, self.lr, self.dtype, self.alpha, self.kind, self.seed = (
            int(n_iter), lr, dtype, alpha, kind, int(seed))
        self.device, self.distributed = device, distributed
        # Engine factory: the HIP engine unless a test injects another one to
        # rehearse the multi-rank orchestration without a GPU.
        self._engine_factory = engine if engine is not None else HipEngine
        self.devices, self.n_gpus = devices, n_gpus
        self._group = _check_devices(devices, n_gpus, device, distributed)
        if self._group is not None and len(self._group) == 1:
            self.device = self._group[0]           # one entry: as device=
        elif self._group is not None and engine is not None:
            raise ValueError("devices= runs HIP engines of its own; it takes no engine=")
        self._anchor = None                 # (rows, kept) between the landmark start and the fit
        if self.landmark_weight > 0.0:
            if not self.degree_steps:
                raise ValueError("landmark_weight > 0 needs degree_steps=True: a landmark touches "
                                 "about landmark_weight * N terms, so the one global step its "
                                 "weighted degree allows, 1 / (2 landmark_weight N), would slow "
                                 "every bin down to it (docs/SPEC.md 2.5.5)")
            self._check_anchor_devices(None)

    def _pick_device(self, world):
        return pick_device(self.device, world > 1)

    @staticmethod
    def _auto_refusal(why):
        return ValueError("alpha='auto' %s; give a float alpha" % why)

    @property
    def alpha_auto(self):
        """Whether the exponent is inferred in the fit (alpha='auto' in any form, SPEC 2.11)."""
        return isinstance(self.alpha, tuple)

    @property
    def alpha_start(self):
        """alpha0 of alpha=('auto', alpha0, ...) (3.0 for 'auto'); a float alpha: that alpha."""
        return self.alpha[1] if self.alpha_auto else self.alpha

    @property
    def alpha_rounds(self):
        """max_rounds of alpha=('auto', alpha0, max_rounds, ...) (8); None for a float alpha."""
        return self.alpha[2] if self.alpha_auto else None

    @property
    def alpha_tol(self):
        """tol of alpha=('auto', alpha0, max_rounds, tol) (1e-3); None for a float alpha."""
        return self.alpha[3] if self.alpha_auto else None

    def _pack_alpha(self):
        """The exponent a map is packed under outside a search: the float alpha, or alpha_ of
        the last 'auto' fit (ValueError before one)."""
        if not self.alpha_auto:
            return self.alpha
        if getattr(self, "alpha_", None) is None:
            raise ValueError("alpha='auto': no exponent inferred yet (alpha_ is set by a fit)")
        return self.alpha_

    @property
    def n_landmarks(self):
        """The landmarks of init='landmark' (64) / ('landmark', n); None for another init."""
        if self.init == "landmark":
            return 64
        return self.init[1] if isinstance(self.init, tuple) else None

    @property
    def landmark_weight(self):
        """The weight of the landmark constraints (SPEC 2.5.5): the third entry of
        init=('landmark', n_landmarks, landmark_weight); 0.0 (none) for every other init."""
        return self.init[2] if isinstance(self.init, tuple) and len(self.init) == 3 else 0.0

    def _landmark_refusal(self, why, instead):
        return ValueError("init='landmark' %s; use %s" % (why, instead))

    def _check_anchor_devices(self, world):
        """Landmark constraints (landmark_weight > 0) run on one device: a group of several, or
        -- `world` given -- a torch.distributed job of several ranks, is refused."""
        if self.landmark_weight > 0.0 and ((self._group is not None and len(self._group) > 1)
                                           or (world is not None and world > 1)):
            raise self._landmark_refusal("with landmark_weight > 0 keeps its constraints on one "
                                         "device (several devices are not covered)",
                                         "one device, or landmark_weight = 0")

    def _check_landmark_route(self, complete):
        """The refusals of a landmark start that need no device (the caller has a sparse input)."""
        if complete is not None:
            raise self._landmark_refusal("does not go with complete='shortest_path', which "
                                         "determines the fold itself", "init='random' or 'spectral'")
        if not hasattr(self._engine_factory, "set_wish_triples"):
            raise self._landmark_refusal("runs on the device and this solver's engine has none",
                                         "init='spectral'")
        if self.landmark_weight > 0.0:
            self._check_anchor_devices(1 if self._group is not None else _dist_state(self.distributed)[1])

    def _landmark_wanted(self, init):
        """Whether a call with this `init=` goes the landmark route: for the start (no init
        given), and -- an array replaces only the start -- for the constraints."""
        return self.n_landmarks is not None and (init is None or self.landmark_weight > 0.0)

    def _landmark_init(self, dev, n_bins, KRnorm, KRexpected):
        """The landmark start of the map in `dev` (a DeviceTriples) under this solver's kind and
        alpha and the fit's KR vectors; `landmarks_` and `landmark_placed_` stay on the solver.
        With landmark_weight > 0 the geodesic rows stay open for the fit (`_anchor`), which hands
        them to its engine and closes them."""
        keep = self.landmark_weight > 0.0
        self._drop_anchor()
        start, info = landmark_start(dev, dev.resolution, n_bins, n_landmarks=self.n_landmarks,
                                     kind=self.kind, alpha=self.alpha, KRnorm=KRnorm,
                                     KRexpected=KRexpected, seed=self.seed, return_info=True,
                                     keep_rows=keep)
        self.landmarks_, self.landmark_placed_ = info.landmarks_, info.placed_
        if keep:
            self._anchor = (info.rows_, info.kept_)
        return start

    def _drop_anchor(self):
        if self._anchor is not None:
            self._anchor[0].close()
            self._anchor = None

    def _take_anchor(self, eng, world):
        """The rows `_landmark_init` kept, copied into the engine (which then owns its copy)
        and closed."""
        if self._anchor is None:
            return
        try:
            self._check_anchor_devices(world)
            if not hasattr(eng, "set_anchors"):
                raise self._landmark_refusal("with landmark_weight > 0 needs an engine that holds "
                                             "the constraints on the device", "HipEngine")
            eng.set_anchors(self._anchor[0], self._anchor[1], self.landmark_weight)
        finally:
            self._drop_anchor()

    def fit(self, X, init=None, complete=None):
        """Solve for the structure of `X`: a ContactMap, a square ndarray, or a
        scipy.sparse matrix (symmetric; either triangle is enough; of several
        COO entries for one pair the last is kept) -- the sparse form never builds
        the dense matrix.

        complete : None or 'shortest_path'
            None: pairs without a contact are no constraint (SPEC 2.1).  'shortest_path': the
            map is first completed on the device by graph shortest paths over its wish
            distances (SPEC 2.1.1, `ContactMap.shortest_paths` with this solver's `kind` and
            `alpha`) -- what a real Hi-C map, with counts only between nearby bins, needs for
            its global fold to be determined -- and the fit is that of
            `StructureSolver(kind='wish', ...).fit(completed)`, dense tiles, bit for bit.
            `completed_unreachable_pairs_` tells how many pairs stayed without a path.  With
            `devices=[...]` the completion runs once on devices[0]; inside a torch.distributed
            job every rank completes the same input on its own GPU.  The dense matrix and a
            work matrix of its size must fit on one device: a whole-genome blocked-sparse map
            (720 GB dense at 10 kb) cannot be completed this way (MemoryError); init='landmark'
            (SPEC 2.5.4) is the route of such a map to its global fold."""
        _check_complete(complete)
        self._check_auto_route(complete)
        if self._landmark_wanted(init):
            try:
                start = self._landmark_init_of_map(X, complete)
                source, n = self._map_source(X)
                return self._fit_impl(source, n, start if init is None else init, None, None)
            finally:
                self._drop_anchor()
        if complete is None:
            source, n = self._map_source(X)
            return self._fit_impl(source, n, init, None, None)
        cm = self._completed(X)
        self.completed_unreachable_pairs_ = cm.unreachable_pairs_
        source, n = self._map_source(cm)
        return self._fit_impl(source, n, init, None, None, kind="wish")

    def _check_auto_route(self, complete):
        if self.alpha_auto and complete is not None:
            raise self._auto_refusal("does not go with complete='shortest_path': the completed "
                                     "distances are sums along paths, not a power of a count, so "
                                     "they cannot be re-exponentiated")

    def _landmark_init_of_map(self, X, complete):
        """fit(X) under init='landmark': the start of a scipy.sparse X, whose COO entries are the
        triples [row, col, value] at resolution 1 over N - 1 bins (an entry that is not finite is
        no constraint there and no edge here); any other input is refused."""
        matrix = X if hasattr(X, "tocoo") else None     # (a ContactMap's matrix is never read)
        if matrix is None:
            raise self._landmark_refusal("needs a sparse input (fit_triples, or fit of a "
                                         "scipy.sparse matrix), not a dense array or a ContactMap",
                                         "complete='shortest_path' or init='spectral'")
        self._check_landmark_route(complete)
        coo = matrix.tocoo()
        n = _square_bins(coo.shape)
        vals = numpy.asarray(coo.data, dtype=numpy.float64)
        triples = numpy.stack([coo.row.astype(numpy.float64), coo.col.astype(numpy.float64),
                               numpy.where(numpy.isfinite(vals), vals, 0.0)], axis=1)
        with _resident_triples(triples, 1, [self._completion_device()]) as dev:
            return self._landmark_init(dev, n - 1, None, None)

    def _completion_device(self):
        """Where a fit's completion runs: devices[0] of a group, else this rank's device."""
        devices = self._group_devices()
        if devices:
            return devices[0]
        return self._pick_device(_dist_state(self.distributed)[1])

    def _completed(self, X, device=None):
        """The shortest-path completion of one input map under this solver's kind and alpha,
        as a resident ContactMap of wish distances."""
        return complete_map(X, kind=self.kind, alpha=self.alpha,
                            device=self._completion_device() if device is None else device)

    # -- the stages fit() and fit_many() share -----------------------------------------
    def _map_source(self, X, sparse=True):
        """(source, n_bins) of one input map.  source is X itself for a ContactMap whose
        matrix lives in HBM (packed device to device; only its shape is read), a COO matrix
        for scipy.sparse input (`sparse` false -- fit_many, which packs dense blocks -- takes
        it as an array), else the host matrix as an ndarray."""
        if getattr(X, "is_resident", False) and hasattr(self._engine_factory, "set_wish_from_cm"):
            return X, _square_bins(X.shape)
        matrix = getattr(X, "matrix", X)
        if sparse and hasattr(matrix, "tocoo"):    # any scipy.sparse matrix
            matrix = matrix.tocoo()
        else:
            matrix = numpy.asarray(matrix)
        return matrix, _square_bins(matrix.shape)

    def _default_start(self, n):
        return numpy.random.default_rng(self.seed).standard_normal((n, 3))

    def _one_step(self, n):
        """The one step for all bins of a map of n bins: lr='auto' is SPEC 2.4's 1 / (2 n)."""
        return 1.0 / (2.0 * n) if self.lr == "auto" else float(self.lr)

    def _fitted(self, structure, who):
        """`structure`, or `structure_` of the last fit where none is given (ValueError before one)."""
        if structure is None:
            structure = getattr(self, "structure_", None)
            if structure is None:
                raise ValueError("%s: no structure given and none fitted yet (structure_)" % who)
        return structure

    def _bin_sums(self, eng, world):
        """What the per-bin steps of SPEC 2.4.1 are made from, summed over the ranks: the
        weighted degrees (weight_power, which is switched on here), the degrees
        (degree_steps), or None for the one step of SPEC 2.4."""
        if self.weight_power:
            eng.set_weight_power(self.weight_power)
            sums = _sum_over_ranks(eng.weight_sums(), eng, world)
        elif self.degree_steps:
            sums = _sum_over_ranks(eng.degrees(), eng, world)
        else:
            return None
        if getattr(eng, "anchored", False):
            # SPEC 2.5.5: the landmark terms join the (weighted) degrees, as float64
            sums = numpy.asarray(sums, dtype=numpy.float64) + eng.anchor_sums()
        return sums

    def _steps(self, sums, n, anchored=False):
        """(lr, scale) for one map of n bins from its slice of `_bin_sums`: `weighted_steps`
        (weighted stress, or `anchored`: the sums hold landmark terms, SPEC 2.5.5) or
        `degree_step_factors`, a float `lr` being the step of the best-connected bin."""
        if self.weight_power or anchored:
            return weighted_steps(sums, n, self.dtype, self.lr, self.degree_steps)
        lr, scale = degree_step_factors(sums)
        return (lr if self.lr == "auto" else float(self.lr)), scale

    def _iterate(self, step, history, converged):
        """`n_iter` iterations through step(k).  With `tol` (early stop) they go in chunks
        of `check_every`: after each the stress history is read back (one sync) and the
        loop ends once converged(history()).  Every rank sees the same all-reduced stress,
        so all ranks stop at the same iteration."""
        if self.tol is None:
            step(self.n_iter)
            return
        done = 0
        while done < self.n_iter:
            k = min(self.check_every, self.n_iter - done)
            step(k)
            done += k
            if converged(history()):
                break

    def _params(self):
        """Every argument of the constructor as this solver holds it now."""
        import inspect
        p = {k: getattr(self, k) for k in inspect.signature(type(self).__init__).parameters
             if k not in ("self", "engine")}
        p["engine"] = None if self._engine_factory is HipEngine else self._engine_factory
        if self._group is not None:
            p["device"] = None                     # (set from a one-entry devices=)
        return p

    def _clone(self, **overrides):
        """A solver with this one's parameters, but for `overrides`."""
        return type(self)(**dict(self._params(), **overrides))

    def _fit_impl(self, matrix, n, init, KRnorm, KRexpected, kind=None):
        kind = self.kind if kind is None else kind      # 'wish' for a completed map
        eng, world, devices, pack = self._engine_for(matrix, n)
        lr = self._one_step(n)
        if init is None and self.init == "random":
            init = self._default_start(n)
        auto = self.alpha_auto
        if auto and not (hasattr(eng, "loglog") and hasattr(eng, "repower")):
            eng.close()
            raise self._auto_refusal("needs an engine with the log-log pass and the "
                                     "re-exponentiation (HipEngine)")
        with _teardown(eng):
            pack(kind, KRnorm, KRexpected, self.alpha_start)
            self._take_anchor(eng, world)
            anchored = bool(getattr(eng, "anchored", False))
            sums = self._bin_sums(eng, world)
            if sums is not None:
                lr, scale = self._steps(sums, n, anchored)
                if scale is not None:
                    eng.set_bin_steps(scale)
            on_device = False
            if init is None:
                # 'spectral'.  The whole block power iteration stays on the device -- on one
                # rank, and on several once they have their exchange (peer arenas or the
                # library's communicator: the per-rank products are then summed where they
                # are).  Its Cholesky-QR needs an iterate of full column rank; maps it cannot
                # take -- fewer than 4 bins (centring leaves at most 2 directions), an empty
                # or unconstrained map -- and transports that sum on the host (gloo, torch)
                # go through the host-driven form below, so the same input runs everywhere.
                v0 = self._default_start(n)
                if world > 1:
                    eng.set_coords(v0)             # (a trial in select_exchange wants a start)
                    select_exchange(eng, lr)
                device_form = hasattr(eng, "spectral_init_device") and n >= 4 and (
                    world == 1 or _exchange_state(eng) in ("peer", "rccl"))
                if device_form:
                    try:
                        info = eng.spectral_init_device(self.spectral_iter, v0, tol=self.spectral_tol)
                        self.spectral_iterations_ = info[0] if info else self.spectral_iter
                        on_device = True
                    except RankDeficient:
                        pass
                    if world > 1:
                        if _exchange_state(eng) == "peer":
                            eng.peer_status()
                        on_device = _all_ranks(on_device)
            if not on_device:
                if init is None:                   # 'spectral', host-driven
                    init, self.spectral_iterations_ = spectral_init(
                        eng, n, world, n_iter=self.spectral_iter, seed=self.seed,
                        tol=self.spectral_tol, return_iterations=True)
                eng.set_coords(init)
            if self.momentum:
                eng.set_momentum(self.momentum)
            if world > 1:
                select_exchange(eng, lr)
            # converged: the relative decrease of the last step is <= tol (never at stress 0)
            def run(lr):
                self._iterate(lambda k: run_iterations(eng, k, lr, world), eng.stress_history,
                              lambda h: h.size >= 2 and h[-2] > 0
                              and abs(h[-2] - h[-1]) <= self.tol * h[-2])
            run(lr)
            if auto:
                lr = self._alpha_search(eng, world, n, run, lambda a: pack(kind, KRnorm, KRexpected, a))
            else:
                self.alpha_, self.alpha_rounds_ = self.alpha, numpy.zeros((0, 5))
                self.alpha_converged_, self.alpha_init_ = True, None
            if _exchange_state(eng) == "peer":
                eng.peer_status()              # raises if a peer wait ran into its time limit
            self.exchange_ = _exchange_state(eng)
            self.structure_ = eng.get_coords()
            self.stress_ = eng.stress_history()
            if self.n_landmarks is not None:
                self.anchor_stress_ = eng.anchor_stress() if anchored else 0.0
                self.landmark_terms_ = eng.anchor_info()[1] if anchored else 0
        self.devices_ = devices
        self.n_bins_, self.lr_, self.n_iter_ = n, lr, int(self.stress_.shape[0])
        return self

    def _engine_for(self, matrix, n):
        """The engine one input map runs on, the map not yet in it: (eng, world, devices, pack).
        pack(kind, KRnorm, KRexpected) packs the map as the form of `matrix` asks -- resident
        ContactMap, device triples, scipy.sparse (blocked-sparse: only the tiles that hold an
        entry exist on the device) or a host matrix.  The caller closes the engine."""
        resident = getattr(matrix, "is_resident", False)
        triples = getattr(matrix, "is_triples", False)
        sparse = hasattr(matrix, "row") and not resident
        if n < 2:
            raise ValueError("need at least 2 bins (the contact map is empty)" if n == 0 else
                             "need at least 2 bins")
        devices = self._group_devices()                 # checked for one entry as well
        group = devices if devices and len(devices) > 1 else None
        rank, world = (0, 1) if devices else _dist_state(self.distributed)
        tiles = None
        if sparse:
            keep = matrix.row != matrix.col
            rows, cols, vals = matrix.row[keep], matrix.col[keep], matrix.data[keep]
            tiles = tiles_from_entries(n, rows, cols, self.dtype)
        elif triples:
            tiles = matrix.tiles(n, self.dtype)
        if group:
            eng = GroupEngine(n, self.dtype, group, tiles=tiles)
        else:
            eng = self._engine_factory(n, self.dtype, rank=rank, world=world,
                                       device=self._pick_device(world), tiles=tiles)

        def pack(kind, KRnorm, KRexpected, alpha=None):
            alpha = self._pack_alpha() if alpha is None else alpha
            if resident:
                eng.set_wish_resident(matrix, kind, alpha)
            elif triples:
                eng.set_wish_triples(matrix, kind, alpha, KRnorm, KRexpected)
            elif sparse:
                eng.set_wish_sparse(rows, cols, vals, kind, alpha, KRnorm, KRexpected)
            else:
                eng.set_wish_dense(matrix, kind, alpha)
        return eng, world, devices, pack

    def _alpha_search(self, eng, world, n, run, pack_at):
        """SPEC 2.11 on the engine of a fit whose round 0 (packed at alpha_start, `n_iter`
        iterations from the fit's start) has just run: the rounds of the search -- log-log sums,
        slope, next exponent, the units re-exponentiated on the device, the structure rescaled
        -- and then the fit proper at alpha_: the map packed once more from the input by
        pack_at(alpha), the steps recomputed, `n_iter` iterations from alpha_init_.  run(lr)
        iterates; returns the lr of that last fit.  Every rank takes the same decisions: the
        sums are the same on all of them."""
        def steps():
            lr = self._one_step(n)
            sums = self._bin_sums(eng, world)
            if sums is not None:
                lr, scale = self._steps(sums, n)
                eng.set_bin_steps(scale)            # (None: one step for all again)
            return lr
        _, alpha, max_rounds, tol = self.alpha
        rounds, converged = [], False
        while True:
            x = eng.get_coords()
            if not numpy.isfinite(x).all():
                # (a distance that is not a number has no logarithm either: the sums would count
                # it with the pairs at d = 0 and the slope would speak of too few pairs)
                raise RuntimeError("alpha='auto': the fit diverged in round %d at alpha = %.6g (its "
                                   "coordinates are not finite): a smaller lr, or a fixed alpha"
                                   % (len(rounds), alpha))
            iters = int(eng.stress_history().shape[0])
            totals =_sum_over_ranks(loglog_totals(eng.loglog()), eng, world)
            p, a, r_log, ubar, vbar = loglog_slope(totals)
            rounds.append((alpha, p, a, r_log, float(iters)))
            converged = abs(p - 1.0) <= tol
            if converged or len(rounds) == max_rounds:
                break
            nxt = next_alpha(rounds)
            power = alpha / nxt
            eng.repower(power)
            lr = steps()
            eng.set_coords(math.exp(power * ubar - vbar) * x)
            alpha = nxt
            run(lr)
        self.alpha_, self.alpha_converged_ = float(alpha), bool(converged)
        self.alpha_rounds_ = numpy.array(rounds, dtype=numpy.float64)
        self.alpha_init_ = math.exp(ubar - vbar) * x
        pack_at(self.alpha_)
        lr = steps()
        eng.set_coords(self.alpha_init_)
        run(lr)
        return lr

    def score(self, X, structure=None):
        """How well a structure fits the map `X` (SPEC 2.8): a `FitScore`.  `X` takes every
        form `fit` takes and is packed the same way, under this solver's kind, alpha, dtype and
        devices; no iteration runs -- one pass over the packed map forms float64 sums per
        genomic separation and per bin, summed over the ranks of a torch.distributed job or
        the members of `devices=`.  structure: (n_bins, 3); None: `structure_` of the last fit.
        The score is against the pairs `X` holds: to score against a completed map, pass
        `ContactMap.shortest_paths(...)` to a kind='wish' solver.  Comparable across
        weight_power: `FitScore.stress` holds all three S_q."""
        source, n = self._map_source(X)
        xyz = _check_coords(self._fitted(structure, "score"), n)
        eng, world, _, pack = self._engine_for(source, n)
        with _teardown(eng):
            pack(self.kind, None, None)
            profile, bins = eng.score(xyz)
            profile = _sum_over_ranks(profile, eng, world)
            bins = _sum_over_ranks(bins, eng, world)
        return FitScore(profile, bins)

    def compare(self, B, A=None, **kw):
        """This fit against another structure `B` of the same bins (SPEC 2.10): a
        `StructureComparison`, `compare_structures(A, B, **kw)` with A = `structure_` of the last
        fit unless given -- B is laid onto A."""
        return compare_structures(self._fitted(A, "compare"), B, **kw)

    def _group_devices(self):
        """The devices of a devices= / n_gpus= fit (one entry included), checked against this
        process (device count, no torch.distributed job), or None without them."""
        if self._group is None:
            return None
        if running_job() is not None:                    # (torch is never imported here)
            raise ValueError("devices= drives several GPUs from one process; inside a "
                             "torch.distributed job every rank runs its own GPU (leave devices "
                             "unset)")
        count = _lib.c_int()
        _lib.check(_lib.load().bb_device_count(count), "bb_device_count")
        bad = [d for d in self._group if d >= count.value]
        if bad:
            raise ValueError("devices: index %d is out of range (%d HIP devices)"
                             % (bad[0], count.value))
        return list(self._group)

    def _balance_on(self, source, n_bins, args, want_expected):
        """fit_triples(balance=...): the bias (and the expected, or all ones) of `source`, a
        DeviceTriples or a ContactMap; the results kept on the solver."""
        if getattr(source, "is_triples", False):
            bias = source.balance(n_bins, **args)
            e = source.expected(n_bins, bias) if want_expected else None
        else:
            bias = source.balance(**args)
            e = source.expected() if want_expected else None
        self.bias_, self.balance_masked_ = bias, source.balance_masked_
        self.balance_iterations_ = source.balance_iterations_
        self.balance_converged_ = source.balance_converged_
        self.balance_variance_ = source.balance_variance_
        if want_expected:
            self.expected_ = e
        return bias, (numpy.ones(n_bins) if e is None else e)

    def fit_triples(self, triples, resolution, n_bins, KRnorm=None, KRexpected=None, init=None,
                    complete=None, balance=None):
        """Solve straight from a Rao-format sparse file's content, never building
        the dense matrix: `triples` is the (n, 3) array [pos_i, pos_j, count] that
        `ContactMap.__init__` reads (reference `blueberry/datatypes.pyx:100-102`),
        bins are `int(pos / resolution)` (pyx:111-112), the matrix has
        `n_bins + 1` bins (pyx:97), and with KRnorm / KRexpected each count is
        balanced and O/E-normalised on the device as `ContactMap.normalize`
        would (pyx:166-169).  A bin pair that occurs more than once keeps its last
        count, as in the reference's scatter (pyx:115-116).
        complete='shortest_path' (see `fit`): the triples are scattered into a dense resident
        matrix (`ContactMap.from_triples`), normalised there if KR vectors are given, and that
        map is completed and fitted.
        balance: None, True or a dict of `balance_triples`' arguments (ignore_diags, min_nnz,
        tol, max_iter, row_sum, expected=False): the raw map is balanced first, on the device
        and from the very triples the fit reads (docs/SPEC.md 2.5.3), and the fit is that of
        `fit_triples(KRnorm=bias, KRexpected=ones)` -- with expected=True `KRexpected=e` -- bit
        for bit.  Leaves `bias_`, `balance_masked_`, `balance_iterations_`,
        `balance_converged_` and (expected=True) `expected_`.  It takes the place of KRnorm /
        KRexpected; with several devices the first one balances, in a distributed job every
        rank its own copy (the same bits); with complete='shortest_path' the dense map is
        balanced (`ContactMap.balance`).  `triples` may be a `DeviceTriples` on this solver's
        device (one-device fits without `complete`), which stays open."""
        _check_complete(complete)
        self._check_auto_route(complete)
        n = int(n_bins) + 1
        landmark = self._landmark_wanted(init)
        if landmark:
            self._check_landmark_route(complete)
        if balance is not None:
            if KRnorm is not None or KRexpected is not None:
                raise ValueError("balance= computes the bias itself: it takes no KRnorm / KRexpected")
            bal_args, bal_expected = _balance_options(balance)
            if not isinstance(triples, DeviceTriples):
                _check_triples(triples)
            if complete is None and not hasattr(self._engine_factory, "set_wish_triples"):
                raise ValueError("balance= runs on the device: this solver's engine has none")
        if KRnorm is not None and (numpy.any(numpy.asarray(KRnorm) == 0.0)
                                   or numpy.any(numpy.asarray(KRexpected)[:n_bins] == 0.0)):
            raise ZeroDivisionError("float division")      # as ContactMap.normalize
        if complete is not None:
            cm = ContactMap.from_triples(triples, resolution, n_bins, KRnorm=KRnorm,
                                         KRexpected=KRexpected, device=self._completion_device())
            if balance is not None:
                cm._KRnorm, cm._KRexpected = self._balance_on(cm, int(n_bins), bal_args, bal_expected)
            if KRnorm is not None or KRexpected is not None or balance is not None:
                cm.normalize()
            return self.fit(cm, init=init, complete=complete)
        if hasattr(self._engine_factory, "set_wish_triples"):
            # nan_to_num (pyx:102), the binning and the tile occupancy on the device: the host
            # never makes a pass over the triples (round 3: two isfinite passes, two divide +
            # astype passes and a scipy COO over 240 MB at chr1@10kb)
            devices = self._group_devices()
            if not (devices and len(devices) > 1):
                devices = [self._pick_device(_dist_state(self.distributed)[1])]
            # (several devices: every member packs from its own device's copy)
            with _resident_triples(triples, resolution, devices) as dev:
                try:
                    if balance is not None:
                        KRnorm, KRexpected = self._balance_on(dev, int(n_bins), bal_args, bal_expected)
                    if landmark:
                        start = self._landmark_init(dev, int(n_bins), KRnorm, KRexpected)
                        init = start if init is None else init
                    return self._fit_impl(dev, n, init, KRnorm, KRexpected)
                finally:
                    self._drop_anchor()
        # engines without a device (tests): bin on the host, as round 3 did
        t = _nan_to_num(_check_triples(triples))     # pyx:102 (no copy when every value is finite)
        rows = (t[:, 0] / resolution).astype(numpy.int64)
        cols = (t[:, 1] / resolution).astype(numpy.int64)
        import scipy.sparse
        keep = rows != cols
        sp = scipy.sparse.coo_matrix((t[keep, 2], (rows[keep], cols[keep])), shape=(n, n))
        return self._fit_impl(sp, n, init, KRnorm, KRexpected)

    def fit_many(self, maps, inits=None, complete=None):
        """Solve SEVERAL maps at once on one GPU -- e.g. the 23 per-chromosome ContactMaps
        of a genome (the reference's ContactMap is per chromosome, `blueberry/
        datatypes.pyx:88`), each of which alone is launch-bound (5-20 us per iteration
        whatever its size).  The maps are laid end to end in one blocked-sparse solver
        (`bb_solver_set_maps`): one sweep and one reduce launch per iteration serve all of
        them, every map with its own step (`lr='auto'`: 1 / (2 n_m)) and its own stress
        history.  Same iteration as `fit()` map by map; results agree with the single fits
        to rounding (1e-5 fp32 / 1e-12 fp64: the partial sums are cut differently), not bit
        for bit.  Inside a torch.distributed job the maps are dealt to the ranks by size,
        every rank solves its own in one solver on its GPU, and every rank gets all results
        (`ranks_of_maps_` tells who solved what): no exchange during the iterations.

        maps: sequence of ContactMaps (resident ones are packed device to device), square
        ndarrays or anything `numpy.asarray` takes.  inits: None, or one (n_m, 3) start per
        map (None entries: the seeded default of `fit()`).  complete='shortest_path' (see
        `fit`): every map is completed on the device that solves it and the fit is that of the
        completed maps under kind='wish'; `completed_unreachable_pairs_` is then a list.
        Sets `structures_` (list of (n_m, 3) float64), `stresses_` (list of per-iteration
        arrays), `n_bins_many_`, `lrs_`, `n_iter_`; returns self."""
        if self._group is not None and len(self._group) > 1:
            raise ValueError("fit_many with devices= / n_gpus= is not supported: fit_many runs "
                             "on one device, or one per rank of a torch.distributed job")
        _check_complete(complete)
        if self.alpha_auto:
            raise self._auto_refusal("is not for fit_many: its maps share one solver and one "
                                     "exponent, and a per-map alpha is not covered")
        if self.n_landmarks is not None:
            raise self._landmark_refusal("is not for fit_many, which packs dense blocks",
                                         "complete='shortest_path' or init='spectral'")
        if not hasattr(self._engine_factory, "set_maps"):
            raise TypeError("fit_many needs an engine that holds several maps (HipEngine)")
        maps = list(maps)
        if not maps:
            raise ValueError("fit_many needs at least one map")
        if inits is None:
            inits = [None] * len(maps)
        if len(inits) != len(maps):
            raise ValueError("inits needs one entry per map")
        rank, world = _dist_state(self.distributed)
        if world > 1:
            # Several GPUs: the maps are independent problems, so every rank solves maps of its
            # own (dealt by size, largest first, to the rank with the least pairs so far) and
            # the results are gathered -- no exchange during the iterations at all.
            sizes = [self._map_source(X, sparse=False)[1] for X in maps]
            load, mine = [0] * world, [[] for _ in range(world)]
            for m in sorted(range(len(maps)), key=lambda q: (-sizes[q], q)):
                r = min(range(world), key=lambda q: (load[q], q))
                load[r] += sizes[m] * sizes[m]
                mine[r].append(m)
            part = None
            if mine[rank]:
                local = self._clone(device=self._pick_device(world), distributed=False,
                                    devices=None, n_gpus=None)
                local._fit_many_local([maps[m] for m in mine[rank]], [inits[m] for m in mine[rank]],
                                      complete)
                part = (mine[rank], local.structures_, local.stresses_, local.lrs_,
                        getattr(local, "completed_unreachable_pairs_", None))
            parts = gather_objects(part, world)
            n = len(maps)
            self.structures_, self.stresses_, self.lrs_ = [None] * n, [None] * n, [None] * n
            unreachable = [None] * n
            for p in parts:
                if p is not None:
                    for k, m in enumerate(p[0]):
                        self.structures_[m], self.stresses_[m], self.lrs_[m] = p[1][k], p[2][k], p[3][k]
                        if p[4] is not None:
                            unreachable[m] = p[4][k]
            if complete is not None:
                self.completed_unreachable_pairs_ = unreachable
            self.n_bins_many_ = sizes
            self.n_iter_ = max(int(h.shape[0]) for h in self.stresses_)
            self.ranks_of_maps_ = [next(r for r in range(world) if m in mine[r]) for m in range(n)]
            return self
        return self._fit_many_local(maps, inits, complete)

    def _fit_many_local(self, maps, inits, complete=None):
        """fit_many on this rank's GPU (see fit_many)."""
        kind = self.kind
        if complete is not None:
            maps = [self._completed(X, device=self._pick_device(1)) for X in maps]
            self.completed_unreachable_pairs_ = [cm.unreachable_pairs_ for cm in maps]
            kind = "wish"
        pairs = [self._map_source(X, sparse=False) for X in maps]
        srcs, sizes = [src for src, _ in pairs], [n for _, n in pairs]
        if min(sizes) < 2:
            raise ValueError("every map needs at least 2 bins")
        # the tile edge of the joint layout: 128 only for a small fp64 problem
        def layout(vw):
            off = [0]
            for n in sizes[:-1]:
                off.append(off[-1] + -(-n // vw) * vw)
            return off, off[-1] + sizes[-1]
        off, total = layout(128)
        if layout_info(total, self.dtype)["vw"] != 128:
            off, total = layout(512)
        vw = layout_info(total, self.dtype)["vw"]
        ti, tj = [], []
        for o, n in zip(off, sizes):
            b0, b1 = o // vw, (o + n + vw - 1) // vw
            jj, ii = numpy.meshgrid(numpy.arange(b0, b1), numpy.arange(b0, b1))
            sel = ii <= jj
            ti.append(ii[sel])
            tj.append(jj[sel])
        ti, tj = numpy.concatenate(ti), numpy.concatenate(tj)
        order = numpy.lexsort((ti, tj))
        tiles = (ti[order].astype(numpy.int32), tj[order].astype(numpy.int32))
        lrs = [self._one_step(n) for n in sizes]
        device = self._pick_device(1)
        x0 = numpy.zeros((total, 3))
        for m, (o, n) in enumerate(zip(off, sizes)):
            init = inits[m]
            if init is None and self.init == "spectral":
                # each map's classical-MDS start from a solver of its own (device form), which
                # only makes the start: unweighted, one step for all, no iterations
                init = self._clone(n_iter=0, init="spectral", device=device, distributed=False,
                                   devices=None, n_gpus=None, degree_steps=False, weight_power=0,
                                   momentum=0.0, tol=None, kind=kind).fit(maps[m]).structure_
            elif init is None:
                init = self._default_start(n)
            x0[o:o + n] = _check_coords(init, n)
        eng = self._engine_factory(total, self.dtype, rank=0, world=1, device=device, tiles=tiles)
        with _teardown(eng):
            eng.set_maps(off + [total], lrs)
            for o, n, src in zip(off, sizes, srcs):
                if getattr(src, "is_resident", False) and src._resident().device == eng.device:
                    eng.set_wish_from_cm_block(src._resident(), o, kind, self.alpha)
                else:
                    m = src.to_host() if getattr(src, "is_resident", False) else src
                    eng.set_wish_dense_block(m, o, kind, self.alpha)
            sums = self._bin_sums(eng, 1)
            if sums is not None:
                # SPEC 2.3.1 / 2.4.1 per map: every bin's whole step goes into `steps`
                # (lr = 1 below), each map's `lr` -- 'auto' or a float -- being the step of its
                # best-connected bin
                steps = numpy.ones(total)
                for q, (o, n) in enumerate(zip(off, sizes)):
                    part = sums[o:o + n]
                    lrs[q], scale = self._steps(part, n)
                    if self.weight_power:
                        steps[o:o + n] = lrs[q] if scale is None else lrs[q] * scale
                    else:
                        # multiplied before it is divided: not the bits of lr * scale, the
                        # factors fit() hands to set_bin_steps (`degree_step_factors`)
                        steps[o:o + n] = lrs[q] * (part.max() + 1.0) / (part + 1.0)
                eng.set_bin_steps(steps)
            eng.set_coords(x0)
            if self.momentum:
                eng.set_momentum(self.momentum)
            nm = len(sizes)
            # converged: every map's last step decreased its stress by <= tol, relatively (a
            # map at stress 0 counts as converged, which the single fit() never stops on)
            self._iterate(lambda k: eng.iterate(k, 1.0),
                          lambda: eng.stress_history().reshape(-1, nm),
                          lambda h: h.shape[0] >= 2 and numpy.all(
                              numpy.abs(h[-2] - h[-1]) <= self.tol * numpy.maximum(h[-2], 1e-300)))
            X = eng.get_coords()
            hist = eng.stress_history().reshape(-1, nm)
        self.structures_ = [X[o:o + n].copy() for o, n in zip(off, sizes)]
        self.stresses_ = [hist[:, m].copy() for m in range(nm)]
        self.n_bins_many_, self.lrs_, self.n_iter_ = sizes, lrs, int(hist.shape[0])
        return self

    def fit_transform(self, X, init=None):
        """`fit(X)` and return the (n_bins, 3) coordinates."""
        return self.fit(X, init=init).structure_


def spectral_init(eng, n, world, n_iter=40, seed=0, tol=0.0, return_iterations=False):
    """Classical-MDS start: the top three eigenpairs of B = -1/2 J (D o D) J,
    J = I - 11'/n, by block power iteration with a Rayleigh-Ritz step, using the
    device matvec over the resident units (`bb_solver_matvec_sq`); X0 = V sqrt(L).
    This is the host-driven form (several ranks: the per-rank products are summed over
    the ranks between steps; and engines without a device); on one rank
    `HipEngine.spectral_init_device` runs the same iteration without leaving the device.
    Exact (up to a rigid motion) for a complete, noise-free distance matrix; for
    incomplete maps the missing pairs count as zero distance, so it is a start,
    not a solution.  tol > 0: the stopping rule of `bb_solver_spectral_init_tol` (after every
    product but the first, ||Z - V V'Z||_F / ||Z||_F < tol ends the loop).  Plays the part
    SURVEY.md 8(f)-2 assigns to the reference's `ContactMap.eigenvector`
    (`blueberry/datatypes.pyx:216-235`)."""
    def apply_B(V):
        U = V - V.mean(axis=0)
        W = _sum_over_ranks(eng.matvec_sq(U), eng, world)
        return -0.5 * (W - W.mean(axis=0))

    def orth(A):
        # fewer than 3 bins: QR gives fewer than 3 columns; the missing ones are zero directions
        Q = numpy.linalg.qr(A)[0]
        if Q.shape[1] < 3:
            Q = numpy.hstack([Q, numpy.zeros((n, 3 - Q.shape[1]))])
        return Q

    G0 = numpy.random.default_rng(seed).standard_normal((n, 3))
    V = orth(G0)
    done, Z = 0, None
    for it in range(int(n_iter)):
        Z = apply_B(V)
        if tol > 0.0 and it > 0:
            zz, G = float((Z * Z).sum()), V.T @ Z
            if (numpy.sqrt(max(0.0, zz - float((G * G).sum())) / zz) if zz > 0.0 else 0.0) < tol:
                break
        V, Z = orth(Z), None
        done = it + 1
    if Z is None:
        Z = apply_B(V)
    evals, evecs = numpy.linalg.eigh(0.5 * (V.T @ Z + Z.T @ V))       # Rayleigh-Ritz, 3x3
    order = numpy.argsort(evals)[::-1]
    U = V @ evecs[:, order]
    # an eigenvector's sign is arbitrary (numpy's eigh and the device path's Jacobi sweeps
    # need not agree): every Ritz vector is turned to the side of the start's first column,
    # here and in bb_solver_spectral_init, so one seed gives one start on every world size
    U = U * numpy.where(U.T @ G0[:, 0] < 0.0, -1.0, 1.0)
    x0 = U * numpy.sqrt(numpy.maximum(evals[order], 0.0))
    return (x0, done) if return_iterations else x0
