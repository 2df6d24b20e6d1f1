"""The engines a fit runs on -- `HipEngine`, one rank's device state, 1:1 over the bb_solver_*
C-ABI, and `GroupEngine`, several of them driven from one process (`bb_group_*`) -- and the checks
of what goes into them."""
import numpy

from . import _lib
from .plan import _DTYPES, _KINDS


class RankDeficient(RuntimeError):
    """The block power iteration of the device-resident spectral start lost rank: the map has
    fewer than three independent directions (an empty or unconstrained map, fewer than 4 bins).
    `fit()` then takes the host-driven start; every other library error propagates."""


class HipEngine(_lib.Handle):
    """One rank's device state: thin, 1:1 over the bb_solver_* C-ABI."""

    prefix = "bb_solver_"
    n_maps = 1                      # several once set_maps() has laid them end to end

    def __init__(self, n_bins, dtype, rank=0, world=1, device=0, tiles=None):
        _lib.Handle.__init__(self)
        self.n_bins, self.dtype, self.rank, self.world, self.device = (
            int(n_bins), dtype, int(rank), int(world), int(device))
        if tiles is None:
            ti = tj = None
            nt = 0
        else:
            ti = numpy.ascontiguousarray(tiles[0], dtype=numpy.int32)
            tj = numpy.ascontiguousarray(tiles[1], dtype=numpy.int32)
            if ti.shape != tj.shape or ti.ndim != 1:
                raise ValueError("tiles must be a pair of equal-length 1-D index arrays")
            nt = ti.shape[0]
        self._create(self.n_bins, _DTYPES[dtype], self.device, self.rank, self.world,
                     None if ti is None else ti.ctypes.data_as(_lib.p_i32),
                     None if tj is None else tj.ctypes.data_as(_lib.p_i32), nt)
        self._exch = None
        self._comm_state = None     # "peer" | "rccl" | "torch" | "host" once chosen
        self._peer = None           # outcome of peer_setup()
        self._peer_error = ""
        self._comm_trial = None     # timings of select_exchange's trial, if one ran
        self._comm_trial_error = None   # what made a leg of that trial fail on this rank

    # -- lifetime ---------------------------------------------------------
    def close(self):
        _lib.Handle.close(self)
        self._exch = None

    # -- layout -----------------------------------------------------------
    def layout(self):
        info = _lib.LayoutInfo()
        ub, ue = _lib.c_i64(), _lib.c_i64()
        self._call("layout", info, ub, ue)
        d = info.as_dict()
        d["u_begin"], d["u_end"] = int(ub.value), int(ue.value)
        return d

    # -- inputs -----------------------------------------------------------
    def set_wish_dense(self, matrix, kind, alpha):
        m = _check_square(matrix, self.n_bins)
        self._call("set_wish_dense", _lib.as_f64_ptr(m), m.strides[0] // 8, _KINDS[kind],
                   float(alpha))

    def set_wish_from_cm(self, dev_matrix, kind, alpha):
        """Device to device from a resident ContactMap matrix (datatypes._DeviceMatrix)."""
        self._call("set_wish_from_cm", dev_matrix._open(), _KINDS[kind], float(alpha))

    def set_wish_resident(self, cm, kind, alpha):
        """A resident ContactMap: device to device when it lives on this engine's GPU."""
        dev = cm._resident()
        if dev.device == self.device:
            self.set_wish_from_cm(dev, kind, alpha)
        else:
            # the map lives on another GPU than this rank's solver (a ContactMap made with
            # an explicit device): through the host once, like a plain matrix
            self.set_wish_dense(cm.to_host(), kind, alpha)

    def set_wish_sparse(self, rows, cols, vals, kind, alpha, KRnorm=None, KRexpected=None):
        r = numpy.ascontiguousarray(rows, dtype=numpy.int64)
        c = numpy.ascontiguousarray(cols, dtype=numpy.int64)
        v = numpy.ascontiguousarray(vals, dtype=numpy.float64)
        if not (r.ndim == c.ndim == v.ndim == 1 and r.shape == c.shape == v.shape):
            raise ValueError("rows, cols, vals must be 1-D arrays of equal length")
        kr, ke = _kr_pair(KRnorm, KRexpected, self.n_bins)
        self._call("set_wish_sparse", r.ctypes.data_as(_lib.p_i64), c.ctypes.data_as(_lib.p_i64),
                   _lib.as_f64_ptr(v), r.shape[0], _KINDS[kind], float(alpha), kr, ke)

    def set_wish_triples(self, dev_triples, kind, alpha, KRnorm=None, KRexpected=None):
        """From triples resident on the device (`DeviceTriples`): binned, KR / O-E
        normalised and converted there."""
        kr, ke = _kr_pair(KRnorm, KRexpected, self.n_bins)
        self._call("set_wish_triples", dev_triples._open(), _KINDS[kind], float(alpha), kr, ke)

    # -- several maps in one solver (bb_solver_set_maps) -----------------------
    def set_maps(self, bin_begin, lr_scale):
        """Declare the maps laid end to end in this solver: map m owns the bins
        [bin_begin[m], bin_begin[m + 1]) and steps with lr * lr_scale[m]."""
        b = numpy.ascontiguousarray(bin_begin, dtype=numpy.int64)
        sc = numpy.ascontiguousarray(lr_scale, dtype=numpy.float64)
        if b.ndim != 1 or sc.ndim != 1 or b.shape[0] != sc.shape[0] + 1:
            raise ValueError("bin_begin needs one entry more than lr_scale")
        self._call("set_maps", sc.shape[0], b.ctypes.data_as(_lib.p_i64), _lib.as_f64_ptr(sc))
        self.n_maps = int(sc.shape[0])

    def set_wish_dense_block(self, matrix, bin_offset, kind, alpha):
        m = _check_square(matrix, numpy.asarray(matrix).shape[0])
        self._call("set_wish_dense_block", _lib.as_f64_ptr(m), m.strides[0] // 8, m.shape[0],
                   int(bin_offset), _KINDS[kind], float(alpha))

    def set_wish_from_cm_block(self, dev_matrix, bin_offset, kind, alpha):
        self._call("set_wish_from_cm_block", dev_matrix._open(), int(bin_offset), _KINDS[kind],
                   float(alpha))

    def _set_steps(self, name, scale, per):
        if scale is None:
            self._call(name, None, 0)
            return
        sc = numpy.ascontiguousarray(scale, dtype=numpy.float64)
        if sc.ndim != 1:
            raise ValueError("scale must be one factor per " + per)
        self._call(name, _lib.as_f64_ptr(sc), sc.shape[0])

    def set_block_steps(self, scale):
        """A step per block of the layout (`bb_solver_set_block_steps`): bin i moves by
        lr * scale[i // vw] * g_i; None = one step for all again."""
        self._set_steps("set_block_steps", scale, "block")

    def set_bin_steps(self, scale):
        """A step per bin (`bb_solver_set_bin_steps`): bin i moves by lr * scale[i] * g_i;
        None = one step for all again."""
        self._set_steps("set_bin_steps", scale, "bin")

    def degrees(self):
        """Per bin, the number of this rank's stored pairs that constrain it (delta > 0):
        `bb_solver_degrees`, one pass over the resident units."""
        out = numpy.zeros(self.n_bins, dtype=numpy.int64)
        self._call("degrees", out.ctypes.data_as(_lib.p_i64), out.shape[0])
        return out

    def set_weight_power(self, q):
        """Weighted stress (SPEC 2.3.1): w = delta^-q, q in {0, 1, 2}
        (`bb_solver_set_weight_power`)."""
        self._call("set_weight_power", int(q))

    def weight_sums(self):
        """Per bin, s_i = sum_j delta_ij^-q over this rank's stored pairs, float64
        (`bb_solver_weight_sums`; q = 0: the degrees)."""
        out = numpy.zeros(self.n_bins, dtype=numpy.float64)
        self._call("weight_sums", _lib.as_f64_ptr(out), out.shape[0])
        return out

    anchored = False                # landmark constraints resident (set_anchors)

    def set_anchors(self, rows, kept=None, weight=0.0):
        """Landmark constraints inside the fit (SPEC 2.5.5, `bb_solver_set_anchors`): the engine
        makes its own copy of the rows of `rows` (a `GeodesicRows`) with kept[a] true (None:
        all), which may be closed afterwards.  rows None or weight 0 clears them."""
        k = None
        if rows is not None and kept is not None:
            k = numpy.ascontiguousarray(kept, dtype=numpy.uint8)
            if k.shape != (rows.n_sources,):
                raise ValueError("kept must have one entry per source")
        self._call("set_anchors", None if rows is None else rows._open(),
                   None if k is None else k.ctypes.data_as(_lib.p_u8), float(weight))
        self.anchored = self.anchor_info()[0] > 0

    def anchor_sums(self):
        """Per bin, weight * sum of D^-q over the landmark terms that touch it, float64
        (`bb_solver_anchor_sums`): what joins `weight_sums` in the steps of SPEC 2.4.1."""
        out = numpy.zeros(self.n_bins, dtype=numpy.float64)
        self._call("anchor_sums", _lib.as_f64_ptr(out), out.shape[0])
        return out

    def anchor_stress(self):
        """The landmark terms' share of the stress at the current coordinates."""
        return float(self._get(_lib.c_dbl, "anchor_stress"))

    def anchor_info(self):
        """(kept rows, terms, bytes resident) of the anchors; zeros without."""
        rows, terms, nbytes = _lib.c_i64(), _lib.c_i64(), _lib.c_i64()
        self._call("anchor_info", rows, terms, nbytes)
        return int(rows.value), int(terms.value), int(nbytes.value)

    def score(self, xyz=None):
        """The sums of SPEC 2.8 over this rank's units (`bb_solver_score`): (profile, bins),
        float64 of shape (n_bins, 9) and (n_bins, 3).  xyz: the structure to score; None: the
        engine's own coordinates."""
        profile = numpy.zeros((self.n_bins, 9), dtype=numpy.float64)
        bins = numpy.zeros((self.n_bins, 3), dtype=numpy.float64)
        self._call("score", None if xyz is None else _lib.as_f64_ptr(_check_coords(xyz, self.n_bins)),
                   _lib.as_f64_ptr(profile), _lib.as_f64_ptr(bins))
        return profile, bins

    def loglog(self, xyz=None):
        """The log-log sums of SPEC 2.11 over this rank's units (`bb_solver_loglog`): float64 of
        shape (n_bins, 7), row k = the pairs of separation k: pairs with d > 0, sum u, sum v,
        sum u^2, sum v^2, sum u v (u = log delta, v = log d), pairs with d = 0.  xyz as `score`."""
        profile = numpy.zeros((self.n_bins, 7), dtype=numpy.float64)
        self._call("loglog", None if xyz is None else _lib.as_f64_ptr(_check_coords(xyz, self.n_bins)),
                   _lib.as_f64_ptr(profile))
        return profile

    def repower(self, p):
        """Every stored wish distance w > 0 becomes w^p under the wish rule of SPEC 2.1, in place
        (`bb_solver_repower`); degrees and weight sums are the caller's to recompute."""
        self._call("repower", float(p))

    def stress_maps(self):
        out = numpy.empty(self.n_maps, dtype=numpy.float64)
        self._call("stress_maps", _lib.as_f64_ptr(out), out.shape[0])
        return out

    def set_wish_from_coords(self, xstar):
        self._call("set_wish_from_coords", _lib.as_f64_ptr(_check_coords(xstar, self.n_bins)))

    def set_coords(self, x0):
        self._call("set_coords", _lib.as_f64_ptr(_check_coords(x0, self.n_bins)))

    def get_coords(self):
        out = numpy.empty((self.n_bins, 3), dtype=numpy.float64)
        self._call("get_coords", _lib.as_f64_ptr(out))
        return out

    # -- iterations -------------------------------------------------------
    def set_momentum(self, mu):
        self._call("set_momentum", float(mu))

    def iterate(self, iters, lr):
        self._call("iterate", int(iters), float(lr))

    def grad(self):
        self._call("grad")

    def apply(self, lr):
        self._call("apply", float(lr))

    def matvec_sq(self, x):
        """(D o D) @ x for this rank's units; x is (n_bins, 3)."""
        x = _check_coords(x, self.n_bins)
        y = numpy.empty_like(x)
        self._call("matvec_sq", _lib.as_f64_ptr(x), _lib.as_f64_ptr(y))
        return y

    def spectral_init_device(self, n_iter, v0, tol=0.0):
        """Classical-MDS start computed and left on the device: `bb_solver_spectral_init_tol`.
        v0: (n_bins, 3) start of the block power iteration (the same on every rank).  With
        several ranks it is collective and needs their exchange set up first (peer arenas or
        the library's communicator): the per-rank products are summed on the device, nothing
        of size N crosses PCIe.  tol > 0: n_iter is the most products made; the loop ends once
        B V lies within tol (relative) of span(V).  Returns (products orthonormalised, last
        distance read or -1).  Raises RankDeficient when the iterate lost rank."""
        v0 = _check_coords(v0, self.n_bins)
        done, res = _lib.c_int(), _lib.c_dbl()
        # explicit: a lost rank is an outcome of its own (the caller takes the host-driven start)
        rc = self._status("spectral_init_tol", int(n_iter), float(tol), _lib.as_f64_ptr(v0), done, res)
        if rc == _lib.BB_ERR_STATE and "lost rank" in _lib.last_error():
            raise RankDeficient(_lib.last_error())
        _lib.check(rc, "bb_solver_spectral_init_tol")
        return int(done.value), float(res.value)

    def stress(self):
        return float(self._get(_lib.c_dbl, "stress"))

    def stress_history(self):
        out = numpy.empty(int(self._get(_lib.c_i64, "get_stress_history", None, 0)),
                          dtype=numpy.float64)
        if out.size:
            self._get(_lib.c_i64, "get_stress_history", _lib.as_f64_ptr(out), out.size)
        return out

    def sync(self):
        self._call("sync")

    def exchange_size(self):
        return int(self._get(_lib.c_i64, "exchange_size"))

    def read_exchange(self):
        """Exchange buffer [g (n_pad,3) | stress hi | lo] as float64 on the host."""
        out = numpy.empty(self.exchange_size(), dtype=numpy.float64)
        self._call("read_exchange", _lib.as_f64_ptr(out), out.size)
        return out

    def write_exchange(self, host):
        host = numpy.ascontiguousarray(host, dtype=numpy.float64)
        self._call("write_exchange", _lib.as_f64_ptr(host), host.size)

    # -- the all-reduce boundary (world > 1) --------------------------------
    def comm_setup(self):
        """Make the library's own RCCL communicator for this job: rank 0 draws the
        128-byte id, torch.distributed only carries it to the other ranks, every
        rank joins (`ncclCommInitRank`).  Collective.  Returns False -- on every
        rank alike -- when RCCL cannot be used, so that the caller can fall back
        to the torch.distributed all-reduce."""
        import ctypes
        import torch.distributed as dist
        box = [None]
        if self.rank == 0:
            buf = ctypes.create_string_buffer(128)
            if self._lib.bb_comm_unique_id(buf) == _lib.BB_OK:
                box[0] = buf.raw
        dist.broadcast_object_list(box, src=0)
        if box[0] is None:
            return False
        # explicit: a failure here is this rank's vote, not an error
        ok = self._status("comm_init", box[0]) == _lib.BB_OK
        # all ranks must take the same path: agree on the outcome
        import torch
        flag = torch.tensor([1 if ok else 0], dtype=torch.int32,
                            device=torch.device("cuda", self.device))
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        return bool(flag.item())

    # the library's communicator cache (bb_comm_cached / bb_solver_comm_attach / _detach):
    # `exchange.comm_reuse` drives these three
    def _comm_cached(self):
        import ctypes
        have = ctypes.c_int(0)
        self._lib.bb_comm_cached(self.device, self.rank, self.world, ctypes.byref(have))
        return bool(have.value)

    def _comm_generation(self):
        """Generation of the free cached communicator for this engine's key -- a hash of the
        unique id it was made with, equal on the ranks that made it together -- or 0."""
        import ctypes
        have, gen = ctypes.c_int(0), ctypes.c_uint64(0)
        self._lib.bb_comm_cached_generation(self.device, self.rank, self.world,
                                            ctypes.byref(have), ctypes.byref(gen))
        return int(gen.value) if have.value else 0

    def _comm_attach(self):
        # explicit: the outcome is agreed between the ranks (`comm_reuse`), not raised
        return self._status("comm_attach") == _lib.BB_OK

    def _comm_detach(self):
        self._status("comm_detach")

    def iterate_dist(self, iters, lr):
        """`iters` x { grad, RCCL all-reduce, apply }, all enqueued by one C call."""
        self._call("iterate_dist", int(iters), float(lr))

    def peer_setup(self):
        """Connect the peer exchange (one-shot all-reduce inside the solver's own
        kernels, include/blueberry_hip.h): every rank exports its receive arena,
        torch.distributed only carries the 128-byte handles, every rank maps all
        arenas.  Collective.  Returns False -- on every rank alike -- when any
        rank could not export or map, so that the caller can fall back to RCCL."""
        import ctypes
        import torch.distributed as dist
        if self._peer is not None:
            return self._peer
        buf = ctypes.create_string_buffer(_lib.BB_PEER_HANDLE_BYTES)
        # explicit, here and at the connect: a failure is this rank's vote, not an error
        mine = buf.raw if self._status("peer_export", buf) == _lib.BB_OK else None
        handles = [None] * self.world
        dist.all_gather_object(handles, mine)
        ok = all(h is not None for h in handles)
        if ok:
            ok = self._status("peer_connect", b"".join(handles)) == _lib.BB_OK
        if not ok:
            self._peer_error = _lib.last_error()
        oks = [None] * self.world
        dist.all_gather_object(oks, bool(ok))
        self._peer = all(oks)
        return self._peer

    def iterate_peer(self, iters, lr):
        """`iters` x { grad, reduce + push to every peer, wait + rank-ordered sum +
        update }, all enqueued by one C call."""
        self._call("iterate_peer", int(iters), float(lr))

    def sync_timeout(self, milliseconds):
        """sync() that raises RuntimeError if the stream has not drained in time."""
        self._call("sync_timeout", int(milliseconds))

    def comm_abort(self):
        self._call("comm_abort")

    def peer_form(self):
        """'one launch' (reduce, push, wait, sum and update in one kernel) or 'two launches'
        (include/blueberry_hip.h, peer exchange)."""
        return "one launch" if self._get(_lib.c_int, "peer_form") else "two launches"

    def peer_set_form(self, one_launch):
        """Choose the exchange's form before its first use (the same on every rank)."""
        self._call("peer_set_form", 1 if one_launch else 0)

    def peer_set_timeout(self, milliseconds):
        self._call("peer_set_timeout", int(milliseconds))

    def comm_world(self):
        """Ranks RCCL reports for the library's communicator, or None without one."""
        n = _lib.c_int()
        # explicit: no communicator is an answer (None), not an error
        if self._status("comm_world", n) != _lib.BB_OK:
            return None
        return int(n.value)

    def peer_status(self):
        """Synchronise and raise if a peer wait ran into its time limit."""
        return int(self._get(_lib.c_int, "peer_status"))

    def exchange_tensor(self):
        """A torch tensor aliasing the exchange buffer [g (n_pad,3) | hi | lo].

        torch allocates it (plumbing: it is what torch.distributed can reduce)
        and the solver is told to write its partial gradient there; the solver
        is also moved onto torch's current stream so that the collective and
        the kernels are ordered without host synchronisation."""
        if self._exch is None:
            import torch
            rts = _lib.hip_runtimes_loaded()
            if len(rts) > 1:
                raise RuntimeError(
                    "two HIP runtimes are loaded (%s): import torch BEFORE the first "
                    "blueberry_amd compute call in a distributed job, so that "
                    "libblueberry_hip.so binds to the runtime torch uses" % ", ".join(rts))
            tdt = torch.float32 if self.dtype == "float32" else torch.float64
            dev = torch.device("cuda", self.device)
            self._exch = torch.zeros(self.exchange_size(), dtype=tdt, device=dev)
            stream = torch.cuda.current_stream(dev)
            self._call("set_stream", _lib.c_void_p(stream.cuda_stream))
            self._call("set_exchange_buffer", _lib.c_void_p(self._exch.data_ptr()))
        return self._exch

    # -- measurement ------------------------------------------------------
    def set_timing(self, enabled):
        """True / 1: HIP events around every iteration; k > 1: every k-th; False: off."""
        self._call("set_timing", int(enabled))

    def timing(self):
        g, r, n = _lib.c_dbl(), _lib.c_dbl(), _lib.c_i64()
        self._call("get_timing", g, r, n)
        return {"grad_ms": float(g.value), "reduce_ms": float(r.value), "launches": int(n.value),
                "step_ms": float(self._get(_lib.c_dbl, "get_step_timing"))}

    def score_timing(self):
        """(profile_ms, fold_ms, bins_ms) of the last `score` or `loglog` (bins_ms = 0) made with
        timing on."""
        t = [_lib.c_dbl() for _ in range(3)]
        self._call("get_score_timing", *t)
        return tuple(float(v.value) for v in t)

    def event_gap_ms(self, pairs=16):
        """Average ms between two HIP events recorded back to back behind a sweep launch:
        what an event-timed interval contains besides its kernel (measurement aid)."""
        return float(self._get(_lib.c_dbl, "measure_event_gap", int(pairs)))

    def anchor_ms(self, launches=10):
        """Average ms of one iteration's three anchor launches alone (`bb_solver_measure_anchors`;
        measurement aid)."""
        return float(self._get(_lib.c_dbl, "measure_anchors", int(launches)))

    def stream_read_ms(self, launches=10):
        """Average ms of a read-only sweep over the resident units (measurement aid)."""
        return float(self._get(_lib.c_dbl, "measure_stream_read", int(launches)))

    def iteration_path(self):
        """'row_owner' (small one-rank maps: one launch per iteration) or 'units'."""
        ro, wpr = _lib.c_int(), _lib.c_int()
        self._call("iteration_path", ro, wpr)
        return ("row_owner", int(wpr.value)) if ro.value else ("units", 0)

    def traffic(self):
        b, p = _lib.c_i64(), _lib.c_i64()
        self._call("traffic", b, p)
        return {"unit_bytes": int(b.value), "pairs_dense": int(p.value)}

    def stream_info(self):
        """The 24-bit stream the fp32 stress sweep reads instead of the units, where it is in
        use (`bb_solver_stream_info`): units held packed and raw, its bytes and the changes of
        format between consecutive units; packed_units 0 and stream_bytes 0 with no stream."""
        v = [_lib.c_i64() for _ in range(4)]
        self._call("stream_info", *v)
        return dict(zip(("packed_units", "raw_units", "stream_bytes", "format_switches"),
                        (int(x.value) for x in v)))


class GroupEngine(_lib.Handle):
    """Several GPUs from ONE process (`bb_group_*`): member r is a HipEngine playing rank r of
    world R on devices[r] (a device may repeat: members then share it), each holding only its
    own units; one host thread per member enqueues its iterations, and the partials are summed
    by group_apply_kernel in rank order, ordered by HIP events.  To `StructureSolver` it looks
    like one engine of world 1: every setter goes to all members, degrees, weight sums, matvecs
    and scores come back summed over the members in rank order (float64 / int64), coordinates and
    stress history are member 0's -- all members hold the same bits."""
    prefix = "bb_group_"

    def __init__(self, n_bins, dtype, devices, tiles=None):
        _lib.Handle.__init__(self)
        self.n_bins, self.dtype = int(n_bins), dtype
        self.devices = [int(d) for d in devices]
        self.device = self.devices[0]
        self.world = 1                     # what the caller sees: one engine, summed results
        self._comm_state = "group"
        self.members = []
        try:
            R = len(self.devices)
            for r, d in enumerate(self.devices):
                self.members.append(HipEngine(n_bins, dtype, rank=r, world=R, device=d, tiles=tiles))
            handles = (_lib.c_void_p * R)(*[m._h.value for m in self.members])
            self._create(handles, R)
        except BaseException:
            self.close()
            raise

    def close(self):
        _lib.Handle.close(self)                # the group before its members
        for m in getattr(self, "members", ()):
            m.close()
        self.members = []

    def _each(self, name, *args):
        """Every member's `name`(*args), in rank order."""
        for e in self.members:
            getattr(e, name)(*args)

    def _summed(self, name, *args):
        """The members' `name`(*args) added on the host in rank order: (m0 + m1) + m2 ..."""
        out = getattr(self.members[0], name)(*args)
        for e in self.members[1:]:
            out = out + getattr(e, name)(*args)
        return out

    def layout(self):
        return self.members[0].layout()

    # -- inputs: every member packs its own units from the one input --------------------
    def set_wish_dense(self, matrix, kind, alpha):
        self._each("set_wish_dense", _check_square(matrix, self.n_bins), kind, alpha)

    def set_wish_sparse(self, rows, cols, vals, kind, alpha, KRnorm=None, KRexpected=None):
        self._each("set_wish_sparse", rows, cols, vals, kind, alpha, KRnorm, KRexpected)

    def set_wish_triples(self, dev_triples, kind, alpha, KRnorm=None, KRexpected=None):
        """`dev_triples.per_device`: the triples uploaded once per distinct device."""
        per_device = getattr(dev_triples, "per_device", {dev_triples.device: dev_triples})
        for e in self.members:
            e.set_wish_triples(per_device[e.device], kind, alpha, KRnorm, KRexpected)

    def set_wish_from_coords(self, xstar):
        self._each("set_wish_from_coords", _check_coords(xstar, self.n_bins))

    def set_wish_resident(self, cm, kind, alpha):
        """A resident ContactMap: members on its device pack device to device, members on
        other devices over peer access where the devices allow it; the rest share ONE host
        download of it."""
        dev = cm._resident()
        host = None
        for e in self.members:
            if e.device == dev.device:
                e.set_wish_resident(cm, kind, alpha)
                continue
            # explicit: "without peer access" sends this member through the host, not an error
            rc = e._status("set_wish_from_cm", dev._open(), _KINDS[kind], float(alpha))
            if rc == _lib.BB_OK:
                continue
            if not (rc == _lib.BB_ERR_INVALID and "without peer access" in _lib.last_error()):
                _lib.check(rc, "bb_solver_set_wish_from_cm")
            if host is None:
                host = cm.to_host()
            e.set_wish_dense(host, kind, alpha)

    # -- per-bin steps, weighting: summed on the host in rank order ---------------------
    def degrees(self):
        return self._summed("degrees")

    def set_weight_power(self, q):
        self._each("set_weight_power", q)

    def weight_sums(self):
        return self._summed("weight_sums")

    def set_bin_steps(self, scale):
        self._each("set_bin_steps", scale)

    def score(self, xyz=None):
        """SPEC 2.8 over the whole map: each of the members' two arrays summed in rank order."""
        profile, bins = self.members[0].score(xyz)
        for e in self.members[1:]:
            p, b = e.score(xyz)
            profile, bins = profile + p, bins + b
        return profile, bins

    def loglog(self, xyz=None):
        """SPEC 2.11 over the whole map: the members' sums added in rank order."""
        return self._summed("loglog", xyz)

    def repower(self, p):
        self._each("repower", p)

    def matvec_sq(self, x):
        """(D o D) @ x over the whole map: the members' products summed in rank order (the
        host-driven spectral start)."""
        return self._summed("matvec_sq", x)

    # -- iterations -------------------------------------------------------
    def set_coords(self, x0):
        self._each("set_coords", _check_coords(x0, self.n_bins))

    def set_momentum(self, mu):
        self._each("set_momentum", mu)

    def iterate(self, iters, lr):
        self._call("iterate", int(iters), float(lr))

    def get_coords(self):
        return self.members[0].get_coords()

    def stress_history(self):
        return self.members[0].stress_history()

    def member_coords(self):
        """Every member's coordinates (identical bits: a check, not a result)."""
        return [e.get_coords() for e in self.members]

    def member_stress_histories(self):
        return [e.stress_history() for e in self.members]

    def sync(self):
        self._each("sync")


def _check_square(matrix, n_bins):
    m = numpy.asarray(matrix)
    _square_bins(m.shape)
    if m.shape[0] != n_bins:
        raise ValueError("contact matrix has %d bins, solver was created for %d"
                         % (m.shape[0], n_bins))
    if m.dtype != numpy.float64 or m.strides[1] != 8 or m.strides[0] % 8 or m.strides[0] < 8 * n_bins:
        m = numpy.ascontiguousarray(m, dtype=numpy.float64)
    return m


def _square_bins(shape):
    """The number of bins of a contact matrix of this shape, which has to be n x n."""
    if len(shape) != 2 or shape[0] != shape[1]:
        raise ValueError("contact matrix must be square, got shape %r" % (shape,))
    return int(shape[0])


def _kr_pair(KRnorm, KRexpected, n_bins):
    """The two KR vectors of an input, padded to n_bins and as the pointers the C-ABI takes
    (they keep their arrays alive), or (None, None) without them."""
    if KRnorm is None and KRexpected is None:
        return None, None
    if KRnorm is None or KRexpected is None:
        raise ValueError("KRnorm and KRexpected go together")
    return (_lib.as_f64_ptr(_pad_vector(KRnorm, n_bins)),
            _lib.as_f64_ptr(_pad_vector(KRexpected, n_bins)))


def _pad_vector(v, n):
    """KR vectors have n_bins entries, the matrix n_bins+1 bins: pad with NaN
    (a NaN divisor = no constraint, as for unmappable bins in Rao's files)."""
    v = numpy.asarray(v, dtype=numpy.float64).ravel()
    if v.shape[0] > n:
        raise ValueError("KR vector longer than the number of bins")
    out = numpy.full(n, numpy.nan)
    out[:v.shape[0]] = v
    return out


def _check_coords(x, n_bins):
    x = numpy.ascontiguousarray(x, dtype=numpy.float64)
    if x.shape != (n_bins, 3):
        raise ValueError("coordinates must have shape (%d, 3), got %r" % (n_bins, x.shape))
    if not numpy.all(numpy.isfinite(x)):
        raise ValueError("coordinates must be finite")
    return x
