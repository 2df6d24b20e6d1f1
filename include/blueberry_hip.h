/*
 * blueberry_hip.h -- C-ABI of libblueberry_hip.so (MI355X / gfx950).
 *
 * The drop-in boundary for the contact-matrix -> 3D-coordinates hot path of
 * jmschrei/blueberry.  Plain C: pointers, sizes, int status codes.  No torch,
 * numpy or C++ types cross this line.  The Python host (blueberry_amd/) binds
 * it with ctypes; INTEGRATION.md shows the binding a maintainer of the
 * reference would add.
 *
 * The reference has NO FFI / plugin interface: its "interface"
 * is Python names star-exported from blueberry/__init__.py:38-43 and Cython
 * `cpdef` functions taking numpy arrays.  Every entry point below therefore
 * cites the reference *function or loop* it replaces; entry points of the
 * 3D-structure solver cite docs/SPEC.md instead, because the reference
 * contains no solver.
 *
 * Conventions
 *   - every function returns BB_OK (0) or a BB_ERR_* code; bb_last_error()
 *     returns a thread-local message for the last failure on this thread;
 *   - host pointers are borrowed for the duration of the call only; device
 *     memory is owned by opaque handles with explicit create/destroy;
 *   - one handle = one device = one host thread at a time (a bb_group's member
 *     solvers belong to the group's own threads while bb_group_iterate runs); the library never
 *     calls the oracle or any CPU fallback: without a usable GPU every compute
 *     entry point fails with BB_ERR_HIP.
 */
#ifndef BLUEBERRY_HIP_H
#define BLUEBERRY_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BB_API __attribute__((visibility("default")))

#define BB_VERSION 100 /* 0.1.0 */

enum {
    BB_OK = 0,
    BB_ERR_INVALID = 1, /* bad argument (null pointer, negative size, ...)   */
    BB_ERR_HIP = 2,     /* a HIP runtime call failed / no usable device      */
    BB_ERR_STATE = 3,   /* call sequence error (e.g. iterate before set_wish) */
    BB_ERR_NOMEM = 4    /* host or device allocation failed                  */
};

enum { BB_F32 = 0, BB_F64 = 1 };              /* arithmetic type of the solver */
enum { BB_KIND_WISH = 0, BB_KIND_COUNTS = 1 }; /* meaning of a dense input      */

BB_API int bb_version(void);
BB_API const char *bb_last_error(void);
/* Number of visible HIP devices; BB_ERR_HIP (count = 0) when there is none. */
BB_API int bb_device_count(int *count);

/* ---------------------------------------------------------------------- */
/* K1  count_band_regions   (reference: blueberry/blueberry.pyx:77-91)      */
/* ---------------------------------------------------------------------- */

/* t = #{(i, j) : 0 <= j < i < n, low <= regions[i] - regions[j] <= high}.
 * `regions` is a host vector of n float64 (what the reference reads through
 * `<double*> regions_ndarray.data`, pyx:80); low/high are C ints as at pyx:82
 * (LOW_FITHIC_CUTOFF / HIGH_FITHIC_CUTOFF, blueberry/utils.py:25-26).  The
 * count is exact (fp64 subtract, integer sum). */
BB_API int bb_band_count(const double *regions, int64_t n, int32_t low, int32_t high,
                         int device, int64_t *count);

/* The same sum restricted to rows i in [i_begin, i_end): one rank's share of
 * a row-sharded count (the shares are summed with an integer all-reduce). */
BB_API int bb_band_count_rows(const double *regions, int64_t n, int32_t low, int32_t high,
                              int64_t i_begin, int64_t i_end, int device, int64_t *count);

/* ---------------------------------------------------------------------- */
/* Device layout of the wish-distance matrix (docs/SPEC.md 3).  Host-only   */
/* arithmetic: callable without a GPU.                                      */
/* ---------------------------------------------------------------------- */

typedef struct bb_layout_info {
    int64_t n_bins;         /* N                                              */
    int64_t n_pad;          /* N rounded up to a multiple of vw               */
    int64_t vw;             /* tile edge = strip width: 512; fp64 <= 4096 bins: 128 */
    int64_t rows_per_unit;  /* rows per 8-KiB unit: 4 (fp32); fp64: 2, or 8 when vw = 128 */
    int64_t units_per_tile; /* vw / rows_per_unit                             */
    int64_t n_blocks;       /* n_pad / vw                                     */
    int64_t n_tiles;        /* upper-triangular tiles incl. the diagonal      */
    int64_t n_units;        /* n_tiles * units_per_tile                       */
} bb_layout_info;

BB_API int bb_layout_dense_info(int64_t n_bins, int dtype, bb_layout_info *info);
/* Tile list of the dense upper triangle in device order (column-strip major:
 * J ascending, then I ascending, I <= J).  cap >= info.n_tiles. */
BB_API int bb_layout_dense_tiles(int64_t n_bins, int dtype, int32_t *tile_I, int32_t *tile_J,
                                 int64_t cap);
/* Contiguous share of n_units units owned by `rank` of `world`. */
BB_API int bb_layout_rank_units(int64_t n_units, int rank, int world, int64_t *u_begin,
                                int64_t *u_end);

/* The sweep plan of a rank (docs/SPEC.md 3.3-3.5): what bb_solver_create derives from the
 * tile list, the rank's units [u_begin, u_end) and the device's CU count before it allocates
 * anything.  Knobs: what the BB_* environment variables of the same names set in a solver. */
typedef struct bb_sweep_knobs {
    int32_t waves_per_cu;   /* 1..32; 0: 8 from 65,000 units per rank, else 4               */
    int32_t pair;           /* not 0: workgroups of 8 waves at 8 waves per CU (the default)  */
    int32_t reduce_slices;  /* 4 or 8; 0: 4 while no reduce list is longer than 64 entries   */
    int32_t row_owner;      /* not 0: also the sizes of the row-owner path                   */
} bb_sweep_knobs;
typedef struct bb_sweep_plan {
    int64_t n_local;          /* u_end - u_begin                                             */
    int64_t t_first;          /* first tile with a local unit                                */
    int64_t n_local_tiles;
    int64_t n_waves;          /* a multiple of wpb                                           */
    int64_t wpb;              /* waves per workgroup: 4 or 8                                 */
    int64_t chunk_q, chunk_r; /* wave w owns units [w q + min(w, r), + q (+ 1 if w < r))     */
    int64_t n_slots;          /* column-partial slots                                        */
    int64_t rowpart_elems;    /* n_local_tiles * 3 vw                                        */
    int64_t colpart_elems;    /* n_slots * 3 vw                                              */
    int64_t zero_off;         /* offset of the chunk of zeros the reduce lists are padded with */
    int64_t part_total;       /* elements of the partials, the zero chunk included           */
    int64_t red_slices;       /* 4 or 8                                                      */
    int64_t red_stride;       /* entries per block of red_lists                              */
    int64_t red_blocks;       /* blocks of red_lists (the layout's n_blocks)                 */
    int64_t defer_cap_units;  /* units of row sums a wave parks in LDS                       */
    int64_t lds_wave_floats;  /* 4-byte words of LDS per wave                                */
    int64_t defer_lds_bytes;  /* dynamic LDS per workgroup                                   */
    int64_t nontemporal;      /* 1: the sweep's matrix loads are non-temporal                */
    int64_t full_ld;          /* row-owner path: row stride of the full matrix, else 0       */
    int64_t ro_wpr, ro_blocks;/* row-owner path: waves per row, workgroups holding rows      */
} bb_sweep_plan;
/* tile_I / tile_J NULL (n_tiles 0): the dense list of (n_bins, dtype).  Every array may be NULL:
 * `plan` alone then gives the counts to size them with -- udesc 2 n_local (row, column of each
 * unit), wave_slots 2 n_waves (first private slot, shared slot or -1), slot_strip n_slots,
 * wave_last_strip n_waves (-1: a wave without units), red_lists red_blocks * red_stride
 * offsets into the partials.  Host-only. */
BB_API int bb_layout_sweep_plan(int64_t n_bins, int dtype, const int32_t *tile_I, const int32_t *tile_J,
                                int64_t n_tiles, int64_t u_begin, int64_t u_end, int cus,
                                const bb_sweep_knobs *knobs, bb_sweep_plan *plan, int32_t *udesc,
                                int32_t *wave_slots, int32_t *slot_strip, int32_t *wave_last_strip,
                                int64_t *red_lists);
/* The table of the 24-bit stream (SPEC 3.7) of n units from min_max, 2 n words (the smallest and
 * the largest stored word of each unit), and udesc as above.  A unit is packable when largest -
 * smallest < 2^24 and stored packed inside a run of at least min_run packable units.  table: NULL,
 * or 4 n words (row, column, offset in KiB | packed << 31, base).  pays: whether a solver builds
 * the stream -- mode 0 never, 1 when a unit is packed, else when it saves an eighth of the raw
 * bytes -- and never at 2^31 KiB or more.  Host-only. */
BB_API int bb_layout_pk24_table(const uint32_t *min_max, const int32_t *udesc, int64_t n, int64_t min_run,
                                int mode, int32_t *table, int64_t *stream_kib, int64_t *packed_units,
                                int64_t *format_switches, int *pays);

/* ---------------------------------------------------------------------- */
/* S0  3D-structure solver  (docs/SPEC.md; absent from the reference)       */
/* ---------------------------------------------------------------------- */

typedef struct bb_solver bb_solver;

/* Create a solver for n_bins bins on `device`, playing `rank` of `world`
 * ranks (world = 1: the whole matrix).  tile_I/tile_J (n_tiles entries, device
 * order, I <= J) select the tiles that exist -- pairs outside them carry no
 * constraint (blocked-sparse input); pass NULL / 0 for the dense upper
 * triangle.  The solver runs on its own HIP stream unless bb_solver_set_stream
 * replaces it. */
BB_API int bb_solver_create(bb_solver **out, int64_t n_bins, int dtype, int device, int rank,
                            int world, const int32_t *tile_I, const int32_t *tile_J,
                            int64_t n_tiles);
BB_API int bb_solver_destroy(bb_solver *s);

/* Run on the caller's stream (a hipStream_t; NULL = the device's null stream),
 * e.g. torch's current stream so that an external all-reduce is ordered with
 * the kernels. */
BB_API int bb_solver_set_stream(bb_solver *s, void *hip_stream);
BB_API int bb_solver_layout(const bb_solver *s, bb_layout_info *info, int64_t *u_begin,
                            int64_t *u_end);

/* Dense (n_bins, n_bins) float64 host matrix, leading dimension ld elements;
 * only elements [i][j] with i < j are read.  kind = BB_KIND_WISH: entries are
 * wish distances (<= 0 / non-finite = no constraint).  kind = BB_KIND_COUNTS:
 * entries are contact counts, converted on the device with
 * delta = c^(-1/alpha) (SPEC 2.1).  On every input route a distance below the wish
 * floor or above the largest finite value of the solver's dtype (SPEC 2.1: 1e-30 and
 * 3.4e38 in fp32) is no constraint.  This is the matrix a ContactMap holds
 * (reference: blueberry/datatypes.pyx:78-86 `matrix`, float64, C-contiguous).
 * Each rank uploads only its own units. */
BB_API int bb_solver_set_wish_dense(bb_solver *s, const double *host, int64_t ld, int kind,
                                    double alpha);
/* SEVERAL MAPS IN ONE SOLVER.  The reference's ContactMap is per chromosome
 * (blueberry/datatypes.pyx:88), so the common job is 23 maps of 1,000-5,000 bins, each of
 * which alone is launch-bound (5-20 us per iteration whatever its size).  Laid end to end --
 * map m owns the bins [bin_begin[m], bin_begin[m+1]), every map starting at a multiple of the
 * tile edge, the solver created with the tile list of the maps' own dense triangles (no tile
 * joins two maps) -- they are ONE blocked-sparse problem: one sweep and one reduce per
 * iteration for all of them.
 *   bb_solver_set_maps            declare the maps (world = 1); map m steps with
 *                                 lr * lr_scale[m] (bb_solver_iterate's lr times it: pass
 *                                 lr = 1 and lr_scale[m] = 1 / (2 n_m) for the SMACOF step),
 *                                 and the stress is kept PER MAP: bb_solver_get_stress_history
 *                                 then returns n_maps values per iteration (iteration-major)
 *   bb_solver_set_wish_dense_block  map m's (n_sub, n_sub) host matrix into its bins
 *                                 [bin_offset, bin_offset + n_sub); as bb_solver_set_wish_dense.
 *                                 A map ends where its last tile ends: the pairs of the tiles
 *                                 the block touches that lie outside the block are cleared
 *                                 (no constraint); other tiles keep what they hold
 *   bb_solver_stress_maps         per-map stress of the current coordinates
 * Coordinates travel as one (n_bins, 3) array (rows between the maps are padding: 0). */
BB_API int bb_solver_set_maps(bb_solver *s, int n_maps, const int64_t *bin_begin,
                              const double *lr_scale);
BB_API int bb_solver_set_wish_dense_block(bb_solver *s, const double *host, int64_t ld,
                                          int64_t n_sub, int64_t bin_offset, int kind, double alpha);
BB_API int bb_solver_stress_maps(bb_solver *s, double *stress, int n_maps);
/* A STEP PER BIN: bin i moves by lr * scale[i] * g_i.  SPEC 2.4's step 1 / (2 N) is the
 * Guttman transform of a COMPLETE map; in an incomplete one the bins do not all have N - 1
 * partners -- the whole genome at 10 kb as blocks: 24,926 for a bin of chr1, 4,813 for one of
 * chr21; inside a real chromosome's block most long-range pairs have no contact at all -- and
 * the one step the largest degree allows is many times too short for the rest.  With
 * scale[i] = (D + 1) / (degree[i] + 1), D the largest degree, and lr = 1 / (2 (D + 1)) every
 * bin takes the step 1 / (2 (degree[i] + 1)) its own number of partners allows (SPEC 2.4.1:
 * still a descent step; on a genome-like tile list 1e-3 of the start's stress in a third of
 * the iterations).
 *   bb_solver_degrees          per bin, how many of THIS rank's stored pairs constrain it
 *                              (delta > 0): one pass over the resident units; world > 1: the
 *                              caller sums the counts over the ranks
 *   bb_solver_set_bin_steps    the factors, one per bin (finite, > 0); NULL: one step for all
 *   bb_solver_set_block_steps  the same from one factor per block of the layout
 *                              (bb_solver_layout: n_blocks blocks of vw bins) -- what a tile
 *                              list alone gives, without a pass over the data
 * The gradient of bin i is scaled where it leaves the reduce -- into the update, the
 * exchange buffer (bb_solver_grad then holds scale * g) or the peers' arenas -- so it works
 * on any number of ranks with every exchange; every rank passes the same factors (maps of at
 * most 4,096 bins on one rank keep their one launch per iteration: its kernel scales too).
 * On a solver of several maps the factors REPLACE the per-map steps of bb_solver_set_maps
 * (pass lr = 1 to bb_solver_iterate and scale[i] = the step of bin i, e.g.
 * 1 / (2 (degree[i] + 1)); clearing them there is BB_ERR_STATE).  BB_ERR_STATE while a
 * bb_solver_grad is pending.  No counterpart in the reference (it has no solver;
 * SURVEY.md 0). */
BB_API int bb_solver_degrees(bb_solver *s, int64_t *degree, int64_t n_bins);
BB_API int bb_solver_set_bin_steps(bb_solver *s, const double *scale, int64_t n_bins);
BB_API int bb_solver_set_block_steps(bb_solver *s, const double *scale, int64_t n_blocks);
/* Weighted stress (docs/SPEC.md 2.3.1): every pair's residual weighted by w = delta^-q,
 *   q = 0  raw stress (the default; bit for bit the unweighted solver)
 *   q = 1  Sammon stress, w = 1 / delta
 *   q = 2  relative stress, w = 1 / delta^2: sum ((d - delta) / delta)^2
 * Pairs without a constraint (delta = 0) contribute 0.  Every entry point that evaluates the
 * stress -- bb_solver_iterate / _dist / _peer, bb_solver_grad, bb_solver_stress, _stress_maps
 * -- then reports and descends S_q; the spectral start (bb_solver_matvec_sq and
 * bb_solver_spectral_init*) stays unweighted.
 *   bb_solver_set_weight_power  q in {0, 1, 2} (else BB_ERR_INVALID); callable any time after
 *                               bb_solver_create, also between iterate calls (BB_ERR_STATE
 *                               while a bb_solver_grad is pending).  The stress history is
 *                               NOT reset: each entry is the S_q in effect at its step
 *   bb_solver_weight_sums       per bin, s_i = sum_j w_ij over THIS rank's stored pairs, in
 *                               fp64 and in a fixed order (bitwise reproducible); q = 0 gives
 *                               the degrees.  The weighted counterpart of bb_solver_degrees
 *                               for SPEC 2.4.1's steps; world > 1: the caller sums over the
 *                               ranks */
BB_API int bb_solver_set_weight_power(bb_solver *s, int q);
BB_API int bb_solver_weight_sums(bb_solver *s, double *sums, int64_t n_bins);
/* Blocked-sparse input: nnz entries (rows[k], cols[k], vals[k]) of the symmetric
 * matrix, either triangle; an unordered pair that occurs more than once keeps its
 * LAST entry, as in the reference's scatter loop (blueberry/datatypes.pyx:110-116)
 * and in bb_contactmap_scatter.  Every entry must fall in a
 * tile of the solver's tile list; all other pairs carry no constraint.  This
 * is the form of the reference's own input files -- sparse (pos_i, pos_j,
 * count) triples (blueberry/datatypes.pyx:31-38, :100-102) -- without the
 * dense (n_bins+1)^2 host matrix, for genome-wide 10 kb maps (BASELINE config 5).
 * KRnorm / KRexpected (n_bins doubles each, or both NULL): each value is first
 * divided by KRnorm[i] * KRnorm[j] * KRexpected[j - i] (i < j), the element-wise
 * form of ContactMap.normalize (blueberry/datatypes.pyx:166-169), followed by the
 * reference's nan_to_num (pyx:171): a NaN quotient is 0 = "no constraint", an overflowing
 * one the largest double (whose wish distance, 1.8e-103, is a constraint in fp64 and
 * below the wish floor in fp32) -- exactly what the dense ContactMap path gives. */
BB_API int bb_solver_set_wish_sparse(bb_solver *s, const int64_t *rows, const int64_t *cols,
                                     const double *vals, int64_t nnz, int kind, double alpha,
                                     const double *KRnorm, const double *KRexpected);
/* The same input WITHOUT host-side binning: the (n, 3) float64 array [pos_i, pos_j, count] of a
 * Rao-format file exactly as ContactMap.__init__ holds it (blueberry/datatypes.pyx:100-102),
 * copied to the device once.  row_major != 0: C-ordered (n, 3) rows; 0: the reference's
 * column-major array (pyx:111-113 read it that way).  numpy.nan_to_num (pyx:102) and
 * bin = (int)(pos / resolution) (pyx:111-112) are applied by the kernels as they read.
 *   bb_triples_tiles            which tiles of the (n_bins, dtype) layout the triples name:
 *                               present[I * n_blocks + J] = 1, I <= J (n_blocks^2 bytes) -- the
 *                               tile list to create the solver with
 *   bb_solver_set_wish_triples  as bb_solver_set_wish_sparse (last entry of a pair wins,
 *                               KRnorm / KRexpected optional), from the resident triples */
typedef struct bb_triples bb_triples;
BB_API int bb_triples_create(bb_triples **out, const double *triples, int64_t n, int32_t resolution,
                             int32_t row_major, int device);
BB_API int bb_triples_destroy(bb_triples *t);
BB_API int bb_triples_tiles(const bb_triples *t, int64_t n_bins, int dtype, uint8_t *present,
                            int64_t n_blocks);
BB_API int bb_solver_set_wish_triples(bb_solver *s, const bb_triples *t, int kind, double alpha,
                                      const double *KRnorm, const double *KRexpected);
/* Synthetic input generated on the device: delta_ij = |x*_i - x*_j| for the
 * (n_bins,3) float64 host coordinates `xstar`, so that
 * N = 50k needs no 20 GB host matrix. */
BB_API int bb_solver_set_wish_from_coords(bb_solver *s, const double *xstar);

BB_API int bb_solver_set_coords(bb_solver *s, const double *xyz); /* (n_bins,3) f64 host */
BB_API int bb_solver_get_coords(bb_solver *s, double *xyz);

/* Heavy-ball momentum (SPEC 2.4): V <- mu V - lr g, X <- X + V, V = 0 after
 * bb_solver_set_coords.  mu = 0 (the default) is the plain gradient step. */
BB_API int bb_solver_set_momentum(bb_solver *s, double mu);

/* world = 1: `iters` iterations of { stress + gradient, update }, enqueued
 * back to back; stress history is kept on the device (2^20 entries: more iterations than
 * that since the last bb_solver_set_coords are refused with BB_ERR_STATE before anything is
 * enqueued -- read the history out and set the coordinates again to go on). */
BB_API int bb_solver_iterate(bb_solver *s, int64_t iters, double lr);

/* world > 1 (also valid for world = 1): one iteration in two halves around
 * the caller's all-reduce(sum) of the exchange buffer.
 *   bb_solver_grad : this rank's partial gradient and stress -> exchange buffer
 *   bb_solver_apply: X <- X - lr * exchange[0:3*n_pad]; records the stress    */
BB_API int bb_solver_grad(bb_solver *s);
BB_API int bb_solver_apply(bb_solver *s, double lr);
/* The exchange buffer: 3*n_pad + 2 elements of the solver's dtype,
 * [ g (n_pad,3) | stress hi | stress lo ].  By default owned by the solver;
 * a caller that needs to hand it to a collective library may supply its own
 * device allocation of that size. */
BB_API int bb_solver_exchange_size(const bb_solver *s, int64_t *n_elems);
BB_API int bb_solver_get_exchange_buffer(bb_solver *s, void **dev_ptr);
BB_API int bb_solver_set_exchange_buffer(bb_solver *s, void *dev_ptr);
/* Direct RCCL path: the library loads librccl at run time and owns a
 * communicator, so the whole multi-rank iteration is enqueued from C on the
 * solver's own stream -- no framework in the loop.
 *   bb_comm_unique_id      one rank makes the 128-byte id (ncclGetUniqueId) ...
 *   bb_solver_comm_init    ... every rank passes it in (ncclCommInitRank; collective)
 *   bb_solver_allreduce    in-place sum of the exchange buffer, between grad and apply
 *   bb_solver_iterate_dist `iters` x { grad, allreduce, apply }; a call the stress history
 *                          cannot hold is refused with BB_ERR_STATE before anything is
 *                          enqueued, as bb_solver_iterate's
 * The id travels by whatever the caller has (MPI_Bcast, torch.distributed, a file). */
BB_API int bb_comm_unique_id(void *id_out_128_bytes);
BB_API int bb_solver_comm_init(bb_solver *s, const void *unique_id_128_bytes);
BB_API int bb_solver_allreduce(bb_solver *s);
BB_API int bb_solver_iterate_dist(bb_solver *s, int64_t iters, double lr);
/* Number of ranks RCCL reports for the library's communicator (ncclCommCount): what the
 * bench line quotes as the world size that really took part in the collective. */
BB_API int bb_solver_comm_world(const bb_solver *s, int *world);
/* Give the communicator up (ncclCommAbort): ends a collective that a peer never
 * joined, so the solver's stream drains again.  The solver falls back to
 * bb_solver_grad / caller's all-reduce / bb_solver_apply. */
BB_API int bb_solver_comm_abort(bb_solver *s);
/* The communicator a bb_solver_comm_init makes is kept by the library for the life of the
 * process, one per (device, rank, world); a solver borrows it and hands it back when it is
 * destroyed.  Later solvers of the same job skip ncclCommInitRank:
 *   bb_comm_cached          *available = 1 if a free communicator for this key is held
 *   bb_solver_comm_attach   borrow it (every rank of the job must take the same path: agree
 *                           on `available` first -- the Python wrapper all-reduces a MIN)
 *   bb_solver_comm_detach   hand a borrowed one back without using it
 *   bb_comm_cache_clear     destroy the communicators no solver holds (ncclCommDestroy) */
BB_API int bb_comm_cached(int device, int rank, int world, int *available);
/* The same with the cached communicator's GENERATION: a hash of the unique id its
 * ncclCommInitRank was given -- equal on the ranks that made it together, different for any
 * other communicator of the same (device, rank, world), e.g. one left over from an earlier
 * process group or made while another rank's solver still held the previous one.  The ranks
 * must hold the SAME generation before any of them attaches (the Python wrapper all-gathers
 * it); 0 when nothing is available.  A communicator whose collective failed to enqueue, or
 * that bb_solver_comm_abort gave up, never returns to the cache. */
BB_API int bb_comm_cached_generation(int device, int rank, int world, int *available,
                                     uint64_t *generation);
BB_API int bb_solver_comm_attach(bb_solver *s);
BB_API int bb_solver_comm_detach(bb_solver *s);
BB_API int bb_comm_cache_clear(void);

/* Peer exchange: a one-shot all-reduce over xGMI written into the solver's own
 * kernels -- no collective library in the loop.  Every rank owns a receive
 * arena (uncached device memory, 2 parities x world slots of the exchange
 * vector + one sequence flag per source rank) that the other ranks map through
 * HIP IPC.  The last reduce launch of an iteration stores this rank's partial
 * gradient straight into its slot on every peer and then raises its flag there;
 * the update kernel waits (bounded) for all `world` flags, sums the slots in
 * RANK ORDER -- bit-identical coordinates on every rank -- and applies the step.
 *   bb_solver_peer_export   allocate the arena, write its handle (BB_PEER_HANDLE_BYTES)
 *   bb_solver_peer_connect  map the arenas of all ranks (handles in rank order;
 *                           collective: every rank must have exported)
 *   bb_solver_iterate_peer  `iters` x { grad, reduce+push, wait+sum+apply }; BB_ERR_STATE,
 *                           nothing enqueued, for a call the stress history cannot hold (as
 *                           bb_solver_iterate) and for a solver of several maps
 *                           (bb_solver_set_maps: the exchange records one stress per iteration)
 *   bb_solver_peer_status   0 = healthy; 1 = a wait ran into the time limit
 *                           (BB_PEER_TIMEOUT_MS, default 10000) or a peer reported
 *                           its own failure: this call reports BB_ERR_STATE
 *   bb_solver_peer_set_timeout  change that limit (a short one for a trial run)
 *   bb_solver_peer_form     1 = the one-launch form below, 0 = the two launches above
 * One-launch form (the default with one rank per GPU): the unit of exchange is what one
 * workgroup of the reduce sums anyway, 128 gradient elements of one block.  Each thread that
 * holds a sum stores it into its rank's slot on every peer, reads the same element of every
 * rank's slot in its own arena until all have ARRIVED, adds the `world` partials in rank
 * order, updates its coordinate and marks the words it read as empty again: { grad, exchange }
 * per iteration, no flags and no fences -- an empty slot word holds all-ones (a NaN that no
 * arithmetic produces; a sum that should ever carry those bits is sent as the canonical NaN),
 * a 4- or 8-byte store is seen whole or not at all, and nothing else is published with it.
 * Nobody waits for any workgroup but the owners of the same elements.  Every
 * workgroup pushes before it waits and workgroups start in index order, so the lowest
 * unfinished one can always finish -- if each rank has its GPU to itself.  bb_solver_peer_connect
 * sees from the handles (PCI ids) whether ranks SHARE a GPU (a rehearsal) and then keeps the
 * two-launch form: waiting workgroups of one rank can keep another rank's sweep off the
 * device.  BB_PEER_FUSED=0|1 overrides, identically on every rank.
 * Failure.  Two-launch form: decided ONCE per iteration, by one wave, for the whole update:
 * X is advanced by a complete step or not at all.  One-launch form: every wave decides
 * for its 64 elements, so a rank that dies in the middle of an exchange can leave its
 * peers with part of a step applied; when nothing of an exchange arrives (a rank that is
 * late, stalled or gone) no workgroup applies anything.  Either way the failed rank stops
 * pushing and leaves a poison word on every peer, so their waits fail at once as well -- no
 * rank goes on consuming partials of coordinates that no longer move -- the status is
 * sticky, and the coordinates of a solver whose status is not 0 are not a result.
 * Who sends what.  Rank q's units lie in tiles (I, J) and carry gradient for the bins of
 * blocks I and J only; its partial for every other block is zero by construction.  Every rank
 * derives the same table (block -> ranks that touch it) from the tile list and the partition
 * at bb_solver_peer_connect, and in both forms a rank pushes a block only if it is in the
 * block's set, and nobody waits for, reads or adds the slot of a rank that is not: not one
 * bit of the result changes (the zeros were added as zeros), but a dense map on 8 ranks sends
 * 72 % of the bytes (rank 0 touches the first third of the blocks), the whole genome as
 * blocks 15 % (a rank's share touches the blocks of a few chromosomes).  BB_PEER_MASK=0:
 * every rank sends every block.
 * The handles travel by whatever the caller has (MPI_Allgather, torch.distributed,
 * a file).  All ranks must be on one node with peer access between their GPUs. */
#define BB_PEER_HANDLE_BYTES 128
BB_API int bb_solver_peer_export(bb_solver *s, void *handle_out);
BB_API int bb_solver_peer_connect(bb_solver *s, const void *handles_rank_order);
BB_API int bb_solver_iterate_peer(bb_solver *s, int64_t iters, double lr);
BB_API int bb_solver_peer_status(bb_solver *s, int *status);
BB_API int bb_solver_peer_set_timeout(bb_solver *s, int64_t milliseconds);
BB_API int bb_solver_peer_form(bb_solver *s, int *one_launch);
/* Choose the form after bb_solver_peer_connect and before the first exchange (identically on
 * every rank): 0 = the two launches, 1 = the one launch.  The one-launch form rests on
 * properties of remote stores over xGMI that no one-GPU test can exercise; the Python host
 * therefore keeps the two-launch form for a fit() that was not preceded by a trial against
 * RCCL (BB_COMM=peer without BB_COMM_TRIAL / BB_PEER_FUSED), and takes the one-launch form
 * where a trial has compared its coordinates with RCCL's (bench.py). */
BB_API int bb_solver_peer_set_form(bb_solver *s, int one_launch);

/* Several GPUs driven from ONE process: a group of existing solvers, member r = rank r of world
 * n, all with the same n_bins, dtype and tile list (else BB_ERR_INVALID naming the mismatch).
 * Every setter stays the per-solver call (wish distances, coordinates, momentum, bin steps,
 * weight power: the same values on every member); the group only iterates them.
 *   bb_group_create   enables peer access between the members' DISTINCT devices (a device may
 *                     repeat: members then share it -- a rehearsal) and starts one host thread
 *                     per member on the member's device
 *   bb_group_iterate  `iters` x, on every member's stream: wait for every member's "applied"
 *                     event of the previous step; grad (bb_solver_grad's two launches); record
 *                     "ready"; host barrier; wait for every member's "ready"; group_apply_kernel
 *                     (the R partials summed in rank order, read straight from the members'
 *                     exchange buffers; the update; the stress); record "applied"; host barrier.
 *                     No kernel waits for another, so members can share a GPU and its hardware
 *                     queues in any number.  The sums are those of the two-launch peer exchange
 *                     at the same world size: bit-identical members and results.  Stress history
 *                     as bb_solver_iterate (BB_ERR_STATE past its capacity, nothing enqueued).  A
 *                     member that fails to enqueue makes every thread stop at the next barrier;
 *                     the call returns its error.  No synchronisation at the end.
 *   bb_group_destroy  joins the threads and drains the members' streams; the members stay
 *                     (destroy the group first, then them)
 * No counterpart in the reference (it has no solver; its one multi-GPU idiom is a device list
 * handed to one constructor). */
typedef struct bb_group bb_group;
BB_API int bb_group_create(bb_group **out, bb_solver *const *members, int n);
BB_API int bb_group_iterate(bb_group *g, int64_t iters, double lr);
BB_API int bb_group_destroy(bb_group *g);

/* Host-staged access to the exchange buffer, widened to float64, for callers
 * whose collective runs on host memory (MPI, gloo): read after bb_solver_grad,
 * sum over ranks, write back, then bb_solver_apply.  n = bb_solver_exchange_size. */
BB_API int bb_solver_read_exchange(bb_solver *s, double *host, int64_t n);
BB_API int bb_solver_write_exchange(bb_solver *s, const double *host, int64_t n);

/* Y = (D o D) X for this rank's resident units: y_i = sum_j delta_ij^2 x_j over
 * the symmetric matrix of squared wish distances (absent pairs count 0), for
 * three right-hand sides at once; x, y are (n_bins,3) float64 on the host.  One
 * sweep of the same kernel and layout as the gradient.  With world > 1 the
 * caller sums y over the ranks.  It is the operator of classical-MDS / spectral
 * initialisation -- the role SURVEY.md 8(f)-2 gives the reference's
 * ContactMap.eigenvector (blueberry/datatypes.pyx:216-235).  A stored distance whose
 * square overflows the solver's dtype (above 1.8e19 in fp32, 1.3e154 in fp64) makes
 * delta^2 = +inf: the rows of that pair are then not finite, and rows next to them may be
 * NaN as well (the sweep folds the sums of neighbouring rows in one reduction, inf * 0). */
BB_API int bb_solver_matvec_sq(bb_solver *s, const double *x, double *y);

/* Classical-MDS start computed and LEFT on the device: `n_iter` block power iterations on
 * B = -1/2 J (D o D) J over the resident units (one sweep each, as bb_solver_matvec_sq) from
 * the (n_bins,3) host start `v0`, Cholesky-QR between them, a 3 x 3 Rayleigh-Ritz step,
 * X0 = V sqrt(Lambda) written straight into the solver's coordinates (history and velocity
 * reset, as bb_solver_set_coords).  The N x 3 algebra of the loop -- centring, Gram matrices,
 * the 3 x 3 Cholesky factors and the maps they define -- runs in kernels that hand their
 * results to one another in device memory: no host round trip per product, three reads of
 * 12 doubles for the whole start.  world > 1: collective; every rank passes the same v0, the
 * per-rank products are summed over the ranks on the device through the exchange the solver
 * already has (bb_solver_peer_connect, or bb_solver_comm_init / _attach; BB_ERR_STATE without
 * one), and every rank ends with the same coordinates.  BB_ERR_STATE "lost rank" when the
 * iterate has fewer than 3 independent directions (coordinates untouched).  The role
 * SURVEY.md 8(f)-2 gives ContactMap.eigenvector as the solver's initialisation
 * (blueberry/datatypes.pyx:216-235). */
BB_API int bb_solver_spectral_init(bb_solver *s, int n_iter, const double *v0);

/* The same start with a stopping rule: `n_iter` is the most products the loop makes; after
 * every product but the first the relative distance of Z = B V from span(V),
 * ||Z - V (V^T Z)||_F / ||Z||_F, is read back (24 doubles) and the loop ends
 * once it is below `tol` (0 = never: exactly bb_solver_spectral_init; the difference of sums
 * it is formed from resolves it down to about 1e-7, the fp32 sweep to about 1e-6).  A complete
 * noise-free map has rank 3 and ends after two products instead of `n_iter`; a noisy or
 * incomplete one runs until the third and fourth eigenvalue have separated that far.
 * `iters_done` (optional) = orthonormalised products made; `residual` (optional) = the last
 * distance read, -1 if none was.  world > 1: the ranks hold identical V and Z, so all of them
 * leave at the same product. */
BB_API int bb_solver_spectral_init_tol(bb_solver *s, int n_iter, double tol, const double *v0,
                                       int *iters_done, double *residual);

/* Stress of the current coordinates (one gradient pass, no update). */
BB_API int bb_solver_stress(bb_solver *s, double *stress);
/* How well a structure fits the resident map (docs/SPEC.md 2.8): ONE pass over this rank's
 * units, no iteration, float64 sums over the stored pairs i < j < n_bins with delta > 0,
 * d = |x_i - x_j| without a floor.
 *   profile  (n_bins, 9), row k = the pairs of genomic separation j - i = k (row 0 is zero):
 *            pairs, sum d, sum delta, sum d^2, sum delta^2, sum d delta, sum (d - delta)^2,
 *            sum (d - delta)^2 / delta, sum ((d - delta) / delta)^2
 *   bins     (n_bins, 3), row i = the pairs that hold bin i: pairs, sum (d - delta)^2,
 *            sum ((d - delta) / delta)^2
 * The counts are exact doubles; the residual columns are summed as written, never formed from
 * the moments.  xyz: the (n_bins, 3) structure to score, or NULL for the solver's own
 * coordinates widened to float64.  No floating-point atomics, every sum in an order fixed by
 * the layout and the rank's unit range: the same bits on every call.  world > 1: the caller
 * sums both arrays over the ranks (as bb_solver_degrees); a rank without units gives zeros.
 * Nothing of the solver changes: coordinates, velocity, stress history and per-bin steps stay.
 * BB_ERR_STATE before wish distances are set, while a bb_solver_grad is pending, for a solver
 * of several maps, and for xyz == NULL before coordinates are set; BB_ERR_INVALID for xyz that
 * is not finite.  The scratch of a call, released before it returns:
 * runs * (2 vw - 1) * 72 bytes, a run being this rank's units of one tile, + 96 n_bins.
 *   bb_solver_get_score_timing  HIP-event times (ms) of the last call's three kernels --
 *                               profile, fold, per bin -- made while bb_solver_set_timing was
 *                               on (else 0); any pointer may be NULL
 * No counterpart in the reference (it has no solver). */
BB_API int bb_solver_score(bb_solver *s, const double *xyz, double *profile, double *bins);
BB_API int bb_solver_get_score_timing(bb_solver *s, double *profile_ms, double *fold_ms,
                                      double *bins_ms);
/* Inferring the count-to-distance exponent (docs/SPEC.md 2.11): the two device passes of the
 * search StructureSolver(alpha='auto') runs; the search itself is the caller's.
 *   bb_solver_loglog   the log-log sums of a structure against the resident map, over the
 *                      pairs of bb_solver_score (stored, i < j < n_bins, delta > 0) and with its
 *                      d: profile (n_bins, 7), row k = the pairs of separation k: pairs with
 *                      d > 0, sum u, sum v, sum u^2, sum v^2, sum u v (u = log delta, v = log d,
 *                      float64), and the pairs with d = 0, which add nothing else (a d that is
 *                      not a number -- xyz = NULL after a fit that diverged -- counts there
 *                      too: check the solver's own coordinates before relying on it).  Same pass,
 *                      same order of every sum, same state rules, same errors and the same xyz
 *                      as bb_solver_score; scratch runs * (2 vw - 1) * 56 bytes + 56 n_bins.
 *                      With bb_solver_set_timing on, bb_solver_get_score_timing then reports
 *                      this call's profile and fold kernels (bins_ms = 0).
 *   bb_solver_repower  every stored word w > 0 of this rank's units becomes pow((double)w, p),
 *                      taken as a BB_KIND_WISH input (floor, ceiling, rounding to the dtype);
 *                      zeros stay.  delta = c^(-1/a) thereby becomes c^(-1/a') for p = a / a'
 *                      without the input.  The row-owner matrix is rebuilt, the 24-bit stream
 *                      is stale; degrees and weight sums are the caller's to recompute (pairs
 *                      may have left by the floor or the ceiling).  Coordinates, velocity and
 *                      stress history stay.  BB_ERR_INVALID unless p is finite and > 0;
 *                      BB_ERR_STATE before wish distances are set, while a bb_solver_grad is
 *                      pending, and with landmark anchors set (geodesic rows are no power of
 *                      anything). */
BB_API int bb_solver_loglog(bb_solver *s, const double *xyz, double *profile);
BB_API int bb_solver_repower(bb_solver *s, double p);
/* Copies the stress history (one value per completed iteration since the
 * last bb_solver_set_coords) to the host; synchronises the stream. */
BB_API int bb_solver_get_stress_history(bb_solver *s, double *out, int64_t cap, int64_t *n);
BB_API int bb_solver_sync(bb_solver *s);
/* The same with a bound: BB_ERR_STATE if the stream has not drained after
 * `milliseconds` (polls hipStreamQuery; the work stays enqueued). */
BB_API int bb_solver_sync_timeout(bb_solver *s, int64_t milliseconds);

/* HIP-event timing of the dominant kernel (stress+gradient) and of the
 * reduce/update kernel on the solver's stream.  Averages are over the timed
 * launches since timing was (re-)enabled.  enabled = 1: every iteration is
 * timed; enabled = k > 1: every k-th one (three event records cost about 10 us
 * of stream time per timed iteration on MI355X, which matters once a step is
 * ~0.1 ms); 0: off. */
BB_API int bb_solver_set_timing(bb_solver *s, int enabled);
BB_API int bb_solver_get_timing(bb_solver *s, double *grad_ms_avg, double *reduce_ms_avg,
                                int64_t *launches);
/* The same events, start of one timed iteration to start of the next: the whole
 * device-side step including the exchange, the update and the gaps between
 * launches (average over consecutive timed iterations; 0 with fewer than two). */
BB_API int bb_solver_get_step_timing(bb_solver *s, double *step_ms_avg);
/* What a pair of HIP events costs by itself on the solver's stream: the average time
 * between two events recorded back to back behind a sweep launch (`pairs` of them): an
 * upper bound of what an event-timed interval contains besides its kernel (bench.py
 * reports it beside its event-timed figures; it subtracts nothing). */
BB_API int bb_solver_measure_event_gap(bb_solver *s, int pairs, double *ms_avg);
/* Measurement aid: average duration of a kernel that only READS this rank's
 * resident units (same grid, same per-wave chunks, same 8-row window, no
 * arithmetic) -- the practical HBM ceiling for the access pattern, to put
 * beside the spec peak in the roofline. */
BB_API int bb_solver_measure_stream_read(bb_solver *s, int launches, double *ms_avg);
/* Which kernel bb_solver_iterate runs: row_owner = 1 for the one-launch-per-iteration
 * path of small one-rank maps (both triangles resident; waves_per_row waves per bin),
 * 0 for the unit sweep + reduce.  Either pointer may be NULL. */
BB_API int bb_solver_iteration_path(const bb_solver *s, int *row_owner, int *waves_per_row);
/* Bytes of wish-distance data the stress+gradient kernel streams per launch on
 * this rank (resident units * unit bytes, or the bytes of the 24-bit stream where the
 * fp32 sweep reads that: bb_solver_stream_info), and pairs evaluated. */
BB_API int bb_solver_traffic(bb_solver *s, int64_t *unit_bytes, int64_t *pairs_dense);
/* The 24-bit stream of the fp32 stress sweep (docs/SPEC.md 3.7): a copy of this rank's units
 * in which every unit whose 2,048 stored words, as uint32, span less than 2^24 is held as 6 KiB
 * of lossless offset codes where at least BB_PACK24_MIN_RUN (64) such units follow each other,
 * and as its 8 KiB otherwise.  Built from the units before the first sweep after the wish
 * distances were set, where it saves an eighth of the bytes of a sweep that streams from HBM
 * (BB_PACK24=1 at create: wherever a unit packs, =0: never); results do not depend on it.
 * Returns the units held packed and raw, the stream's bytes and the changes of format between
 * consecutive units; with no stream in use: 0, all units, 0, 0.  Pointers may be NULL. */
BB_API int bb_solver_stream_info(bb_solver *s, int64_t *packed_units, int64_t *raw_units,
                                 int64_t *stream_bytes, int64_t *format_switches);

/* ---------------------------------------------------------------------- */
/* A2/A3/A4  the ContactMap stage, resident on the device                   */
/*        (reference: blueberry/datatypes.pyx:97-116, :161-171, :122-141)   */
/* ---------------------------------------------------------------------- */

/* One (d, d) float64 matrix, d = n_bins + 1, that stays in HBM across
 * scatter -> normalize -> filter -> solver, as `ContactMap.matrix` stays in host
 * memory across the same calls in the reference (datatypes.pyx:97-120, :161-171,
 * :140-141).  No matrix-sized host transfer happens unless the caller asks for
 * one (bb_cm_upload / bb_cm_download).  Every operation is bit-exact fp64. */
typedef struct bb_cm bb_cm;
BB_API int bb_cm_create(bb_cm **out, int64_t d, int device);   /* zero-filled (pyx:99) */
BB_API int bb_cm_destroy(bb_cm *cm);
BB_API int bb_cm_dim(const bb_cm *cm, int64_t *d);
/* The resident matrix itself (row-major, leading dimension d) for callers that share
 * the HIP context; borrowed, valid until bb_cm_destroy (bb_cm_filter changes d). */
BB_API int bb_cm_device_ptr(const bb_cm *cm, const double **dev_matrix, int64_t *d, int *device);
BB_API int bb_cm_upload(bb_cm *cm, const double *matrix, int64_t ld);   /* host (d,d) -> device */
BB_API int bb_cm_download(bb_cm *cm, double *matrix, int64_t ld);       /* device -> host (d,d) */
/* ContactMap.__init__'s loop (pyx:110-116): zero the matrix, then for every triple
 * (column-major `triples`, as bb_contactmap_scatter) set [j][k] and [k][j]; later
 * triples overwrite earlier ones.  Needs no scratch the size of the matrix. */
BB_API int bb_cm_scatter(bb_cm *cm, const double *triples, int64_t n, int32_t resolution);
/* The same with two conveniences for a caller that holds C-ordered rows and wants
 * `regions` (pyx:120, numpy.union1d of the two position columns) without sorting 2n
 * doubles: row_major != 0 reads `triples` as (n, 3) rows instead of the reference's
 * column-major (3, n); `present` (d bytes) receives 1 for every bin some position falls
 * in and *on_grid 1 if every position equals bin * resolution exactly -- then regions
 * are the present bins times the resolution, bit for bit.  present / on_grid may both
 * be NULL. */
BB_API int bb_cm_scatter_ex(bb_cm *cm, const double *triples, int64_t n, int32_t resolution,
                            int32_t row_major, uint8_t *present, int32_t *on_grid);
/* ContactMap.normalize (pyx:161-171), in place: m[j][j+i] /= KRnorm[j]*KRnorm[j+i]*
 * KRexpected[i], mirrored, then nan_to_num over the whole matrix.  d must be n_bins+1. */
BB_API int bb_cm_normalize(bb_cm *cm, int64_t n_bins, const double *KRnorm,
                           const double *KRexpected);
/* Column marginals `matrix.sum(axis=0)` (pyx:140), d doubles to the host: rows are
 * added in order, which is bit for bit what numpy computes. */
BB_API int bb_cm_marginals(bb_cm *cm, double *sums);
/* ContactMap.filter (pyx:140-141): keep the rows and columns whose marginal is
 * > threshold (a NaN marginal is dropped, as `NaN > t` is false in numpy).  The
 * resident matrix becomes (d_new, d_new), compacted in place (same device pointer, leading
 * dimension d_new; the allocation keeps its size); keep_out (d bytes, may be NULL)
 * receives the 0/1 mask over the OLD indices. */
BB_API int bb_cm_filter(bb_cm *cm, double threshold, int64_t *d_new, uint8_t *keep_out);
/* y = M x over the resident matrix (x, y: d doubles on the host): one HBM sweep. */
BB_API int bb_cm_symv(bb_cm *cm, const double *x, double *y);
/* ContactMap.eigenvector (pyx:216-235: scipy.sparse.linalg.eigsh(matrix, k=1), i.e.
 * ARPACK's eigenpair of LARGEST MAGNITUDE): restarted Lanczos with full
 * re-orthogonalisation over the resident matrix, one HBM sweep per matrix-vector
 * product.  Stops when |M v - lambda v| <= tol * |lambda| or after max_matvecs products.
 * vec: d doubles, unit length, largest-magnitude component positive (ARPACK's sign is
 * arbitrary).  eigenvalue / matvecs_used / residual may be NULL. */
BB_API int bb_cm_eigenvector(bb_cm *cm, double *vec, double *eigenvalue, double tol,
                             int64_t max_matvecs, int64_t *matvecs_used, double *residual);
/* ContactMap.correlation (pyx:173-188): matrix <- numpy.corrcoef(matrix), in place on the
 * resident matrix: rows centred, Gram matrix on the fp64 matrix cores
 * (v_mfma_f64_16x16x4_f64; the one dense contraction on this path), scaled and clipped
 * in numpy's order of operations.  Equal to numpy to rounding (BLAS sums in another
 * order).  tflops (may be NULL): rate of the Gram kernel alone, by HIP events. */
BB_API int bb_cm_correlation(bb_cm *cm, double *tflops);
/* bb_cm_correlation's temporaries (centred rows + Gram matrix, about 2x the matrix) live in one
 * grow-only scratch per device, shared by every map on it; this frees it (it is made again by
 * the next call that needs it). */
BB_API int bb_cm_release_scratch(int device);
/* Completion by shortest paths (docs/SPEC.md 2.1.1): dst <- the all-pairs shortest-path lengths
 * of the graph whose edges are src's wish distances -- c^(-1/alpha) of every finite positive
 * entry of the upper triangle for kind = BB_KIND_COUNTS, the entry itself for BB_KIND_WISH; any
 * other entry is no edge and the diagonal is ignored.  dst gets a 0 diagonal and 0 ("no
 * constraint") where no path exists; it is symmetric bit for bit, float64, and a BB_KIND_WISH
 * input for the solver.  Blocked Floyd-Warshall on the device, no atomics, the same bits on
 * every run.  dst has src's edge and device; dst == src works in place.  The work matrix (the
 * edge rounded up to 64, squared, x 8 bytes) comes from the scratch bb_cm_release_scratch
 * frees; if it cannot be allocated: BB_ERR_NOMEM with both sizes in the message, nothing
 * changed.  alpha <= 0, an unknown kind, a mismatch of edge or device: BB_ERR_INVALID.
 * unreachable_pairs (may be NULL): the number of pairs i < j without a path. */
BB_API int bb_cm_shortest_paths(const bb_cm *src, bb_cm *dst, int kind, double alpha,
                                int64_t *unreachable_pairs);
/* Balancing of a raw map (docs/SPEC.md 2.5.2), over the leading n_bins x n_bins block of the
 * resident matrix (d must be n_bins + 1; row and column n_bins are never read).  Only the upper
 * triangle is read and the matrix is taken to be symmetric, as bb_cm_symv takes it.  Float64, no
 * floating-point atomics, every sum in an order fixed by n_bins alone: the same bits on every
 * run.  Neither call changes the matrix.
 *
 * bb_cm_balance: the bias vector of iterative correction (Imakaev et al. 2012) over the counted
 * cells A_ij = M_ij, |i - j| >= ignore_diags.  A counted cell of the upper triangle that is
 * negative or not finite: BB_ERR_INVALID with their number in the message.  Bin i is masked if
 * it has fewer than min_nnz non-zero counted cells, or if its marginal over the cells shared
 * with unmasked bins is 0 (repeated to the fixed point); no bin left: BB_ERR_INVALID.  From
 * b = 1, x = 1 (0 at masked bins), it = 0:  s_i = x_i sum_j A_ij x_j over the live bins, mean =
 * sum s_i / n_live, var = sum (s_i / mean - 1)^2 / n_live; stop if var < tol or it == max_iter;
 * else b_i *= s_i / mean, x_i = 1 / b_i, ++it.  Then b *= sqrt(mean / target), target = row_sum,
 * or (row_sum <= 0) the mean of iteration 0, so that the counts keep their magnitude.  The loop
 * runs on the device, one sweep of the upper triangle per iteration (8 B per pair), a batch of
 * iterations per scalar read-back.
 * bias: n_bins doubles, NaN at masked bins (as Rao's KRnorm files mark them); masked: n_bins
 * bytes, 1 = masked; iterations (updates made) and variance (the last var) may be NULL. */
BB_API int bb_cm_balance(bb_cm *cm, int64_t n_bins, int64_t ignore_diags, int64_t min_nnz, double tol,
                         int64_t max_iter, double row_sum, double *bias, uint8_t *masked,
                         int64_t *iterations, double *variance);
/* The distance decay of the balanced map, per diagonal k = 0 .. n_bins - 1, in one sweep of the
 * upper triangle:  sums[k] = sum_i M[i][i+k] x_i x_{i+k} and counts[k] = #{i : x_i x_{i+k} != 0},
 * x = 1 / bias and 0 where the bias is NaN; bias == NULL: all ones.  A pair with x_i x_{i+k} == 0
 * is left out whatever its cell holds.  counts are exact; sums[k] / counts[k] is the expected
 * vector bb_cm_normalize takes. */
BB_API int bb_cm_expected(bb_cm *cm, int64_t n_bins, const double *bias, double *sums,
                          int64_t *counts);
/* Balancing without the dense matrix (docs/SPEC.md 2.5.3): the calls above on the matrix that
 * resident triples DEFINE -- what bb_cm_scatter_ex would build from them over n_bins + 1 bins:
 * nan_to_num of every value read, bin = (int)(pos / resolution), a triple names the unordered
 * pair of its bins, the LAST triple of a pair wins, a pair that touches bin n_bins is never read
 * -- which is never formed.  The first call for a given n_bins builds the canonical index of the
 * stored cells on the handle (a stable sort by cell and a keep-last compaction into a CSR of the
 * symmetric matrix: 12 B per directed entry resident, 64 B per triple plus the sort's counters
 * while it is built; bb_triples_destroy frees it); a later call with another n_bins rebuilds it.
 * A position that maps to a bin outside [0, n_bins]: BB_ERR_INVALID, as the scatter; device
 * memory that cannot be had: BB_ERR_NOMEM; either way nothing half-built stays on the handle.
 * Float64, no floating-point atomics, every sum in an order fixed by the index and n_bins alone:
 * the same bits on every run and for every duplicate-free triple list of the same matrix
 * (permuted, either orientation, row- or column-major).  One device: the handle's.
 *
 * bb_triples_balance: the arguments, the results and the refusals of bb_cm_balance.  One pass
 * over the index per iteration (12 B per directed entry).
 * bb_triples_expected: those of bb_cm_expected.  counts[k] is the number of pairs (i, i + k) of
 * bins with x_i != 0 and x_{i+k} != 0, with or without a triple; sums[k] runs over the stored
 * pairs, in a diagonal-major ordering of the index made by the first call.
 * bb_triples_pairs: the number of distinct stored pairs i <= j < n_bins. */
BB_API int bb_triples_balance(bb_triples *t, int64_t n_bins, int64_t ignore_diags, int64_t min_nnz,
                              double tol, int64_t max_iter, double row_sum, double *bias,
                              uint8_t *masked, int64_t *iterations, double *variance);
BB_API int bb_triples_expected(bb_triples *t, int64_t n_bins, const double *bias, double *sums,
                               int64_t *counts);
BB_API int bb_triples_pairs(bb_triples *t, int64_t n_bins, int64_t *n_pairs);
/* Shortest paths from a few sources over the graph resident triples define, without the dense
 * matrix (docs/SPEC.md 2.1.2) -- the geodesic rows of a landmark start (SPEC 2.5.4).
 * Nodes are 0 .. n_nodes - 1 (fit_triples' matrix size, n_bins + 1).  The calls use the handle's
 * canonical index for n_nodes (bb_triples_balance's rules: nan_to_num, the binning, the LAST
 * triple of a pair wins; built if it is not there; a later call with another size rebuilds it).
 * A position that maps to a bin outside [0, n_nodes): BB_ERR_INVALID, as
 * bb_solver_set_wish_triples refuses a bin outside its map (here a diagonal triple too).  There is
 * one undirected edge per stored off-diagonal cell; its weight is the wish distance of SPEC 2.1 in
 * float64, formed as bb_solver_set_wish_triples forms it before rounding to the run's dtype: the
 * value, divided by KRnorm[i] * KRnorm[j] * KRexpected[j - i] (i < j; n_nodes doubles each, both
 * or neither) and nan_to_num'ed if the vectors are given, then c^(-1/alpha) for BB_KIND_COUNTS or
 * the value itself for BB_KIND_WISH, then the float64 flush.  Anything that is not a finite
 * positive distance is no edge.  alpha <= 0 (either kind), an unknown kind: BB_ERR_INVALID.
 *
 * bb_triples_edge_degrees: deg[i] = the number of edges of node i, exact; n_nodes values.
 * bb_triples_paths: the lengths of the shortest paths from sources[a], a < n_sources, to every
 * node.  1 <= n_sources <= BB_PATHS_MAX_SOURCES; sources may repeat and come in any order; one
 * outside [0, n_nodes) is BB_ERR_INVALID.  Multi-source Bellman-Ford over the index: one launch
 * per sweep, a wave per segment of a row and 64 sources, a batch of sweeps per read of the
 * "changed" flags, the end at the first sweep that changes nothing and after n_nodes sweeps at
 * the latest.  Float64; the only atomic is an integer min on the bit pattern of a non-negative
 * double.  The distances are updated in place, and the fixed point of d[v] = min(d[v], fl(d[u] +
 * w)) is unique for positive weights: the results are, bit for bit and on every run, those of
 * Dijkstra's algorithm in float64 (scipy.sparse.csgraph.dijkstra); the NUMBER of sweeps depends
 * on the order the hardware runs the waves in and is NOT reproducible.  Device memory: 8 B x
 * n_nodes x (n_sources rounded up to 64), kept by the result, plus 8 B per directed entry of the
 * index during the call; the size is checked first, and what cannot be had is BB_ERR_NOMEM with
 * the sizes in the message, nothing half-built left on the handle (a complete index stays).
 * Nothing is allocated per sweep.
 * The result lives in a bb_paths, which owns its device memory and outlives the triples (the
 * lifetime rules of bb_sig); *out is NULL after an error.
 *   bb_paths_info     n_sources, n_nodes, sweeps (launches made, the confirming one included; 0
 *                     for a graph without stored cells), unreachable (the (source, node) pairs
 *                     without a path); each may be NULL
 *   bb_paths_read     dist (n_sources, n_nodes) float64 to the host, in SPEC 2.1.1's convention:
 *                     0 where no path exists ("no constraint") and on a source's own node
 *   bb_paths_read_columns  the same for the m nodes listed: out (n_sources, m); a node outside
 *                     [0, n_nodes) is BB_ERR_INVALID
 *   bb_paths_reached  reached[a] = the number of nodes source a has a path to, its own included;
 *                     n_sources values
 *   bb_paths_place    landmark placement on the device: for every node j with a path from EVERY
 *                     source that takes part, xyz[j][c] = -1/2 sum_a coef[a][c] (D[j][a]^2 -
 *                     mu[a]), a ascending, float64, placed[j] = 1; else placed[j] = 0 and xyz[j]
 *                     is left as it was.  A source whose coef row and mu are all 0 takes no part,
 *                     in the sum or in `placed` (a landmark that was dropped).
 *                     coef (n_sources, 3), mu n_sources, xyz (n_nodes, 3), placed n_nodes: host.
 *   bb_paths_timing   HIP-event times (ms) of the call: the weights, and all sweeps
 *   bb_paths_destroy  frees it (NULL is fine) */
#define BB_PATHS_MAX_SOURCES 1024
typedef struct bb_paths bb_paths;
BB_API int bb_triples_edge_degrees(bb_triples *t, int64_t n_nodes, int kind, double alpha,
                                   const double *KRnorm, const double *KRexpected, int64_t *deg);
BB_API int bb_triples_paths(bb_triples *t, int64_t n_nodes, int kind, double alpha,
                            const double *KRnorm, const double *KRexpected, const int64_t *sources,
                            int64_t n_sources, bb_paths **out);
BB_API int bb_paths_info(const bb_paths *p, int64_t *n_sources, int64_t *n_nodes, int64_t *sweeps,
                         int64_t *unreachable);
BB_API int bb_paths_reached(const bb_paths *p, int64_t *reached);
BB_API int bb_paths_read(const bb_paths *p, double *dist);
BB_API int bb_paths_read_columns(const bb_paths *p, const int64_t *nodes, int64_t m, double *out);
BB_API int bb_paths_place(const bb_paths *p, const double *coef, const double *mu, double *xyz,
                          uint8_t *placed);
BB_API int bb_paths_timing(const bb_paths *p, double *weights_ms, double *sweeps_ms);
BB_API int bb_paths_destroy(bb_paths *p);
/* Landmark constraints inside the fit (docs/SPEC.md 2.5.5): the kept rows of a bb_paths stay in
 * the solver as weighted wish distances between each landmark s_a and every node v,
 *     S(X) = S_q(X) + weight * sum_a sum_v D_av^-q (|x_{s_a} - x_v|_eps - D_av)^2,
 * q the solver's weight power (bb_solver_set_weight_power, also when set afterwards), eps the
 * floor of SPEC 2.2.  A term exists where D_av, rounded to the solver's dtype by the value rule of
 * every input route (finite, positive, inside the dtype's wish floor and ceiling), is > 0 and
 * v != s_a; each ordered (a, v) is a term of its own, and one that coincides with a stored pair
 * is added to it.
 *   bb_solver_set_anchors   the solver makes its OWN resident copy: row a of the paths for every
 *                           a with kept[a] != 0 (kept: n_sources bytes; NULL = all), converted on
 *                           the device, n_pad values per row in the solver's dtype (0 in the
 *                           padding and on the landmark's own node), and the kept sources' nodes;
 *                           the paths may be destroyed afterwards.  paths == NULL or weight == 0
 *                           clears the anchors.  The size is checked first: BB_ERR_NOMEM with the
 *                           sizes in the message; after any failure the solver is as it was.
 *                           BB_ERR_INVALID: a negative or non-finite weight, n_nodes != the
 *                           solver's bins, paths of another device, fewer than 1 kept row, two
 *                           kept rows of one node; BB_ERR_STATE: world > 1, a solver of several
 *                           maps (n_maps > 1; bb_solver_set_maps refuses while anchors are set),
 *                           a pending bb_solver_grad
 *   bb_solver_anchor_sums   per bin, weight * sum of D^-q over the terms that touch it (as node
 *                           and as landmark), float64, a fixed order: what joins the weighted
 *                           degrees of SPEC 2.4.1; zeros without anchors
 *   bb_solver_anchor_stress the second sum of S at the current coordinates, alone (0 without)
 *   bb_solver_anchor_info   kept rows, terms, bytes resident; each may be NULL
 * While anchors are set, bb_solver_iterate runs per iteration the sweep, the reduce into the
 * exchange buffer, three launches that add the terms there -- per node, a ascending over the
 * coalesced rows; per (landmark, chunk of 1,024 nodes) into own slots; one fold in chunk order,
 * the stress into hi / lo in double -- and the update of bb_solver_apply; maps of the one-launch
 * path (bb_solver_iteration_path) take this path too.  bb_solver_grad (world 1) adds the terms,
 * so bb_solver_read_exchange shows them; bb_solver_stress, the history and bb_solver_apply
 * report the total S (bb_solver_iterate_dist at world 1 and a bb_group of one member go through
 * the same buffer and add them too; bb_solver_iterate_peer, whose kernels step from the reduce
 * itself, is BB_ERR_STATE).  No floating-point atomics: the same bits on every run.  Without anchors
 * every path, launch and bit is what it was.  An anchored map needs a step per bin
 * (bb_solver_set_bin_steps from the sums above): a landmark touches about n_bins terms. */
BB_API int bb_solver_set_anchors(bb_solver *s, const bb_paths *paths, const uint8_t *kept,
                                 double weight);
BB_API int bb_solver_anchor_sums(bb_solver *s, double *sums, int64_t n_bins);
BB_API int bb_solver_anchor_stress(bb_solver *s, double *stress);
BB_API int bb_solver_anchor_info(const bb_solver *s, int64_t *kept_rows, int64_t *terms,
                                 int64_t *bytes);
/* Measurement aid: the average HIP-event time of the three anchor launches of one iteration,
 * back to back `launches` times at the current coordinates into the (zeroed) exchange buffer.
 * BB_ERR_STATE without anchors or while a bb_solver_grad is pending. */
BB_API int bb_solver_measure_anchors(bb_solver *s, int launches, double *ms_avg);
/* The Fit-Hi-C significance call on a resident map (docs/SPEC.md 2.9; reference:
 * blueberry/fithic.py:413-435, one text line at a time through scipy.special.bdtrc).
 *
 * bb_binomial_sf: out[i] = P(X >= k[i]), X ~ Binomial(n, p[i]), for m host values; n a whole
 * number in [0, 2^53].  Float64: Loader's saddle-point pmf at the first term, then the ratio
 * recurrence of the tail (upward above the mode, else the lower tail and 1 - sum), within 1.2e-13
 * of an 80-digit sum over the table on which scipy's bdtrc is off by up to 1.7e-3
 * (docs/MEASUREMENTS.md).  k <= 0: 1; k > n: 0; p outside
 * [0, 1]: NaN.  An element with 0 < p < 1 and n p > 1,048,576 -- the limit the sum's cap of terms
 * was derived for -- is BB_ERR_INVALID, nothing written; a sum that reaches the cap all the same
 * is BB_ERR_STATE, nothing written.
 *
 * bb_cm_significance: over the leading n_bins x n_bins block of the resident matrix (d must be
 * n_bins + 1; row and column n_bins are never read; the matrix stays as it is), the cells (i, j),
 * i <= j, k_lo <= j - i <= k_hi (0 <= k_lo <= k_hi < n_bins), are the counted cells.  One that is
 * negative, not finite or not a whole number: BB_ERR_INVALID "significance needs raw counts".
 * A counted cell is LISTED if its count is >= 1, bias_lo <= bias[i], bias[j] <= bias_hi (a NaN
 * bias fails; pass -inf / +inf for no bounds) and its prior pi = prior_by_distance[j - i] *
 * bias[i] * bias[j] lies in [0, 1]; bias and prior_by_distance hold n_bins doubles.  The result is
 * the list in canonical order -- row-major, i ascending, then j -- with p = P(Binomial(n_total,
 * pi) >= count) for every listed cell, made by a count, an exclusive scan and a write (no atomic
 * cursor): the same bits on every run.  A listed cell with pi < 1 and n_total * pi > 1,048,576:
 * BB_ERR_INVALID.  The matrix is read twice.
 * bb_triples_significance: the same on the matrix resident triples define (bb_triples_balance's
 * rules; the canonical index is built on the handle if it is not there, and stays): the same
 * list, bit for bit, as bb_cm_significance on the scattered matrix.  One chromosome: a list with
 * chromosome boundaries is out of scope.
 * The results live in a bb_sig, which owns its device memory; *out is NULL after an error.
 *   bb_sig_size    the number of listed cells; terms (may be NULL): pmf values summed over all
 *   bb_sig_read    row, col (int32), count, p (float64) to the host, bb_sig_size values each
 *   bb_sig_timing  HIP-event times (ms) of the call: count + scan + write, and the p-value pass
 *   bb_sig_destroy frees it (NULL is fine)
 *
 * The q-values of the list, on the device (docs/SPEC.md 2.9.7):
 *   bb_sig_q_values  q of the resident p-values with n_tests tests, kept on the handle: q[order] =
 *                  the Benjamini-Hochberg scan of p[order], order = the STABLE sorted order of p
 *                  (numpy's order of float64: NaN last, -0.0 equal to 0.0, ties in list order).
 *                  A 64-bit key per value, a stable radix sort of (key, place), a gather of the
 *                  original values, the scan of bb_benjamini_hochberg, a scatter: bit for bit what
 *                  that function gives on the host-sorted values, the same bits on every run.
 *                  Calling it again recomputes.  sort_ms / scan_ms (may be NULL): HIP-event times
 *                  of keys + sort, and of gather + scan + scatter.  Its buffers (40 B per cell
 *                  plus the sort's counters) are freed before it returns; one that cannot be
 *                  allocated is BB_ERR_NOMEM and leaves the handle without q.  A list of 2^32
 *                  cells or more is BB_ERR_INVALID.
 *   bb_sig_read_q  q (float64) to the host, bb_sig_size values; BB_ERR_STATE before
 *                  bb_sig_q_values.
 *   bb_sig_select  a NEW bb_sig of the cells with q <= q_max -- row, col, count, p and q -- in
 *                  canonical order (a flag, an exclusive scan, a write); a NaN q is never
 *                  selected.  NaN q_max: BB_ERR_INVALID; before bb_sig_q_values: BB_ERR_STATE;
 *                  *out is NULL after an error.  bb_sig_size (terms: 0), bb_sig_read,
 *                  bb_sig_read_q and bb_sig_destroy work on the result. */
typedef struct bb_sig bb_sig;
BB_API int bb_binomial_sf(const int64_t *k, double n, const double *p, double *out, int64_t m,
                          int device);
BB_API int bb_cm_significance(bb_cm *cm, int64_t n_bins, int64_t k_lo, int64_t k_hi,
                              const double *bias, double bias_lo, double bias_hi,
                              const double *prior_by_distance, double n_total, bb_sig **out);
BB_API int bb_triples_significance(bb_triples *t, int64_t n_bins, int64_t k_lo, int64_t k_hi,
                                   const double *bias, double bias_lo, double bias_hi,
                                   const double *prior_by_distance, double n_total, bb_sig **out);
BB_API int bb_sig_size(const bb_sig *s, int64_t *n_listed, int64_t *terms);
BB_API int bb_sig_read(const bb_sig *s, int32_t *row, int32_t *col, double *count, double *p);
BB_API int bb_sig_timing(const bb_sig *s, double *list_ms, double *p_ms);
BB_API int bb_sig_q_values(bb_sig *s, int64_t n_tests, double *sort_ms, double *scan_ms);
BB_API int bb_sig_read_q(const bb_sig *s, double *q);
BB_API int bb_sig_select(const bb_sig *s, double q_max, bb_sig **out);
BB_API int bb_sig_destroy(bb_sig *s);
/* Pooling a map to a coarser resolution (docs/SPEC.md 2.12).  Coarse bin I holds the fine bins
 * [I factor, min((I + 1) factor, n_bins)), nc = ceil(n_bins / factor); pooled cell (I, J), I < J,
 * is the sum of the block's fine cells, (I, I) the sum of the block's upper triangle with its
 * diagonal; BB_COARSEN_MEAN divides that sum once by the number of fine cells pooled (absent and
 * zero cells count).  Float64 in a FIXED order -- per fine row of the block, top to bottom, a
 * partial of its cells left to right; then the partials top to bottom; all from +0.0 -- so that
 * both routes give the same bits, on every run.  No atomics.  Values are added as stored: a NaN
 * or an infinity reaches its own pooled cell alone.  Any factor >= 1 works (beyond n_bins: one
 * bin).  factor < 1, an unknown `how`, n_bins < 0: BB_ERR_INVALID.
 *
 * bb_cm_coarsen: from the upper triangle of the leading n_bins x n_bins block of src (its edge
 * must be n_bins + 1: a filtered map is refused; the matrix is taken to be symmetric, as
 * bb_cm_symv takes it) into dst, another map of edge nc + 1 on the same device: the lower
 * triangle mirrors the upper bit for bit, the padding row and column are 0.  src is not changed.
 * bb_cm_coarsen_timing: the ms of the pooling kernel that wrote dst, by HIP events.
 *
 * bb_triples_coarsen: the same on the matrix resident triples define (bb_triples_balance's rules
 * and index), device to device: *out is a NEW handle on src's device, at resolution
 * src's x factor (which must fit 31 bits), of one triple [I R, J R, value] per pooled cell
 * I <= J that has at least one stored fine cell (a stored 0 included), I ascending, then J.
 * *out is NULL after an error; bb_triples_destroy frees it; it does not depend on src.
 * bb_triples_coarsen_timing: the ms of count + scan + write that made dst (the index apart).
 * bb_triples_size: the number of triples of a handle.  bb_triples_download: they, as (n, 3)
 * C-ordered rows, to the host -- the values as stored (nan_to_num is a reader's rule). */
enum { BB_COARSEN_SUM = 0, BB_COARSEN_MEAN = 1 };
BB_API int bb_cm_coarsen(const bb_cm *src, int64_t n_bins, int64_t factor, int how, bb_cm *dst);
BB_API int bb_cm_coarsen_timing(const bb_cm *dst, double *kernel_ms);
BB_API int bb_triples_coarsen(bb_triples *src, int64_t n_bins, int64_t factor, int how,
                              bb_triples **out);
BB_API int bb_triples_coarsen_timing(const bb_triples *dst, double *pool_ms);
BB_API int bb_triples_size(const bb_triples *t, int64_t *n);
BB_API int bb_triples_download(const bb_triples *t, double *triples);
/* The insulation sums of a map (docs/SPEC.md 2.13; Crane et al. 2015, cooltools' convention).
 * M is the leading n x n block (n = n_bins) of the resident (n_bins + 1)^2 matrix, or the matrix
 * resident triples define (bb_triples_balance's rules and index); symmetric, only a <= b is read.
 * window w >= 1 in bins; ignore_diags g >= 0; bias: n_bins host doubles, NULL = all ones.
 * x = 1 / bias, 0 where the bias is NaN; bin a is live iff x_a != 0; a cell is live iff both of
 * its bins are.  The diamond of bin i is the cells (a, b) with
 *   max(0, i - w + 1) <= a <= i <= b <= min(n - 1, i + w - 1)  and  b - a >= g
 * (bin i sits on both sides; w > n is legal: the diamond is clipped).
 * sums[i], float64 in a FIXED order: per row a of the diamond, top to bottom, a row partial of
 * M_ab (x_a x_b) over the row's live cells, left to right; then the partials top to bottom; every
 * accumulator from +0.0, so that a zero, dead or absent cell may be added as 0 or skipped (as in
 * bb_cm_coarsen).  The product and the sum are two roundings (no fma).  Both routes give the
 * same bits, on every run; no atomics.  Values are added as stored: a NaN or an infinity reaches
 * exactly the bins whose diamond holds its live cell.
 * counts[i]: the number of live cells of the diamond, zero and absent cells included -- for each
 * live row a the live bins of [max(i, a + g), min(n - 1, i + w - 1)], from a prefix count of the
 * live bins; one host rule for both routes.
 * window < 1, ignore_diags < 0, an edge that is not n_bins + 1 (a filtered map), a triple's bin
 * outside [0, n_bins]: BB_ERR_INVALID.  The map is not changed.
 * bb_cm_insulation_timing, bb_triples_insulation_timing: the ms of the kernel of the handle's
 * last call, by HIP events (the triples' index build apart). */
BB_API int bb_cm_insulation(bb_cm *cm, int64_t n_bins, int64_t window, int64_t ignore_diags,
                            const double *bias, double *sums, int64_t *counts);
BB_API int bb_cm_insulation_timing(const bb_cm *cm, double *kernel_ms);
BB_API int bb_triples_insulation(bb_triples *t, int64_t n_bins, int64_t window, int64_t ignore_diags,
                                 const double *bias, double *sums, int64_t *counts);
BB_API int bb_triples_insulation_timing(const bb_triples *t, double *kernel_ms);
/* Hand the resident matrix to a solver of n_bins = d bins on the same device, device
 * to device (same meaning of kind / alpha as bb_solver_set_wish_dense).  A solver on another
 * device packs over peer access where hipDeviceCanAccessPeer allows it (enabled here); without
 * it BB_ERR_INVALID "... on another device ...". */
BB_API int bb_solver_set_wish_from_cm(bb_solver *s, const bb_cm *cm, int kind, double alpha);
/* The same into the bins [bin_offset, bin_offset + d) of a solver of several maps
 * (bb_solver_set_maps), d = the map's edge. */
BB_API int bb_solver_set_wish_from_cm_block(bb_solver *s, const bb_cm *cm, int64_t bin_offset,
                                            int kind, double alpha);

/* The same two loops around a HOST matrix (round-1 entry points; upload, kernel,
 * download): */

/* matrix (d,d) float64 host, d = n_bins+1, zero-filled on entry.  `triples`
 * is the (n,3) array exactly as the reference's pointer arithmetic reads it:
 * column-major (pos_i[0..n), pos_j[0..n), count[0..n)).  bin = pos/resolution
 * truncated; later triples overwrite earlier ones. */
BB_API int bb_contactmap_scatter(const double *triples, int64_t n, int32_t resolution,
                                 double *matrix, int64_t d, int device);
/* In place on the host matrix: m[j][j+i] /= KRnorm[j]*KRnorm[j+i]*KRexp[i],
 * mirrored, then numpy.nan_to_num over the whole matrix.  bit-exact fp64. */
BB_API int bb_contactmap_normalize(double *matrix, int64_t n_bins, const double *KRnorm,
                                   const double *KRexpected, int device);

/* ---------------------------------------------------------------------- */
/* The remaining numeric Cython helpers of blueberry.pyx                    */
/* ---------------------------------------------------------------------- */

/* q[i] = max_{k<=i} min(p[k] * n / (k+1), 1) for d sorted p-values and n tests
 * (reference: blueberry/blueberry.pyx:40-75; a parallel prefix-max, exact). */
BB_API int bb_benjamini_hochberg(const double *p_values, int64_t d, int64_t n, double *q_values,
                                 int device);
/* The q-values of m host p-values in ANY order (docs/SPEC.md 2.9.7): q[order] =
 * bb_benjamini_hochberg(p[order], n_tests) with order the stable sorted order of p (numpy's order
 * of float64), bit for bit, sorted on the device.  order (may be NULL) receives that order.  m = 0
 * is fine; m >= 2^32 or a negative n_tests is BB_ERR_INVALID.  Host in, host out, on the
 * per-device stream and staging arena of bb_benjamini_hochberg. */
BB_API int bb_q_values(const double *p, int64_t m, int64_t n_tests, double *q, int64_t *order,
                       int device);
/* yp5i (n5,n5) float32, in place: yp5i[i][j] = max(yp5i[i][j], 5x5 block of yp1
 * (n1,n1)) for i, j < n5-1 (reference: blueberry/blueberry.pyx:93-104). */
BB_API int bb_downsample(const float *yp1, int64_t n1, float *yp5i, int64_t n5, int device);

/* ---------------------------------------------------------------------- */
/* Structure against structure (docs/SPEC.md 2.10)                          */
/* ---------------------------------------------------------------------- */

/* a, b: (n, 3) float64 host, 2 <= n < 2^31.  A bin is USED when use[i] != 0 (use = NULL: every
 * bin) and its six coordinates are finite; without used bins the means are NaN and every sum
 * is 0 (the Python wrapper refuses fewer than 2 before it calls).  Host in, host out, all arithmetic float64 on the device, every sum in an order fixed by n and the used
 * bins alone: two calls give the same bits.  No counterpart in the reference (it has no solver;
 * SURVEY.md 0).
 *   bb_structures_moments  what a superposition needs, over the used bins, in two passes (means,
 *                          then centred sums).  out18: the number of used bins, cA (3), cB (3),
 *                          EA = sum |A_i - cA|^2, EB = sum |B_i - cB|^2, and H row-major,
 *                          H[p][q] = sum (B_i - cB)_p (A_i - cA)_q.
 *   bb_structures_compare  transform13 = R row-major, t, s.  aligned (n, 3; may be NULL) =
 *                          s R B + t; bin_dev (n) = |A_i - aligned_i|^2 -- both NaN at unused
 *                          bins.  Over the pairs i < j of used bins, dA = |A_i - A_j| and dB =
 *                          |aligned_i - aligned_j|: profile (n, 7), row k = the pairs of
 *                          separation j - i = k: pairs, sum dA, sum dB, sum dA^2, sum dB^2,
 *                          sum dA dB, sum (dA - dB)^2; bins (n, 2), row i = the pairs that hold
 *                          bin i: pairs, sum (dA - dB)^2.  With BB_CMP_SPEARMAN in flags,
 *                          rank_sums (4; else may be NULL) = m, sum rA^2, sum rB^2, sum rA rB:
 *                          m the pairs, r the average rank of a pair's distance among its
 *                          structure's m, less (m + 1) / 2; the flag without rank_sums, or with
 *                          m >= 2^32, is BB_ERR_INVALID.  ms (5; may be NULL): HIP-event
 *                          milliseconds of the transform, the pair pass, its fold, the per-bin
 *                          pass and the ranks.  Device memory: under 1,200 B per bin + 0.5 MB,
 *                          and 40 B per pair with the flag; a failed allocation is BB_ERR_NOMEM
 *                          and the text names the bytes asked for. */
enum { BB_CMP_SPEARMAN = 1 };
BB_API int bb_structures_moments(const double *a, const double *b, const uint8_t *use, int64_t n,
                                 int device, double *out18);
BB_API int bb_structures_compare(const double *a, const double *b, const uint8_t *use, int64_t n,
                                 const double *transform13, int flags, int device, double *aligned,
                                 double *bin_dev, double *profile, double *bins, double *rank_sums,
                                 double *ms);

#ifdef __cplusplus
}
#endif
#endif /* BLUEBERRY_HIP_H */
