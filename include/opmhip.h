/* opmhip.h — C-ABI of libopmhip.so: the MI355X (gfx950) implementation of OPM Flow's per-Newton-iteration
 * hot path (black-oil AD assembly + ILU0/BiCGStab solve on 3x3 block-CSR).
 *
 * This header is the drop-in boundary.  Every entry point names the reference interface it replaces
 * (paths relative to the reference tree, opm-simulators 2021.10-pre).  Conventions:
 *   - plain C types only; all pointers are caller-owned HOST memory unless the name says "dev";
 *   - every function returns OPMHIP_SUCCESS (0) or a negative opmhip_status; nothing throws across the
 *     boundary (the reference turns a non-success SolverStatus into a Dune fallback,
 *     linalg/ISTLSolverEbos.hpp:277-297, so a C++ shim maps these codes back to bda::SolverStatus);
 *   - one context per GPU, single-threaded per context (the reference calls its backend from the one
 *     Newton-loop thread of a rank, linalg/bda/BdaBridge.cpp:192-255);
 *   - block size is 3, values are IEEE double, indices 32-bit int (bda/BdaSolver.hpp:86-88);
 *   - block-CSR layout exactly as BdaBridge hands it over (bda/BdaBridge.cpp:231-232): rows[Nb+1] block row
 *     pointers, cols[nnzb] block columns ascending inside a row, vals[nnzb*9] row-major 3x3 blocks.
 */
#ifndef OPMHIP_H
#define OPMHIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define OPMHIP_ABI_VERSION 11 /* 11: opmhip_get_iq_cells, opmhip_set_source_cells (the well model's traffic is its perforated cells, not the grid);
                               * 10: opmhip_config gained half_product (the product after an ILU0 application from the sweep's row sums), pin_host_arrays,
                               *     fused_reductions; opmhip_get_product_form, opmhip_preconditioned_product;
                               * 9: opmhip_wells gained `distributed` (standard wells whose perforations lie in several subdomains of a decomposed run);
                               * 8: opmhip_default_config: reorder = OPMHIP_REORDER_AUTO, cpr_amg_ilu_levels = -1 (the measured configuration);
                               *    opmhip_get_ordering_info, opmhip_wells gained the multisegment-well leg (num_ms_wells, ms_apply);
                               * 7: opmhip_config names cpr_amg_ilu_levels, cpr_gather_rows (were reserved[0..1]);
                               * 6: opmhip_set_hysteresis, opmhip_get_hysteresis, opmhip_set_hysteresis_params (additive); opmhip_config names
                               *    cpr_async_setup (was reserved[0]);
                               * 5: opmhip_set_water_compaction, opmhip_get_max_water_saturation, opmhip_relative_change, opmhip_cpr_recreate (additive);
                               * 4: opmhip_config names chain_length, spmv_pipe_wgs, preconditioner (were reserved[0..2]);
                               *    opmhip_set_endpoint_scaling, opmhip_sat_end_points, opmhip_sat_probe, opmhip_synchronize, opmhip_comm_info,
                               *    opmhip_set_composition_change_limits, opmhip_set_irreversible_compaction, opmhip_set_vappars, opmhip_begin_time_step;
                               * 3: opmhip_fluid gained pc_scaling, opmhip_set_pcw */

typedef struct opmhip_ctx opmhip_ctx;

typedef enum opmhip_status {
    OPMHIP_SUCCESS = 0,
    /* the three below mirror bda::SolverStatus (bda/BdaSolver.hpp:32-37) */
    OPMHIP_ANALYSIS_FAILED = -1,
    OPMHIP_CREATE_PRECONDITIONER_FAILED = -2,
    OPMHIP_UNKNOWN_ERROR = -3,
    OPMHIP_INVALID_ARGUMENT = -4, /* bad pointer/size, dim != 3 (bda/BdaBridge.cpp:207-211) */
    OPMHIP_NOT_READY = -5,        /* call order violated (e.g. solve before set_pattern) */
    OPMHIP_DEVICE_ERROR = -6,     /* a HIP call failed; text in opmhip_last_error */
    OPMHIP_NO_DEVICE = -7         /* no gfx950 device visible: the library never falls back to the CPU */
} opmhip_status;

/* --opencl-ilu-reorder (linalg/FlowLinearSolverParameters.hpp:317-321, bda/ILUReorder.hpp) */
typedef enum opmhip_reorder {
    OPMHIP_REORDER_LEVEL_SCHEDULING = 1, /* same factors as the CPU's natural-order ILU0 (bda/Reorder.cpp:266-318) */
    OPMHIP_REORDER_GRAPH_COLORING = 2,   /* Jones-Plassmann rounds, deterministic weights (bda/Reorder.cpp:59-172) */
    OPMHIP_REORDER_GRAPH_COLORING_GREEDY = 3, /* first-fit colouring: red-black on Cartesian 7-point grids */
    OPMHIP_REORDER_LINE_COLORING = 4, /* chains of <= config.chain_length (default 8) rows along each row's farthest
                                        neighbour (the vertical one in CpGrid's natural order), chains coloured greedily:
                                        an exact ILU0 of that ordering, near the natural order's strength at colouring's
                                        parallelism (no counterpart in the reference) */
    OPMHIP_REORDER_AUTO = 5,         /* line colouring where it pays - a structured grid in its natural order of at least 30 000 rows,
                                        chains of 4 below 200 000 rows, of 8 below 700 000, of 10 above (chain_length = 0; a non-zero
                                        chain_length is taken as given) - and the greedy colouring elsewhere: the chain sweeps walk their
                                        steps one after the other, which a small or irregular system cannot hide (a 44 777-cell
                                        corner-point grid: 31 Newton its/s with chains of 10, 259 greedy).  ABI 7.  With
                                        opmhip_set_ilu_fillin_level n >= 1: see there */
    OPMHIP_REORDER_DISTANCE2_COLORING = 6 /* first-fit colouring of the graph of A^2 (no two rows of one colour share a neighbour):
                                        the colours stay independent under level-1 fill, so ILU(1) sweeps one launch per colour
                                        (13 on a 7-point grid); for ILU0 one more colouring */
} opmhip_reorder;

/* --linear-solver-configuration (linalg/setupPropertyTree.cpp:62-76).  The CPR variants: pressure system solved by one AMG
 * V-cycle, ILU0 (relaxation 1) post-smoothing (setupPropertyTree.cpp:94-138); see csrc/cpr.hip for what of it is the
 * reference's and what is not */
typedef enum opmhip_preconditioner {
    OPMHIP_PRECOND_ILU0 = 0,           /* "ilu0" */
    OPMHIP_PRECOND_CPR_QUASIIMPES = 1, /* "cpr_quasiimpes": weights from the diagonal blocks (getQuasiImpesWeights.hpp:46-85) */
    OPMHIP_PRECOND_CPR_TRUEIMPES = 2   /* "cpr" = "cpr_trueimpes" (the reference's default CPR): weights from the storage term
                                          of the state on the device (contexts that assemble) or handed in with
                                          opmhip_set_cpr_weights (getQuasiImpesWeights.hpp:89-128) */
} opmhip_preconditioner;

/* how the ILU relaxation factor w enters M^-1 */
typedef enum opmhip_relax_mode {
    OPMHIP_RELAX_POST_SCALE = 0, /* v = w * U^-1 L^-1 d : the CPU path, linalg/ParallelOverlappingILU0.hpp:848-903 */
    OPMHIP_RELAX_IN_SWEEP = 1    /* x_i = w * D_i^-1 (y_i - sum U_ij x_j) : bda/openclKernels.cpp:301-383 */
} opmhip_relax_mode;

/* Solver configuration.  Defaults (opmhip_default_config) are Flow's: tol 1e-2, maxit 200, w 0.9
 * (linalg/FlowLinearSolverParameters.hpp:142-154) - and, where Flow has no say because the choice is this library's (the ILU ordering of the
 * accelerator path, the pressure AMG's smoother), the configuration bench.py measures.  ctor arguments of bda::BdaSolver (bda/BdaSolver.hpp:79). */
typedef struct opmhip_config {
    int abi_version;       /* OPMHIP_ABI_VERSION */
    int device_id;         /* --bda-device-id */
    int verbosity;         /* linear_solver_verbosity */
    int maxit;             /* --linear-solver-max-iter */
    double tolerance;      /* --linear-solver-reduction */
    double ilu_relaxation; /* --ilu-relaxation */
    int relax_mode;        /* opmhip_relax_mode */
    int reorder;           /* opmhip_reorder (opmhip_default_config: OPMHIP_REORDER_AUTO since ABI 8; opmhip_get_ordering_info says what it became) */
    int zero_diag_fix;     /* 1: exact 0.0 on a diagonal block's diagonal -> 1e-15 (bda/BdaBridge.cpp:125-161) */
    int chain_length;      /* OPMHIP_REORDER_LINE_COLORING: rows per chain (0 = 8) */
    int spmv_pipe_wgs;     /* pipelined SpMV: resident workgroups it is sized for (0 = 2048, the MI355X default; < 0 = one
                            * tile per workgroup instead); tuning only, results are the same bits either way */
    int preconditioner;    /* opmhip_preconditioner: --linear-solver-configuration */
    int cpr_reuse_setup;   /* --cpr-reuse-setup (linalg/FlowLinearSolverParameters.hpp:315, ISTLSolverEbos.hpp:401-426): when the
                            * STRUCTURE of the CPR hierarchy (aggregates, coarse patterns) is built anew from the matrix in hand:
                            * 0 for every linear solve, 1 at the first Newton iteration of every time step (contexts that
                            * assemble; others: never), 2 when the last solve took more than 10 iterations, 3 never after the
                            * first (Flow's default, and opmhip_default_config's).  The VALUES always follow the matrix. */
    int cpr_async_setup;   /* 1: with cpr_reuse_setup = 2 the new structure is built on a host thread BESIDE the solves and swapped in at
                            * the first solve boundary after it is ready (the solves in between keep the old one; one build at a time);
                            * which solve that is depends on the host's speed, so iteration counts are no longer reproducible run to
                            * run.  0 (default): the reference's rule to the letter - the solve that finds the rule met waits for the
                            * rebuild (0.28 s of host work at 10^6 cells).  (was reserved[0] until ABI 6) */
    int cpr_amg_ilu_levels; /* the pressure AMG's smoother: this many of its finest levels smooth with a scalar ILU0, relaxation 1 - the
                            * reference's AMG smoother (linalg/PreconditionerFactory.hpp:126-151, setupPropertyTree.cpp:116-137) - the others
                            * with damped Jacobi.  Level 0 eliminates in the ordering of the block ILU0 (opmhip_reorder), the levels below
                            * colour by colour of a greedy multi-colouring.  0: Jacobi on every level.  < 0 (opmhip_default_config's -1 since ABI 8): the library's choice -
                            * level 0 where the block ILU0's ordering has at most three colours (level 0's sweeps are one launch per colour),
                            * Jacobi otherwise.  (was reserved[0] until ABI 7) */
    int cpr_gather_rows;   /* decomposed runs (opmhip_comm_init_*): the pressure stage of the CPR spans the ranks, as the reference's does (Dune's
                            * parallel AMG behind linalg/OwningTwoLevelPreconditioner.hpp, PressureTransferPolicy.hpp:92-160).  Level 0 smooths
                            * with the pressure operator of the WHOLE system (ghost entries of the iterates exchanged: one double per boundary
                            * cell), its residual is summed over the aggregates down to the rank's first level of at most this many rows,
                            * those levels - their own entries plus the Galerkin sums of the couplings between aggregates of different
                            * subdomains - are joined into one system that every rank holds, coarsens further and cycles on (one all-gather
                            * of a right-hand side per application, one of matrix values per solve), and the post-smoothing residual
                            * d - A (0, x_p, 0) is the whole system's.  Aggregates never cross a rank boundary.  0: the default - over the loopback communicator ON with 100 000 rows (on a 10^6-cell subdomain its third level, aggregates of ~15 cells), over
                            * RCCL OFF until a multi-GPU run has covered its collectives (no round has had more than one GPU; ask for it with a positive value);
                            * < 0: off - one hierarchy per subdomain, no communication inside the preconditioner, iteration counts that
                            * grow with the number of ranks.  Ignored on a single rank; cpr_amg_ilu_levels and cpr_async_setup are ignored
                            * where it is in force.  (was reserved[1] until ABI 7) */
    int half_product;      /* ILU0-BiCGStab: the product that follows an M^-1 application is formed from the backward sweep's row sums.  On a
                            * pattern without triangles (every TPFA grid without well cliques or NNC triangles) no elimination step of the block
                            * ILU0 touches an entry right of the diagonal (linalg/ParallelOverlappingILU0.hpp:466-481 modifies A_ik only where
                            * (i,j), (j,k) and (i,k) all exist), so U == upper(A) bit for bit and u_i = sum_{j>i} U_ij z_j, which the backward
                            * sweep of z = U^-1 y forms anyway (:881-895), IS the upper part of (A z)_i.  The sweep stores u (24 bytes per row)
                            * and the product streams the matrix without its U part: y_i = (sum over lower entries, diagonal and ghost columns,
                            * ascending, of A_ik (w z_k)) + w u_i - 0.8 GB per preconditioned product instead of 1.0 (bda/cusparseSolverBackend.cu:
                            * 103-118 runs the sweep and then bsrmv over the whole matrix on the same vector).  Same products as the reference's
                            * A (w z), summed in another order: results differ from the plain form in the last bits, iteration counts
                            * agree (tests/test_gpu_half_product.py; the oracle states the same order).  0 (default): the library's choice - on
                            * where the pattern allows it, the ordering is line-coloured and the system is large enough for the pipelined
                            * kernels; > 0: wherever the pattern and the ordering allow it; < 0: never.  Ignored with a CPR preconditioner.
                            * Subdomains of a decomposed run: the tiles none of whose rows has a ghost column take the form (68 % of them on a
                            * 10^6-cell subdomain of a 2 x 2 x 2 decomposition), the boundary tiles keep the whole product - behind the halo
                            * exchange, as before; a subdomain without such tiles keeps the plain form.  opmhip_get_product_form says what
                            * is in force.  ABI 10 */
    int pin_host_arrays;   /* 1: the host arrays handed to opmhip_solve_system (vals, b) and opmhip_get_result (x) are registered with the
                            * driver (hipHostRegister) the first time each address is seen, so that every later copy is a DMA at the link's
                            * rate instead of a staged copy out of pageable memory (500 MB of values at 10^6 cells: 13.5 ms -> the PCIe
                            * figure).  For callers whose arrays keep their addresses for the life of the context - Flow's do:
                            * the matrix and the vectors are allocated once (bda/BdaBridge.cpp:199-232, linalg/ISTLSolverEbos.hpp:216-219),
                            * which is what the reference's CUDA back-end relies on when it copies from them every solve
                            * (bda/cusparseSolverBackend.cu:314-338); host/hipSolverBackend.hpp sets it.  The ranges are unregistered by
                            * opmhip_destroy; a refused registration falls back to the plain copy.  0 (default): plain copies - arrays that
                            * come and go (numpy temporaries) must not be pinned behind their owner's back.  ABI 10 */
    int fused_reductions;  /* 1: BiCGStab with ONE reduction per half iteration instead of two.  The reference forms alpha, |r|, omega, |r| and
                            * rho from five scalar products in four reductions per iteration (bda/cusparseSolverBackend.cu:92, 120-127, 151-161;
                            * in parallel runs each is an all-reduce, flow/BlackoilModelEbos.hpp:599-603 for the convergence sums alike).  Here
                            * the product's kernel leaves three sums - v.rw, v.v, v.r in the first half, t.r, t.t, t.rw in the second - and
                            *   |r - alpha v|^2 = r.r - 2 alpha v.r + alpha^2 v.v,   |r - omega t|^2 = r.r - 2 omega t.r + omega^2 t.t,
                            *   rho' = (rho - alpha v.rw) - omega t.rw
                            * give the norms and rho without a second pass: two reductions (of three doubles) and two scalar kernels per
                            * iteration instead of four, update kernels without partial sums.  The stopping rule then looks at RECURRED norms;
                            * the residual vector itself is still updated explicitly, its true norm is formed once at the end of the solve and
                            * reported in opmhip_result.reduction, and a solve whose true norm exceeds twice the tolerance although the recurred
                            * one met it comes back with converged = 0.  Same mathematics, other rounding: iteration counts may differ by a half
                            * step from the default form's; the oracle states the same arithmetic (oracle/linalg.hpp: bicgstab_fused_reductions).
                            * The recurred |r|^2 carries an absolute error of eps |r_0|^2, i.e. the norm a floor of 1.5e-8 |r_0|: opmhip_create refuses
                            * the mode with tolerance < 1e-6 (Flow's default is 1e-2).
                            * 0 (default): the reference's recurrence to the letter.  Meant for runs over many GPUs, where a half iteration's
                            * time is its all-reduces; measured on one GPU in DESIGN.md section 7.  ABI 10 */
} opmhip_config;

/* bda::BdaResult (bda/BdaResult.hpp:28-40) plus the reference's per-phase timers. */
typedef struct opmhip_result {
    int iterations;    /* min(it, maxit), it counted in half steps (bda/cusparseSolverBackend.cu:172) */
    int converged;     /* it != maxit + 0.5 (:176) */
    double reduction;  /* |r| / |r0| */
    double conv_rate;  /* reduction^(1/it) */
    double elapsed;    /* seconds in the whole call */
    double it;         /* raw half-iteration counter */
    double t_copy;     /* H2D of values/rhs (0 when the system is already device resident) */
    double t_factor;   /* ILU0 factorisation   = linear_solve_setup_time (timestepping/SimulatorReport.hpp:29-49) */
    double t_solve;    /* BiCGStab loop        = linear_solve_time */
    int num_colors;    /* colours / levels of the ILU ordering */
    int reserved[3];
} opmhip_result;

/* Standard-well contributions, the data bda::WellContributions carries across the boundary
 * (bda/WellContributions.hpp:60-214; fill order C, D, B per well, wells/StandardWellEval.cpp:1206-1250):
 * applied after each SpMV as y -= C^T (D^-1 (B x)) (bda/WellContributions.cu:36-126). dim = 3, dim_wells = 4.
 * One workgroup per well; where two wells perforate the same cell their updates of that cell are atomic adds (the
 * reference's kernel races there), so the result is then defined up to the order of two additions.
 *
 * Multisegment wells (ABI 8): the reference's WellContributions counts them in getNumWells() (bda/WellContributions.hpp:164-166) but
 * keeps their data in MultisegmentWellContribution objects whose D^-1 is a sparse LU on the HOST (UMFPack,
 * bda/MultisegmentWellContribution.cpp:35-62); its back-ends apply them through a host round trip after every product, in front of
 * the standard wells in the CUDA back-end (bda/WellContributions.cu:160-187), behind them in the OpenCL one (WellContributions.cpp:116-150).  The same here, in the CUDA back-end's order: with num_ms_wells > 0 the
 * library brings x and y (N doubles each, NATURAL order - the caller's objects know nothing of the ILU ordering, so there is no
 * setReordering to do) to pinned host memory after every product, calls ms_apply(ms_user, h_x, h_y) - which performs
 * y -= C^T (D^-1 (B x)) for every multisegment well, e.g. by looping MultisegmentWellContribution::apply(h_x, h_y) - and takes
 * h_y back.  num_wells counts the STANDARD wells only.  The callback runs on the calling thread, inside opmhip_solve_system.
 * That round trip is the reference's shape and the default here; it drains the stream twice per product.  The alternative is the
 * device-resident form of the same operator, opmhip_set_ms_wells below: the wells' arrays are handed over once, D is inverted on the
 * device and every product applies the wells in one kernel, with no host in the loop.  A solve takes one form or the other, never both.
 *
 * Decomposed runs (ABI 9).  Cell indices are the rank's local ones and must be OWNED cells (< Nb).  By default Flow's partitioner keeps
 * every well inside one subdomain (--allow-distributed-wells=false, ebos/eclbasevanguard.hh:148-151): distributed = 0, each rank hands
 * over its own wells, nothing is exchanged.  With distributed wells the reference sums B x over the ranks that share the well
 * (wellhelpers::ParallelStandardWellB::mv, wells/WellHelpers.hpp:68-123, called from StandardWell::apply, wells/StandardWell_impl.hpp:
 * 1254-1280) and has D and the well residual summed at assembly (sumDistributedWellEntries, StandardWell_impl.hpp:260-261), so that D^-1
 * and C^T are applied rank by rank without further exchange.  The same here with distributed = 1: EVERY rank hands over the SAME list
 * of wells in the same order - its own perforations of each (none: val_pointers[w] == val_pointers[w + 1]) and the complete D^-1 - and
 * the num_wells x 4 partial products travel through one all-reduce per operator application (all ranks, not a sub-communicator per
 * well: ranks without perforations add zeros).  Every call that takes such a list is then COLLECTIVE (all ranks, same order); a
 * different num_wells on some rank - including 0: an empty list with distributed = 1 still takes part in the comparison - is reported on
 * every rank (INVALID_ARGUMENT) instead of hanging in the reduction, and so is a rank-local failure to take the list (a null array, a
 * perforation outside the owned cells, an allocation): the local checks run first, their outcome travels in the same reduction and every
 * rank leaves with an error.  A rank that passes NULL or distributed = 0 where the others pass a shared list cannot be caught.
 * opmhip_wells_recover_solution forms resWell - sum_ranks(B x) as the reference's mmv does for a shared well (WellHelpers.hpp:126-142). */
typedef void (*opmhip_ms_apply_fn)(void* user, const double* h_x, double* h_y);
typedef struct opmhip_wells {
    int num_wells;           /* standard wells (num_std_wells of the reference, NOT getNumWells()) */
    const int* val_pointers; /* [num_wells+1] perforation ranges */
    const int* Ccols;        /* [nperf] cell (block row) of each perforation */
    const int* Bcols;        /* [nperf] */
    const double* Cnnzs;     /* [nperf*12] 4x3 row-major */
    const double* Dnnzs;     /* [num_wells*16] 4x4 row-major, already inverted (D^-1) */
    const double* Bnnzs;     /* [nperf*12] */
    int num_ms_wells;        /* multisegment wells behind ms_apply (0: none) */
    opmhip_ms_apply_fn ms_apply; /* must be non-NULL when num_ms_wells > 0 */
    void* ms_user;           /* handed back to ms_apply */
    int distributed;         /* decomposed runs only (ignored on one rank); see above.  0: every well of the list lies inside this rank's
                              * subdomain; 1: the same list of wells on every rank, each rank with the perforations in ITS cells */
} opmhip_wells;

/* Multisegment wells, device-resident form (additive to ABI 11).  The constructor arguments of Opm::MultisegmentWellContribution
 * (bda/MultisegmentWellContribution.hpp:95-117), concatenated over the wells; dim = 3, dim_wells = 4.  Well w has Mb = Mb_pointers[w + 1] -
 * Mb_pointers[w] segments, M = 4 Mb scalar well equations and the blocks block_pointers[w] .. block_pointers[w + 1] - 1.
 *   B and C share one blocked-CSR pattern (one 4 x 3 block per perforation): Brows holds, well after well, Mb + 1 block-row pointers RELATIVE
 *   to the well's first block (so each well's part starts with 0; well w's part starts at Brows[Mb_pointers[w] + w]); Bcols the cell of
 *   each block (natural order); the values are indexed as the reference's apply indexes them: Bvals[blk * 12 + j * 3 + k],
 *   Cvals[blk * 12 + j + k * 3] (j the well equation in B, the cell equation in C).
 *   D (M x M) in scalar CSC as UMFPack takes it: Dcol_pointers holds, well after well, M + 1 column pointers relative to the well's first
 *   entry (well w's part starts at Dcol_pointers[4 * Mb_pointers[w] + w]); Drows / Dvals the entries, well w's from Dnnz_pointers[w] on.
 *   Entries that name the same place are added up.
 * opmhip_set_ms_wells takes the list over for EVERY operator application that follows - opmhip_solve_system with ILU0 / ILU(n) / CPR,
 * opmhip_spmv, opmhip_preconditioned_product - until it is replaced or cleared (ms == NULL or num_ms_wells == 0).  It is independent of
 * the per-solve opmhip_wells list (standard wells), which every call that takes one sets anew; the multisegment wells are applied in front
 * of the standard wells, as in the CUDA back-end.  Flow rebuilds its wells for every solve over a fixed pattern: an array that arrives
 * unchanged is not copied again, and D is inverted again only when Dvals (or the structure) changed.
 * What the device does: per change of values one workgroup per well scatters D into a dense M x M array, eliminates it with PARTIAL
 * PIVOTING (row exchanges over the whole column - D mixes flow and pressure rows of very different scale) and leaves the explicit D^-1
 * (Gauss-Jordan), so that a product costs one dense matrix-vector product instead of M dependent substitution steps.  Per product one
 * workgroup per well forms z1 = B (xs x) in the statement order of MultisegmentWellContribution.cpp:78-90, z2 = D^-1 z1, and
 * y[cell] -= C^T z2 in the order of :97-108.  Where no cell is shared between two blocks of the list the updates of y are plain stores;
 * otherwise they are atomic adds and the result is then defined up to the order of two additions (as for standard wells).
 * Accuracy: that of an explicit inverse - a forward error of the order M eps cond(D) |z2|, NOT the componentwise bound of a pivoted solve;
 * for a badly row-scaled D the two differ (numpy's inv(D) @ z shows the same).
 * Size caps: a well may have at most OPMHIP_MS_WELLS_MAX_M scalar equations (its z1, z2 live in LDS, its dense D^-1 takes 8 M^2 bytes and
 * the elimination is M^3 work for one workgroup) and the list's dense arrays at most OPMHIP_MS_WELLS_MAX_KIB KiB in all.  A list above
 * either cap is refused (INVALID_ARGUMENT) and leaves no list set, so that the caller can fall back to the callback form.
 * Refused with a text that names the reason: before the pattern is set (NOT_READY); INVALID_ARGUMENT for dim / dim_wells other than 3 / 4,
 * a null array, inconsistent pointers, a cell outside [0, Nb), a well above the caps, a decomposed context (nranks > 1), and a SINGULAR D:
 * a zero pivot is flagged on the device and reported by the next call that synchronises anyway - opmhip_solve_system, opmhip_spmv,
 * opmhip_preconditioned_product, opmhip_get_ms_wells_info - which returns INVALID_ARGUMENT and clears the list; never a silent NaN.
 * A solve that is handed opmhip_wells.num_ms_wells > 0 with a callback WHILE a device list is set is refused (INVALID_ARGUMENT): the
 * operator would be applied twice.
 * The TREE form (opmhip_set_ms_wells_form below) is the second, opt-in form of the same list, for wells of any length up to
 * OPMHIP_MS_WELLS_TREE_MAX_SEGMENTS.  D of a multisegment well is block-sparse over the segment tree - 4 x 4 blocks on the diagonal and
 * between a segment and its outlet - and eliminating the leaves first produces no fill: per segment i with parent p and children c,
 *     S_i = D_ii - sum_c E_c D_ci,   E_i = D_pi S_i^-1,
 * 48 doubles per segment (S_i^-1, E_i, D_ip) instead of 8 M^2 bytes, work linear in the segments.  Per product z2 = D^-1 z1 is a sweep
 * from the leaves to the roots (z_p -= E_c z_c) and one back (x_i = S_i^-1 (z_i - D_ip x_p)): 2 x depth dependent steps for one
 * workgroup (z, the tree's index lists and - where they fit - the well's blocks are in LDS for them).  Every sum is taken in a stated order (children ascending); opm-autodiff_amd/mswells.py tree_solve is the arithmetic in numpy.
 * Accuracy of the tree form: that of a BLOCK elimination WITHOUT pivoting across blocks.  Rows are exchanged inside a segment's 4 x 4
 * block only, so the form relies on every S_i being well conditioned against the blocks beside it, which holds for the well equations
 * (each segment's own unknowns dominate its equations) but not for an arbitrary non-singular D: a D whose diagonal block is singular
 * while D is not is REFUSED by the tree form (INVALID_ARGUMENT at the next synchronisation, naming well and segment; the list is
 * cleared) where the dense form, which pivots over the whole column, solves it.
 * The block pattern must be a forest over the segments (segments i != j are neighbours if an entry of D lies in block (i, j) or (j, i)); a
 * pattern with a cycle is refused naming the well and the two segments of an edge that closes it. */
#define OPMHIP_MS_WELLS_MAX_M 256      /* 64 segments */
#define OPMHIP_MS_WELLS_MAX_KIB 32768  /* 32 MiB of dense D^-1 over the list: 64 wells of the largest size */
#define OPMHIP_MS_WELLS_TREE_MAX_SEGMENTS 1024  /* tree form: the well's z of 4096 doubles (32 KiB) stays in LDS */
#define OPMHIP_MS_WELLS_DENSE 0
#define OPMHIP_MS_WELLS_TREE 1
#define OPMHIP_MS_WELLS_AUTO 2
typedef struct opmhip_ms_wells {
    int num_ms_wells;
    int dim, dim_wells;          /* 3, 4 */
    const int* Mb_pointers;      /* [num_ms_wells+1] segment ranges */
    const int* Brows;            /* [Mb_pointers[n] + n] per well Mb+1 block-row pointers, relative to the well's first block */
    const int* block_pointers;   /* [num_ms_wells+1] block ranges */
    const int* Bcols;            /* [nblocks] cell of each block */
    const double* Bvals;         /* [nblocks*12] */
    const double* Cvals;         /* [nblocks*12] */
    const int* Dcol_pointers;    /* [4*Mb_pointers[n] + n] per well 4 Mb + 1 column pointers, relative to the well's first entry */
    const int* Drows;            /* [Dnnz] scalar row inside the well */
    const double* Dvals;         /* [Dnnz] */
    const int* Dnnz_pointers;    /* [num_ms_wells+1] entry ranges */
} opmhip_ms_wells;
int opmhip_set_ms_wells(opmhip_ctx* ctx, const opmhip_ms_wells* ms);
/* info[0] wells held on the device, info[1] the largest M = 4 Mb among them, info[2] device memory held for them in KiB (rounded up),
 * info[3] inversions of the list done so far on this context (unchanged values are not factored again).  Reports a pending singular D. */
int opmhip_get_ms_wells_info(opmhip_ctx* ctx, int info[4]);
/* replaces: the sparse LU of D on the host, umfpack_di_symbolic / _numeric / _solve (bda/MultisegmentWellContribution.cpp:56-57, :93).
 * The form of the lists set AFTER this call (additive to ABI 11): OPMHIP_MS_WELLS_DENSE (the default: everything above, caps and texts
 * included), OPMHIP_MS_WELLS_TREE (every well of the list in the tree form; a well whose block pattern is not a tree, or that has more
 * than OPMHIP_MS_WELLS_TREE_MAX_SEGMENTS segments, is refused and no list stays set) or OPMHIP_MS_WELLS_AUTO (per well: within both
 * dense caps dense; above OPMHIP_MS_WELLS_MAX_M tree if its pattern is a tree and it is within the tree cap; otherwise the list is
 * refused with the dense cap's message).  One list may so hold both forms; OPMHIP_MS_WELLS_MAX_KIB counts the dense wells only.  A list
 * already set is cleared when the form CHANGES.  Any other value: INVALID_ARGUMENT. */
int opmhip_set_ms_wells_form(opmhip_ctx* ctx, int form);
/* replaces: nothing in the reference (UMFPack's own report, umfpack_di_report_info, is the nearest).
 * info[0] the form set, info[1] wells of the list in dense form, info[2] wells in tree form, info[3] the largest tree well's segments,
 * info[4] the largest tree depth in levels, info[5] KiB held for the tree wells' blocks (rounded up).  Reports a pending singular D. */
int opmhip_get_ms_wells_form_info(opmhip_ctx* ctx, int info[6]);

/* ---- lifetime ------------------------------------------------------------------------------------------ */
void opmhip_default_config(opmhip_config* cfg);
/* replaces: BdaBridge ctor selecting a backend by string (bda/BdaBridge.cpp:55-121) */
int opmhip_create(const opmhip_config* cfg, opmhip_ctx** out);
void opmhip_destroy(opmhip_ctx* ctx);
/* last error text of this context (or of the failed create when ctx == NULL); never NULL */
const char* opmhip_last_error(const opmhip_ctx* ctx);
int opmhip_abi_version(void);
/* waits until everything this context has enqueued on its stream is done (callers that time a region from outside) */
int opmhip_synchronize(opmhip_ctx* ctx);

/* ---- linear solve (drop-in for bda::BdaSolver<3>) --------------------------------------------------- */
/* replaces: first-call branch of solve_system -> initialize + analyse_matrix
 * (bda/cusparseSolverBackend.cu:187-260, 348-422; bda/BILU0.cpp:51-158).  The pattern is fixed for the life of
 * the context (linalg/ISTLSolverEbos.hpp:216-219).  Computes the ILU ordering, the device tiling and uploads
 * the index arrays. */
int opmhip_set_pattern(opmhip_ctx* ctx, int Nb, int nnzb, const int* rows, const int* cols);
/* Domain-decomposed variant (one context per GPU, one subdomain per context): the matrix has Nb owned block rows; columns
 * may also reference Nghost ghost cells numbered Nb .. Nb+Nghost-1 - the owner-cells-first local ordering the reference
 * requires of parallel runs (linalg/ISTLSolverEbos.hpp:171-178).  Ghost columns take part in the operator (SpMV) and in
 * the assembly; the ILU0 is block-Jacobi per subdomain and ignores them, like detail::ghost_last_bilu0_decomposition
 * (linalg/ParallelOverlappingILU0.hpp:439-494, loop bounds :857-860).  Per-cell state/static arrays then have
 * Nb+Nghost entries, solver vectors (rhs, x, residual) Nb. */
int opmhip_set_pattern_dd(opmhip_ctx* ctx, int Nb, int Nghost, int nnzb, const int* rows, const int* cols);

/* replaces: bda::BdaSolver<3>::solve_system(N, nnz, dim, vals, rows, cols, b, wellContribs, res)
 * (bda/BdaSolver.hpp:86-88).  N = 3*Nb scalar rows, nnz = 9*nnzb scalars, dim = 3.  If the pattern was not set
 * yet this call sets it from rows/cols (the reference's "initialized == false" path); afterwards rows/cols may
 * be NULL.  vals == NULL and b == NULL mean "use the Jacobian and residual the context assembled on the
 * device".  vals may be modified when zero_diag_fix is on, as the reference does (bda/BdaBridge.hpp:68).
 * wells may be NULL.  A non-converged solve is NOT an error: it returns OPMHIP_SUCCESS with res->converged = 0
 * (the caller then falls back, linalg/ISTLSolverEbos.hpp:277-289). */
int opmhip_solve_system(opmhip_ctx* ctx, int N, int nnz, int dim, double* vals, const int* rows, const int* cols,
                        const double* b, const opmhip_wells* wells, opmhip_result* res);

/* replaces: bda::BdaSolver<3>::get_result(x) (bda/BdaSolver.hpp:90): N doubles to caller memory, natural order */
int opmhip_get_result(opmhip_ctx* ctx, double* x);

/* The two other places where the standard wells' Schur complement touches reservoir vectors, for runs that keep
 * residual and solution on the device.  res_well: num_wells x 4 well residuals (host).
 * replaces: BlackoilWellModel::apply(r) -> StandardWell::apply(BVector& r): r -= C^T (D^-1 resWell)
 *   (wells/BlackoilWellModel_impl.hpp:1031-1042, wells/StandardWell_impl.hpp:1283-1296), applied to the residual the
 *   last opmhip_assemble left on the device (before opmhip_solve_system); */
int opmhip_wells_apply_residual(opmhip_ctx* ctx, const opmhip_wells* wells, const double* res_well);
/* replaces: BlackoilWellModel::addWellContributions(mat) -> StandardWell::addWellContributions
 *   (wells/StandardWell_impl.hpp:1688-1712), the --matrix-add-well-contributions=true mode: A -= C^T D^-1 B written into
 *   the device-resident matrix (uploaded or assembled) instead of being applied after every SpMV; block (Ccols[c],
 *   Bcols[b]) of every perforation pair of a well must be in the pattern given to set_pattern (the "well cliques"
 *   ISTLSolverEbos adds to the sparsity pattern in that mode), else INVALID_ARGUMENT and the matrix is left untouched.
 *   Decomposed runs: only wells that lie inside this rank's subdomain (distributed = 0).  A shared list (distributed = 1) is refused with
 *   INVALID_ARGUMENT on every rank, before anything is exchanged: the blocks that couple perforations of different subdomains are in no
 *   rank's pattern - such wells go through the operator form (opmhip_solve_system's `wells`). */
int opmhip_add_well_contributions(opmhip_ctx* ctx, const opmhip_wells* wells);
/* the right-hand side / residual currently on the device (after opmhip_assemble, opmhip_upload_system or
 * opmhip_wells_apply_residual): N doubles, natural order - what linearizer().residual() holds on the host in Flow */
int opmhip_get_rhs(opmhip_ctx* ctx, double* b);
/* replaces: StandardWell::recoverSolutionWell: xw = D^-1 (resWell - B x) with x the solution of the last
 *   opmhip_solve_system, still on the device (wells/StandardWell_impl.hpp:1298-1311); xw: num_wells x 4 (host, out) */
int opmhip_wells_recover_solution(opmhip_ctx* ctx, const opmhip_wells* wells, const double* res_well, double* xw);

/* ---- pieces of the solve, exposed for parity tests and roofline measurement ------------------------- */
/* upload a system (natural order in, internal order on the device) without solving */
int opmhip_upload_system(opmhip_ctx* ctx, const double* vals, const double* b);
/* y = A x  (Dune::MatrixAdapter::apply, linalg/WellOperators.hpp:127-138); x, y host, natural order */
int opmhip_spmv(opmhip_ctx* ctx, const double* x, double* y);
/* block ILU0 of the uploaded matrix (ParallelOverlappingILU0::update, linalg/ParallelOverlappingILU0.hpp:923-1068);
 * lu_out (nullable, nnzb*9) receives the factors in the layout of Dune's in-place ILU (strict lower = L, strict
 * upper = U, diagonal = D^-1) of the REORDERED matrix, i.e. of the block-CSR pattern that
 * reorderBlockedMatrixByPattern (bda/Reorder.cpp:179-207) produces from opmhip_get_ordering's permutation */
int opmhip_ilu0_factor(opmhip_ctx* ctx, double* lu_out);
/* v = M^-1 d (ParallelOverlappingILU0::apply, :848-903); needs opmhip_ilu0_factor first */
int opmhip_ilu0_apply(opmhip_ctx* ctx, const double* d, double* v);
/* t = A (M^-1 d) formed the way ILU0-BiCGStab forms it inside a solve - the ILU0 application, then the product, in the form in force
 * (opmhip_get_product_form: the whole matrix, or the matrix beside its U part plus the backward sweep's row sums, opmhip_config.half_product)
 * - the pair bda/cusparseSolverBackend.cu:103-118 runs per half iteration.  z (nullable) receives M^-1 d.  Needs opmhip_ilu0_factor first;
 * for parity tests of the half-product form.  ABI 10 */
int opmhip_preconditioned_product(opmhip_ctx* ctx, const double* d, double* t, double* z);
/* replaces: the weights argument of the CPR preconditioner (linalg/ISTLSolverEbos.hpp:440-475: getTrueImpesWeights /
 * getQuasiImpesWeights handed to the preconditioner factory).  weights: 3 doubles per block row, natural order - what
 * Amg::getTrueImpesWeights (linalg/getQuasiImpesWeights.hpp:89-128) returns; they stay in force for every later solve.
 * NULL: back to the weights the library computes itself (quasi-IMPES from the matrix, or - OPMHIP_PRECOND_CPR_TRUEIMPES, contexts that
 * assemble - true-IMPES from the storage term of the present state with the dt of the last opmhip_assemble). */
int opmhip_set_cpr_weights(opmhip_ctx* ctx, const double* weights);
/* replaces: the decision ISTLSolverEbos::shouldCreateSolver takes (linalg/ISTLSolverEbos.hpp:401-426) where the host takes it:
 * the next solve builds the CPR hierarchy's structure anew from the matrix it is given, whatever opmhip_config.cpr_reuse_setup
 * says.  (Contexts that assemble decide modes 0 - 2 themselves; a host that only hands matrices over - the BdaSolver plug-in -
 * knows the Newton iteration number, the library does not.) */
int opmhip_cpr_recreate(opmhip_ctx* ctx);
/* the weights of the last CPR set-up (3 per block row, natural order): diagnosis and tests */
int opmhip_get_cpr_weights(opmhip_ctx* ctx, double* weights);

/* v = M_cpr^-1 d with the CPR preconditioner of the matrix now on the device (contexts created with a CPR preconditioner;
 * needs opmhip_ilu0_factor first: the fine smoother's factors) - for parity tests of the preconditioner alone.  It refreshes the
 * hierarchy's values but does not advance the --cpr-reuse-setup rules.  In decomposed runs with opmhip_config.cpr_gather_rows >= 0
 * it is a COLLECTIVE like opmhip_solve_system: every rank must call it (the joined level's values and right-hand side are
 * all-gathered); a rank that fails before it reaches a collective leaves its peers waiting, as with any MPI-style exchange. */
int opmhip_cpr_apply(opmhip_ctx* ctx, const double* d, double* v);
/* the ordering chosen at set_pattern: toOrder/fromOrder [Nb], rowsPerColor [num colours] (any may be NULL);
 * returns the number of colours/levels or a negative status */
int opmhip_get_ordering(opmhip_ctx* ctx, int* toOrder, int* fromOrder, int* rowsPerColor);
/* what opmhip_config's "the library chooses" settings resolved to at set_pattern: info[0] the opmhip_reorder in force (never
 * OPMHIP_REORDER_AUTO), info[1] rows per chain of the line colouring (0: no chains), info[2] colours / levels, info[3] the
 * cpr_amg_ilu_levels in force (0 without a CPR preconditioner).  The reference prints the same kind of line at set-up
 * (bda/openclSolverBackend.cpp:229-246, BILU0.cpp:106-108).  ABI 8 */
int opmhip_get_ordering_info(opmhip_ctx* ctx, int info[4]);
/* --ilu-fillin-level (setupPropertyTree.cpp: preconditioner.ilulevel): the block ILU(n) of the reference's ParOverILU0 with ilulevel n
 * (level-of-fill rule of milun_decomposition, MILU variant ILU) in place of ILU0.  Call after opmhip_create and before opmhip_set_pattern
 * / the first opmhip_solve_system; later calls return OPMHIP_INVALID_ARGUMENT, as do n < 0 and n >= 1 on a decomposed context
 * (opmhip_comm_init_*).  n = 0 is ILU0, the default.  With a CPR preconditioner the level is ignored: its fine smoother is ILU0
 * (setupPropertyTree.cpp:109-110).  n >= 1: the fill is computed in the ordering's elimination order (OPMHIP_REORDER_LEVEL_SCHEDULING:
 * the natural order, the reference's preconditioner) and the sweeps run by the levels of the filled factors (opmhip_get_ordering_info
 * info[2]); OPMHIP_REORDER_AUTO resolves to OPMHIP_REORDER_DISTANCE2_COLORING (measured: DESIGN.md section 5).  A pattern
 * whose factors would hold more than 8 x nnzb blocks is refused at set_pattern with OPMHIP_INVALID_ARGUMENT.  The half-product form
 * is off (U != upper(A)).  Additive to ABI 11 */
int opmhip_set_ilu_fillin_level(opmhip_ctx* ctx, int n);
/* after set_pattern: info[0] the fill level in force (0 with a CPR preconditioner), info[1] blocks in L, info[2] blocks in U (strict parts),
 * info[3] levels (colours) per sweep */
int opmhip_get_ilu_info(opmhip_ctx* ctx, int info[4]);
/* the factors of the last factorisation in the internal order, for tests: toOrder [Nb] (natural row -> internal row), lrowptr / urowptr
 * [Nb + 1], lcol [nl], ucol [nu] (internal column numbers, ascending), L [nl * 9], U [nu * 9], invD [Nb * 9] (the inverted diagonal blocks),
 * nl / nu as opmhip_get_ilu_info reports them.  Any pointer may be NULL (size query: opmhip_get_ilu_info).  Works for n = 0 as well (then
 * the pattern is the matrix's own).  Needs a factorisation for L, U, invD */
int opmhip_get_ilu_factors(opmhip_ctx* ctx, int* toOrder, int* lrowptr, int* lcol, int* urowptr, int* ucol, double* L, double* U, double* invD);
/* what opmhip_config.half_product resolved to at set_pattern: info[0] 1 if ILU0-BiCGStab forms the product after M^-1 from the backward
 * sweep's row sums, else 0; info[1] 1 if the pattern has the property it rests on (no elimination step touches an entry right of the
 * diagonal: U == upper(A)); info[2] the blocks that product streams: the matrix beside its U part (a subdomain with ghost columns: its interior tiles' rows beside
 * their U part plus its boundary tiles' whole rows); info[3] launch positions of that
 * product.  ABI 10 */
int opmhip_get_product_form(opmhip_ctx* ctx, int info[4]);
/* Split assembly, for tests and measurements: on the plain ILU0 context of the half-product form (no CPR, no fill, no ghost columns, no well
 * list in its matrix-add form) opmhip_assemble writes the Jacobian straight into the two arrays the ILU0 solve reads - the matrix beside its
 * U part and the U part - and the factorisation copies nothing; the matrix's own array is brought up to date only when something reads it.
 * info[0] 1 if the next opmhip_assemble writes that way; info[1] 1 if the matrix in force lives in the two arrays only; info[2] assemblies
 * written that way so far; info[3] times the matrix's own array was gathered from them.  rest (nullable, info[2] of opmhip_get_product_form
 * x 9): the matrix beside its U part, internal order, as the product after M^-1 streams it (needs the half-product form).  matrix
 * (nullable, nnzb x 9): the matrix in force, natural order (gathers first where needed).  No ABI change: a new symbol */
int opmhip_get_split_assembly(opmhip_ctx* ctx, long long info[4], double* rest, double* matrix);
/* Device-timed repetitions of one kernel on the uploaded system, for bench.py's roofline object:
 * which = 0 SpMV, 1 ILU0 apply, 2 ILU0 factor, 3 one BiCGStab iteration's vector kernels, 4 a plain streaming read of
 * the Jacobian's value array (72 * nnzb bytes; the on-box HBM ceiling the roofline fractions are put beside), 5 / 6 the SpMV
 * with the partial sums of one / two scalar products (the forms BiCGStab launches); contexts with the half-product form in force
 * (opmhip_get_product_form): 7 the product over the matrix beside its U part, 8 the same with two scalar products, 9 the ILU0 application
 * with the backward sweeps' row sums stored.
 * Launches the kernel `reps` times back to back on the context's stream between two HIP events and returns the
 * average milliseconds per launch in *ms_per_launch. */
int opmhip_time_kernel(opmhip_ctx* ctx, int which, int reps, double* ms_per_launch);
/* CPR only: unknowns and entries of the pressure-AMG levels after the first solve (n, nnz: cap entries each); returns the
 * number of levels */
int opmhip_cpr_levels(opmhip_ctx* ctx, int* n, int* nnz, int cap);

/* ---- assembly ("linearization") half of the Newton iteration ------------------------------------------ */
/* Deck-level fluid and saturation-function tables, SI units, flat arrays: what PVTW, DENSITY, PVDG, PVTO, SWOF,
 * SGOF and ROCK provide (python/test_data/SPE1CASE1/SPE1CASE1.DATA:109-250).  Region r of the PVT tables is
 * PVTNUM r+1, of the saturation tables SATNUM r+1.  Live oil + dry gas + water (no PVTG). */
typedef struct opmhip_fluid {
    int num_pvt, num_sat;
    const double* pvtw;         /* [num_pvt*5]  p_ref, Bw_ref, c_w, mu_ref, c_v */
    const double* density;      /* [num_pvt*3]  oil, water, gas at surface conditions */
    const int* pvdg_ptr;        /* [num_pvt+1]  row ranges into pvdg */
    const double* pvdg;         /* rows (p, Bg, mu_g) */
    const int* pvto_node_ptr;   /* [num_pvt+1]  Rs-node ranges */
    const double* pvto_rs;      /* [nodes]      Rs of each node */
    const int* pvto_row_ptr;    /* [nodes+1]    row ranges into pvto; the first row of a node is the saturated point */
    const double* pvto;         /* rows (p, Bo, mu_o) */
    const int* swof_ptr;        /* [num_sat+1] */
    const double* swof;         /* rows (Sw, krw, krow, pcow) */
    const int* sgof_ptr;        /* [num_sat+1] */
    const double* sgof;         /* rows (Sg, krg, krog, pcog) */
    double rock_pref, rock_cr;  /* ROCK: reference pressure, compressibility (ebos/eclproblem.hh:1454-1486) */
    /* Wet gas (PVTG; NULL / no nodes = dry gas from PVDG, and then pvdg is mandatory): per PVT region its gas-pressure
     * nodes, per node the rows (Rv, Bg, mu_g) as the deck lists them - the saturated row first, Rv descending.  With PVTG
     * the oil component may vaporise into the gas phase: Rv, the third primary-variable meaning OPMHIP_SW_PG_RV, DRVDT cap
     * through opmhip_set_problem_extras (FluidSystem::enableVaporizedOil). */
    const int* pvtg_node_ptr;   /* [num_pvt+1]  pressure-node ranges */
    const double* pvtg_pg;      /* [nodes]      gas pressure of each node */
    const int* pvtg_row_ptr;    /* [nodes+1]    row ranges into pvtg */
    const double* pvtg;         /* rows (Rv, Bg, mu_g) */
    /* ROCKTAB: per rock region rows (p, pore-volume multiplier, transmissibility multiplier), evaluated with linear
     * extrapolation at the (effective) oil pressure: rockCompPoroMultiplier / rockCompTransMultiplier
     * (ebos/eclproblem.hh:1936-2007).  num_rock = 0: none. */
    int num_rock;
    const int* rocktab_ptr;     /* [num_rock+1] */
    const double* rocktab;
    /* Per-cell end points of the saturation functions (the deck has ENDSCALE, PCW or SWATINIT).  Non-zero: the context
     * keeps the extended intensive-quantity record and accepts opmhip_set_pcw / opmhip_set_endpoint_scaling. */
    int pc_scaling;
} opmhip_fluid;

/* primary-variable meaning per cell: BlackOilPrimaryVariables::PrimaryVarsMeaning */
#define OPMHIP_SW_PO_SG 0
#define OPMHIP_SW_PO_RS 1
#define OPMHIP_SW_PG_RV 2 /* wet gas only: oil phase absent, pressure variable = gas pressure, third variable = Rv */

/* replaces: FluidSystem / MaterialLawManager initialisation from the deck (setup, once) */
int opmhip_set_fluid(opmhip_ctx* ctx, const opmhip_fluid* fluid);

/* replaces: the per-cell / per-connection arrays EclProblem serves to the assembly
 * (ebos/eclproblem.hh:1332-1340 transmissibility, :1409 thresholdPressure, :1430-1447 porosity & depth,
 * dofTotalVolume, pvtRegionIndex/satnumRegionIndex, :1711-1732 maxGasDissolutionFactor).
 * trans, area, thpres: one value per block-CSR entry in the NATURAL pattern order (0 on diagonal entries); must be
 * symmetric ((I,J) == (J,I)); thpres may be NULL (= 0).  poro, volume, depth: per cell.  pvtnum/satnum: per cell,
 * 0-based, NULL = region 0.  rsmax: per cell cap on Rs (DRSDT), NULL = unlimited.  Needs set_pattern first. */
int opmhip_set_static(opmhip_ctx* ctx, const double* trans, const double* area, const double* thpres,
                      const double* poro, const double* volume, const double* depth, const int* pvtnum,
                      const int* satnum, const double* rsmax);

/* replaces: EclProblem::maxOilVaporizationFactor (DRVDT cap on Rv, ebos/eclproblem.hh:1734-1754), rockTableIdx_ (ROCKNUM,
 * :1943-1945) and overburdenPressure_ (:1954-1955).  Per cell, natural order, any may be NULL (no cap / table 0 / none);
 * only meaningful for a fluid with PVTG or ROCKTAB tables (else INVALID_ARGUMENT).  Needs set_static; recomputes the cached
 * intensive quantities if a state is set. */
int opmhip_set_problem_extras(opmhip_ctx* ctx, const double* rvmax, const int* rocknum, const double* overburden);

/* replaces: the DRSDT / DRVDT bookkeeping of EclProblem - maxDRs_ / maxDRv_ = rate x time-step size (ebos/eclgenericproblem.cc,
 * beginTimeStep_), lastRs_ / lastRv_ (updateCompositionChangeLimits_, ebos/eclproblem.hh:2010-2107, called when the initial
 * solution is applied, :1811, and from endTimeStep, :1125) and maxGasDissolutionFactor / maxOilVaporizationFactor
 * (:1711-1754).  drsdt / drvdt: per PVT region, in 1/s (Sm3/Sm3 per second); negative = no limit in that region; NULL = the
 * keyword is not in force.  drsdt_all_cells (per region, nullable = 0): the OILVAP option - non-zero: the limit binds every
 * cell, zero: only cells with free gas (Sg > 1e-7).  The caps then live on the device: lastRs / lastRv are taken from the
 * state now present (call it after opmhip_set_state, like initialSolutionApplied) and after every opmhip_end_time_step;
 * opmhip_begin_time_step(dt) turns them into this step's caps, replacing the rsmax / rvmax arrays of opmhip_set_static /
 * opmhip_set_problem_extras.  DRVDT needs a fluid with PVTG.  (The convective DRSDTCON variant is not built.) */
int opmhip_set_composition_change_limits(opmhip_ctx* ctx, const double* drsdt, const int* drsdt_all_cells, const double* drvdt);

/* replaces: ROCKCOMP's hysteresis mode IRREVERS - minOilPressure_ (ebos/eclgenericproblem.cc:155-170; initialised from the
 * initial state, ebos/eclproblem.hh:2293-2294; updateMinPressure_, :2172-2197; used by rockCompPoroMultiplier /
 * rockCompTransMultiplier, :1948-1952, 1988-1992): the rock tables are read at min(p_o, lowest p_o the cell has seen at the
 * start of a time step).  enable != 0: start tracking from the state now present; 0: reversible compaction again.  Needs a
 * fluid with ROCKTAB. */
int opmhip_set_irreversible_compaction(opmhip_ctx* ctx, int enable);

/* replaces: VAPPARS - EclProblem::maxOilSaturation (ebos/eclproblem.hh:1682-1688; initialised from the initial state,
 * :2291-2292; updateMaxOilSaturation_, :2110-2141) and what the PVT classes make of it: saturated Rs x max(1e-3, (S_o /
 * S_o,max)^vap2), saturated Rv x max(1e-3, (S_o / S_o,max)^vap1) where S_o is below the largest oil saturation the cell has
 * seen at the start of a time step (LiveOilPvt / WetGasPvt of opm-material, absent from the reference tree: restated).
 * enable != 0: start tracking from the state now present.  The power function makes this the one feature whose device
 * results agree with the CPU restatement to rounding (1e-12 of a quantity's magnitude, measured 1.1e-13), not to the bit.  Needs a context with the extended
 * record (a fluid with PVTG, ROCKTAB or pc_scaling). */
int opmhip_set_vappars(opmhip_ctx* ctx, int enable, double vap1, double vap2);

/* replaces: water-induced rock compaction (ROCKCOMP with ROCK2D / ROCK2DTR / ROCKWNOD) - the tables rockCompPoroMultWc_ /
 * rockCompTransMultWc_ (built in ebos/eclgenericproblem.cc:186-240), their use in rockCompPoroMultiplier /
 * rockCompTransMultiplier (ebos/eclproblem.hh:1962-1967, 2001-2005: multiplier(effective oil pressure, SwMax - Sw_initial),
 * SwMax = max(Sw, the largest Sw the cell has seen at the start of a time step), extrapolating) and the tracker
 * maxWaterSaturation_ (initialised from the initial state, :2289-2290; updateMaxWaterSaturation_, :2144-2169, run by
 * opmhip_begin_time_step - including its statement :2150, which hands cell 1 the stored maximum of cell 0 before the loop).
 * num_tables rock regions (0: feature off), selected per cell by the rocknum of opmhip_set_problem_extras; table t has
 * num_pressure[t] >= 2 pressure nodes [Pa] (ROCK2D records) and num_sw[t] >= 2 saturation nodes (ROCKWNOD), both ascending
 * and concatenated over the tables; pv_mult / trans_mult: num_pressure[t] x num_sw[t] values per table, row-major by pressure
 * node, concatenated; trans_mult NULL = no ROCK2DTR (multiplier 1).  The initial water saturation and the tracker start from
 * the state now present: call it after opmhip_set_state.  Not together with ROCKTAB tables in the fluid (the reference reads
 * the one or the other); needs a context with the extended record (a fluid with PVTG or pc_scaling).  The table class
 * (UniformXTabulated2DFunction of opm-material) is absent from the reference tree: restated, see oracle/blackoil.hpp. */
int opmhip_set_water_compaction(opmhip_ctx* ctx, int num_tables, const int* num_pressure, const int* num_sw, const double* pressure,
                                const double* sw, const double* pv_mult, const double* trans_mult);
/* the tracker of the above per cell (natural order, Nb + Nghost entries; zeros when the feature is off) */
int opmhip_get_max_water_saturation(opmhip_ctx* ctx, double* max_water_saturation);

/* replaces: the per-cell work of EclProblem::beginTimeStep (ebos/eclproblem.hh:1042-1075) for a time step of size dt [s]:
 * updateMaxWaterSaturation_, updateMinPressure_, updateMaxOilSaturation_, the DRSDT / DRVDT caps of this step, invalidateAndUpdateIntensiveQuantities(0); and, since
 * recycleFirstIterationStorage() is false with DRSDT / DRVDT (:1758-1765), the old time level's storage term formed with ITS
 * caps (time index 1: lastRs / lastRv without the increment) - opmhip_assemble(iteration 0) then leaves it alone.  Call it
 * after opmhip_advance_time_level, and again before every retry of a chopped step.  Also updateHysteresis_ (:1060) when
 * opmhip_set_hysteresis is in force.  A no-op (SUCCESS) when none of these features is in force. */
int opmhip_begin_time_step(opmhip_ctx* ctx, double dt);

/* the trackers, for restart files and tests: lastRs, lastRv, minimum oil pressure, maximum oil saturation per cell (natural
 * order, Nb + Nghost entries each; any may be NULL; an array that is not kept comes back as zeros) */
int opmhip_get_trackers(opmhip_ctx* ctx, double* last_rs, double* last_rv, double* min_oil_pressure, double* max_oil_saturation);

/* replaces: the per-cell scaled end point maxPcow of the oil-water capillary pressure - the PCW array of the deck, or
 * what SWATINIT made of it during equilibration (ebos/equil/initstateequil.hh:1330-1343 -> EclMaterialLawManager::
 * applySwatinit) - as EclEpsTwoPhaseLaw applies it with enablePcScaling: pcow(Sw) = table(Sw) * (pcw / table(Swl)),
 * the factor taken as 1 where pcw equals the table's own maximum.  (opm-material is absent from the reference tree:
 * restated from its published form, see oracle/blackoil.hpp.)  pcw: per cell, natural order, Pa; NULL = unscaled.
 * Needs a fluid with pc_scaling set, and set_static first. */
int opmhip_set_pcw(opmhip_ctx* ctx, const double* pcw);

/* Saturation end-point scaling (ENDSCALE, SCALECRS, SWL ... SOGCR, KRW / KRO / KRG, KRWR / KRORW / KRORG / KRGR, PCW / PCG).
 * replaces: the per-cell scaled end points the EclMaterialLawManager holds and hands to the material laws
 * (materialLawParams(elemIdx), ebos/eclproblem.hh:1490-1498; EclEpsScalingPointsInfo / EclEpsConfig / EclEpsTwoPhaseLaw of
 * opm-material, which is absent from the reference tree: restated from its published form, see oracle/fluid.hpp).
 * Indices of the end points of a cell / of a saturation region's tables: */
enum {
    OPMHIP_EPS_SWL = 0,  /* connate water */        OPMHIP_EPS_SWCR = 1,    /* critical water */
    OPMHIP_EPS_SWU = 2,  /* maximum water */        OPMHIP_EPS_SOWCR = 3,   /* critical oil in water */
    OPMHIP_EPS_SGL = 4,  /* connate gas */          OPMHIP_EPS_SGCR = 5,    /* critical gas */
    OPMHIP_EPS_SGU = 6,  /* maximum gas */          OPMHIP_EPS_SOGCR = 7,   /* critical oil in gas */
    OPMHIP_EPS_MAXPCOW = 8,  /* PCW */              OPMHIP_EPS_MAXPCGO = 9, /* PCG */
    OPMHIP_EPS_MAXKRW = 10,  /* KRW */              OPMHIP_EPS_MAXKROW = 11, /* KRO (oil-water) */
    OPMHIP_EPS_MAXKRG = 12,  /* KRG */              OPMHIP_EPS_MAXKROG = 13, /* KRO (gas-oil) */
    OPMHIP_EPS_KRWR = 14, OPMHIP_EPS_KRORW = 15, OPMHIP_EPS_KRGR = 16, OPMHIP_EPS_KRORG = 17,   /* values at the displacing phase's critical saturation */
    OPMHIP_EPS_COUNT = 18
};
typedef struct opmhip_endpoint_scaling {
    int sat_scaling;     /* ENDSCALE: two-point scaling of the saturation axis of every curve */
    int three_point_kr;  /* SCALECRS YES: the relative permeabilities keep a third point (the other phase's critical saturation) */
    int krw, kro, krg;   /* vertical scaling of krw / kro (krow and krog) / krg: 0 none, 1 at the maximum (KRW / KRO / KRG), 2 also
                          * at the displacing phase's critical saturation (KRWR / KRORW, KRORG / KRGR) */
    int pcw, pcg;        /* PCW / PCG: capillary pressures scaled to the cell's maximum */
    const double* points[OPMHIP_EPS_COUNT]; /* per cell (natural order, Nb + Nghost entries), SI; NULL = the end point of the
                                             * cell's SATNUM tables (opmhip_sat_end_points) */
} opmhip_endpoint_scaling;
/* Needs a fluid with pc_scaling set, and set_static.  eps == NULL: scaling off.  Recomputes the cached intensive quantities
 * if a state is set.  Not to be combined with opmhip_set_pcw (PCW then is points[OPMHIP_EPS_MAXPCOW] with pcw = 1).
 * Refused with OPMHIP_INVALID_ARGUMENT, naming the cell and its saturation region, before anything changes: with sat_scaling, points
 * that leave a curve no saturation interval (the maps divide by its length); a vertical mode for a curve whose table denominator is 0
 * - the table's maximum in mode 1, its value at the displacing phase's critical saturation in mode 2.  With opmhip_set_hysteresis
 * in force the imbibition points and regions are held to the same; opmhip_set_hysteresis checks them under the options in force. */
int opmhip_set_endpoint_scaling(opmhip_ctx* ctx, const opmhip_endpoint_scaling* eps);
/* the end points of the tables of saturation region sat_region (opm-common's satfunc end-point extraction, restated):
 * out[OPMHIP_EPS_COUNT].  Needs opmhip_set_fluid only. */
int opmhip_sat_end_points(opmhip_ctx* ctx, int sat_region, double* out);

/* replaces: relative-permeability hysteresis - SATOPTS HYSTER / EHYSTR / IMBNUM: the per-cell material-law parameters the
 * EclMaterialLawManager serves (ebos/eclproblem.hh:1490-1498 materialLawParams) with EclHysteresisTwoPhaseLaw as the two-phase
 * law, and their update at the start of a time step (updateHysteresis_, :1060, 2603-2626, done by opmhip_begin_time_step).
 * kr_model = EHYSTR item 2: 0 = Carlson's model for the non-wetting phases (oil in the oil-water system, gas in the gas-oil
 * system), wetting phases on their drainage curves; 1 = the same with the wetting phases on their IMBIBITION curves; other
 * values are refused as the reference refuses them (opm/simulators/utils/PartiallySupportedFlowKeywords.cpp:299-302: "only
 * Carlson Hysteresis Models supported (0 or 1)"; capillary pressures stay on the drainage curves, :502-507); negative = not in
 * force.  imbnum: per cell (natural order, Nb + Nghost) the saturation region (0-based, of opmhip_fluid's SWOF / SGOF tables)
 * that holds the imbibition curves; the drainage curves are those of set_static's satnum.  imb (nullable; only with
 * opmhip_set_endpoint_scaling in force): its points[] are the scaled end points of the IMBIBITION curves (ISWL, ISWCR, ...;
 * NULL entries = the imbibition tables' own), its flags are ignored (those of the drainage scaling apply).  The state per cell
 * and two-phase system - the smallest wetting saturation seen at the start of a time step (krnSwMdc; restart vectors KRNSW_OW /
 * KRNSW_GO, ebos/eclwriter.hh:285-288) and the imbibition curve's shift (deltaSwImbKrn) - starts at "nothing seen" (2, 0);
 * the first opmhip_begin_time_step sets it from the state then present, as the reference's first beginTimeStep does.  Needs a
 * context with the extended record (a fluid with PVTG, ROCKTAB or pc_scaling) and set_static.  The law itself lives in
 * opm-material, which is not in the reference tree: restated from its published form, UNVERIFIED (oracle/fluid.hpp). */
int opmhip_set_hysteresis(opmhip_ctx* ctx, int kr_model, const int* imbnum, const opmhip_endpoint_scaling* imb);
/* the hysteresis state per cell (natural order, Nb + Nghost; any NULL): turning point and shift of the oil-water system, of
 * the gas-oil system (what eclwriter writes as KRNSW_OW / KRNSW_GO - PCSWM_* are equal to them: the reference updates both with
 * the same saturation) */
int opmhip_get_hysteresis(opmhip_ctx* ctx, double* krn_sw_mdc_ow, double* delta_sw_imb_krn_ow, double* krn_sw_mdc_go, double* delta_sw_imb_krn_go);
/* replaces: initHysteresisParams of a restarted run (ebos/ecloutputblackoilmodule.hh:569-589 -> setOilWaterHysteresisParams /
 * setGasOilHysteresisParams): the turning points handed in, the shifts recomputed from them */
int opmhip_set_hysteresis_params(opmhip_ctx* ctx, const double* krn_sw_mdc_ow, const double* krn_sw_mdc_go);

/* Point evaluation of the fluid-system and saturation functions the assembly uses, ON THE DEVICE, for host-side setup
 * code (equilibration, ebos/equil/initstateequil.hh) and for tests that pin these functions against the reference's
 * EQUIL expectations.  For each of n points: out[8 i + 0..7] = 1/B_w(p), 1/B_g(p), 1/B_o(p, rs) (the saturated curve
 * where rs >= RsSat(p), as the equilibration's oil density does, initstateequil.hh:214-233), RsSat(p), pcow(sw),
 * pcgo(sg), mu_o(p, rs) [Pa s], mu_g(p).  Needs opmhip_set_fluid only.  All arrays host memory. */
int opmhip_fluid_probe(opmhip_ctx* ctx, int pvt_region, int sat_region, int n, const double* p, const double* rs,
                       const double* sw, const double* sg, double* out);

/* The saturation functions at (sw, sg) the same way, optionally with ONE set of scaled end points (eps: flags as in
 * opmhip_set_endpoint_scaling, points[f] pointing at ONE double each or NULL = the table's own; eps == NULL: unscaled):
 * out[5 i + 0..4] = krw, kro, krg, pcow, pcgo.  What an equilibration with ENDSCALE inverts per cell (equil.py). */
int opmhip_sat_probe(opmhip_ctx* ctx, int sat_region, const opmhip_endpoint_scaling* eps, int n, const double* sw, const double* sg,
                     double* out);

/* The gas-phase functions at (p_g, Rv) the same way: out[3 i + 0..2] = 1/B_g, mu_g (on the saturated curve where
 * Rv >= RvSat(p_g), as the equilibration's gas density does, initstateequil.hh:240-285), RvSat(p_g).  Dry-gas fluids:
 * 1/B_g(p), mu_g(p), 0. */
int opmhip_gas_probe(opmhip_ctx* ctx, int pvt_region, int n, const double* p, const double* rv, double* out);

/* replaces: model().solution(0) = ... ; model().invalidateAndUpdateIntensiveQuantities(0)
 * (flow/BlackoilModelEbos.hpp:552-562).  pv: Nb x 3 (Sw, p_o, Sg|Rs), meaning: Nb bytes. Natural order. */
int opmhip_set_state(opmhip_ctx* ctx, const double* pv, const unsigned char* meaning);
int opmhip_get_state(opmhip_ctx* ctx, double* pv, unsigned char* meaning);

/* replaces: BlackoilModelEbos::relativeChange (flow/BlackoilModelEbos.hpp:431-510), the error measure of the PID time-step
 * control (timestepping/TimeStepControl.cpp:127-161; Flow's default --time-step-control=pid+newtoniteration): the sum over
 * the owned cells of (p_new - p_old)^2 + sum_phases (S_new - S_old)^2 over the sum of p_new^2 + sum_phases S_new^2, new = the
 * state on the device, old = the time level opmhip_advance_time_level kept; summed over the ranks of a decomposed run.  Call
 * it after an accepted time step.  The cells are summed by a fixed tree: equal to the reference's sequential sum to rounding. */
int opmhip_relative_change(opmhip_ctx* ctx, double* relative_change);

/* The two time levels of the discretisation (opm-models FvBaseDiscretization: advanceTimeLevel() copies solution(0)
 * into solution(1) when a time step starts; updateFailed() copies it back and recomputes the intensive quantities
 * when the Newton method gave up - the path AdaptiveTimeSteppingEbos takes before it retries with a shorter step,
 * opm/simulators/timestepping/AdaptiveTimeSteppingEbos.hpp:355-441).  Device-to-device, ghost cells included,
 * asynchronous on the context's stream.  update_failed needs a preceding advance_time_level (else NOT_READY). */
int opmhip_advance_time_level(opmhip_ctx* ctx);
int opmhip_update_failed(opmhip_ctx* ctx);

/* replaces: the drift part of EclProblem::endTimeStep (ebos/eclproblem.hh:1126-1135) and of EclProblem::source
 * (:1847-1875).  Flow compensates systematic mass drift by default (EclEnableDriftCompensation = true, :496-498): after
 * every ACCEPTED time step of size dt the residual of its last linearisation, times dt, is remembered per cell and
 * subtracted as a rate from the source term of the following steps, capped at max_compensation (default 10 x
 * NewtonTolerance = 0.1, :352-356, :1854) of the cell's pore volume per step.  opmhip_end_time_step stores
 * residual * dt on the device (asynchronous; a rolled-back step never reaches it, so opmhip_update_failed leaves the
 * drift alone); opmhip_assemble applies it.  opmhip_set_drift_compensation(enable = 0) = --ecl-enable-drift-compensation=false;
 * switching it either way clears the stored drift. */
int opmhip_end_time_step(opmhip_ctx* ctx, double dt);
int opmhip_set_drift_compensation(opmhip_ctx* ctx, int enable, double max_compensation);

/* replaces: EclProblem::source (ebos/eclproblem.hh:1823-1845): total surface-volume rate per cell and equation
 * [m^3/s] (what BlackoilWellModel::computeTotalRatesForDof adds up, wells/BlackoilWellModel_impl.hpp:496-512) and
 * its 3x3 derivative w.r.t. the cell's primary variables.  Either may be NULL (= zero). */
int opmhip_set_source(opmhip_ctx* ctx, const double* source, const double* dsource);
/* The same for a well model: the rates of `n` perforated cells (natural local ids; a cell named twice receives the sum), every other
 * cell's source and derivative zero.  source[n*3], dsource[n*9] (nullable = zero).  What crosses PCIe is 100 bytes per perforation
 * instead of 96 bytes per cell of the grid (computeTotalRatesForDof visits the perforations, wells/BlackoilWellModel_impl.hpp:496-512).
 * n == 0: no sources at all.  ABI 11 */
int opmhip_set_source_cells(opmhip_ctx* ctx, int n, const int* cells, const double* source, const double* dsource);

/* ---- analytic aquifers (Carter-Tracy, Fetkovich), resident on the device.  Additive to ABI 11 ----------------------------
 * replaces: aquiferModel_.addToSource in EclProblem::source (ebos/eclproblem.hh:1843) and the classes behind it,
 * opm/simulators/aquifers/AquiferInterface.hpp, AquiferCarterTracy.hpp, AquiferFetkovich.hpp, BlackoilAquiferModel_impl.hpp.
 * An aquifer's influx depends on the connected cell's present water pressure and carries a derivative, so it is formed anew in
 * front of every linearisation - on the device, from the cached intensive quantities, without a host round trip.  The aquifers'
 * state (pressure_previous_, W_flux_, fluxValue_, aquifer_pressure_) lives on the device from time step to time step.
 * The list: the aquifers concatenated, Carter-Tracy first, then Fetkovich - the order of BlackoilAquiferModel::addToSource
 * (BlackoilAquiferModel_impl.hpp:112-127); only what the in-tree code reads from AQUCT_data / AQUFETP_data.  Every per-aquifer
 * array has num_aquifers entries; an entry that belongs to the other type is ignored.
 * NOT covered: decomposed contexts (alphai_, the equilibrium pressure and W_flux_ are sums over the ranks: refused); numerical
 * aquifers (they are grid cells and need nothing from this library); the AQUTAB default influence table and the deck-level
 * formulas for the time constant and the influx constant (opm-common's, not in the reference tree: the caller hands in Tc, beta
 * and the table). */
typedef struct opmhip_aquifers {
    int num_aquifers;
    const int* type;               /* 0 Carter-Tracy, 1 Fetkovich; no Carter-Tracy aquifer behind a Fetkovich one */
    const int* id;                 /* aquiferID, reported back only */
    const int* conn_pointers;      /* [num_aquifers + 1] connection ranges */
    const int* cell;               /* per connection: natural id of an owned cell; within one aquifer a cell at most once
                                    * (cellToConnectionIdx_ keeps one connection per cell, AquiferInterface.hpp:248); a cell may be in several aquifers */
    const double* alpha;           /* per connection: alphai_, the normalised area fraction (initializeConnections, :224-317, is grid work: the caller's) */
    const double* time_constant;   /* Tc_ [s], > 0 */
    const double* water_density;   /* rhow_ */
    const double* datum_depth;     /* aquiferDepth() */
    const double* initial_pressure;     /* pa0_ where has_initial_pressure is set */
    const int* has_initial_pressure;    /* 0: equilibrate with the reservoir at opmhip_set_aquifers (calculateReservoirEquilibrium, :330-373); NULL = all given */
    const double* influx_constant; /* Carter-Tracy: beta_ */
    const int* table_pointers;     /* [num_aquifers + 1] node ranges of the influence tables (Carter-Tracy: >= 2 nodes, td ascending; Fetkovich: empty) */
    const double* td;              /* dimensionless_time nodes */
    const double* pd;              /* dimensionless_pressure nodes */
    const double* prod_index;      /* Fetkovich */
    const double* total_compr;     /* Fetkovich; total_compr * initial_watvolume > 0 */
    const double* initial_watvolume;    /* Fetkovich */
    const int* has_restart;        /* restart values (initFromRestart, :91-102); NULL = none.  Refused for a Carter-Tracy aquifer as the
                                    * reference refuses them (AquiferCarterTracy.hpp:107-111) */
    const double* restart_W_flux;  /* W_flux_ */
    const double* restart_pressure;     /* Fetkovich: aquifer_pressure_ */
} opmhip_aquifers;
/* replaces: initialSolutionApplied -> initQuantities (AquiferInterface.hpp:104-107, 167-183): call it after opmhip_set_static and
 * opmhip_set_state.  NULL or num_aquifers == 0 clears the list.  Where the initial pressure is absent it is computed once, here:
 * p_w and rho_w of the connected cells are gathered from the intensive-quantity cache and summed on the host in ascending cell
 * order (the reference's element loop) with the gravity constant the assembly uses.  W_flux_ = 0 unless restart data was given.
 * OPMHIP_NOT_READY before static / state; OPMHIP_INVALID_ARGUMENT (the text names the reason) for a null array or inconsistent
 * pointers, a cell outside [0, Nb) or repeated within an aquifer, Tc <= 0, a table that is not ascending or has fewer than two nodes,
 * total_compr * initial_watvolume <= 0, restart data for a Carter-Tracy aquifer, a decomposed context.  A refused call leaves no list set. */
int opmhip_set_aquifers(opmhip_ctx* ctx, const opmhip_aquifers* aquifers);
/* replaces: AquiferInterface::beginTimeStep (:109-128) - pressure_previous_ = p_w of the state now present, on the device - and the
 * per-step scalars of calculateEqnConstants / getInfluenceTableValues (AquiferCarterTracy.hpp:113-160: td = time / Tc, PI(td + dt)
 * and its derivative by linear interpolation with linear extrapolation - opm-common's linearInterpolation is not in the reference
 * tree: restated, UNVERIFIED) and of AquiferFetkovich::calculateInflowRate (:143-144: (1 - exp(-dt / Tc)) / (dt / Tc)); computed on
 * the host, sent up asynchronously.  time = simulator.time(), the start of the step.  Call it beside opmhip_begin_time_step, and again
 * before every retry of a chopped step.  A no-op without aquifers. */
int opmhip_aquifers_begin_time_step(opmhip_ctx* ctx, double time, double dt);
/* what aquiferData() reports, per aquifer (any pointer may be NULL): W_flux_ (volume), pressure (Fetkovich: aquifer_pressure_,
 * Carter-Tracy: pa0_), the sum of the last assemble's Qai_ in connection order (fluxRate), pa0_ (initPressure) */
int opmhip_get_aquifers(opmhip_ctx* ctx, double* W_flux, double* pressure, double* flux_rate, double* init_pressure);
/* for tests: Qai_ of the last assemble per connection, q4[4 i + 0..3] = value, d/dSw, d/dp, d/dX */
int opmhip_get_aquifer_rates(opmhip_ctx* ctx, double* q4);
/* With aquifers set:
 * opmhip_assemble returns OPMHIP_NOT_READY before the first opmhip_aquifers_begin_time_step and OPMHIP_INVALID_ARGUMENT when its dt
 * is not that call's.  Every assemble forms Qai_ from the state now present (calculateInflowRate in the statement order of
 * AquiferCarterTracy.hpp:135-169 / AquiferFetkovich.hpp:112-148) and adds it, with its three derivatives (p_w depends on Sw and p),
 * to the water equation's source of the connected cells, Carter-Tracy before Fetkovich.  The caller's source arrays hold exactly
 * what the caller put there afterwards: the connected cells' water rows are saved, raised and restored around the assembly
 * kernel, traffic proportional to the connections.  Per cell the assembly forms ((w + Q_1 + ...) / V - drift) * V where the
 * reference forms w / V + Q_1 / V + ... (ebos/eclproblem.hh:1838-1843): at most one rounding apart, and only in a cell that has both
 * a well rate and an aquifer connection.
 * opmhip_end_time_step also does endTimeStep of both classes (AquiferCarterTracy.hpp:62-70, AquiferFetkovich.hpp:64-70): W_flux_ += Q_i * dt
 * over the aquifer's connections in connection order; fluxValue_ = W_flux_; aquifer_pressure_ = pa0_ - W_flux_ / (total_compr *
 * initial_watvolume).  opmhip_update_failed leaves the aquifers alone: a rolled-back step never reaches endTimeStep. */

/* ---- open boundaries (the BC keyword: FREE and RATE faces), resident on the device.  Additive to ABI 11 ----------------------
 * replaces: EclProblem::boundary (ebos/eclproblem.hh:1602-1671) with the lists readBoundaryConditions_ (:2686-2830) builds, the
 * boundary gradients of the flux module (calculateBoundaryGradients_, ebos/eclfluxmodule.hh:362-468) and what the local residual
 * does with a boundary rate vector (evalBoundary_: rate times the face's area, ADDED to the interior cell's residual).
 * A FREE face's flux depends on the interior cell's present pressures, densities and mobilities and carries a 3 x 3 derivative, so
 * it is formed anew in front of every linearisation - on the device, from the cached intensive quantities.
 * The list: one entry per boundary face, in any order; the faces of one cell are applied in list order.
 * SIGN: a boundary rate is positive OUT of the domain.  boundary() passes the deck's RATE on without a sign change, so a positive
 * rate of a RATE face leaves the domain and an influx is negative.
 * FREE: the exterior fluid state is initialFluidStates_[globalDofIdx] - the interior cell's own state at the moment of
 * opmhip_set_boundary_conditions, values only: phase pressures, densities, mobilities, 1/B, Rs (and Rv on the extended record).
 * Per phase, in the reference's statement order: rhoAvg = (rhoIn + rhoEx) / 2; pEx += rhoAvg * (distZ * g), distZ = zIn - zFace;
 * dp = pEx - pIn; dp > 0: the exterior is upstream, q = dp * mobEx * (-trans / area) with the captured mobility as a plain number
 * (the reference re-evaluates the relative permeabilities of the exterior state with the cell's material parameters: without
 * hysteresis that IS the captured mobility); otherwise q = dp * mobIn * (-(trans * tmult) / area), tmult the value of the cell's
 * ROCKTAB transmissibility multiplier (rockCompTransMultiplier<double>, 1 without tables).  Derivatives: the interior cell's.
 * From phase volume fluxes to the three equations (BlackOilBoundaryRateVector::setFreeFlow / setMassRate and evalPhaseFluxes_ are
 * opm-models', not in the reference tree: restated from the published form, UNVERIFIED): per phase the RAW phase pressures
 * pBoundary (captured) and pInside, without the gravity term, choose the fluid state that supplies 1/B, Rs and Rv - pBoundary <
 * pInside: the interior's, with derivatives; pBoundary > pInside: the captured one's; equal: the phase adds nothing -, surface
 * volume flux = 1/B * q into the phase's own equation, Rs times it into the gas equation (oil phase), Rv times it into the oil
 * equation (gas phase, wet gas).  On a Z face the two direction tests may disagree (gravity): each then decides what the
 * published form lets it decide, the mobility by dp, the composition by the raw pressures.
 * RATE: rate[3] is a MASS rate per area in the equation order of opmhip_set_source (oil, water, gas); setMassRate divides each by
 * the component's reference density in the cell's PVT region (Flow conserves surface volumes); no derivative.
 * NOT covered: decomposed contexts; relative-permeability hysteresis with a FREE face; water-induced compaction tables; the
 * thermal boundary (setThermalFlow); solvent and polymer; the deck's unit conversion and the BC keyword's boxes (the caller's:
 * area, the boundary half transmissibility - ebos/ecltransmissibility.cc:241-282, the interior cell's half transmissibility alone,
 * no NTG or MULT* - and the depth of the face centre, scvf.integrationPos()[2], are handed in). */
#define OPMHIP_BC_RATE 0
#define OPMHIP_BC_FREE 1
typedef struct opmhip_boundary_conditions {
    int num_faces;
    const int* cell;        /* natural id of an owned cell */
    const int* direction;   /* indexInInside: 0 X-, 1 X+, 2 Y-, 3 Y+, 4 Z-, 5 Z+; a (cell, direction) pair at most once */
    const int* type;        /* OPMHIP_BC_RATE | OPMHIP_BC_FREE */
    const double* area;     /* scvf.area(), > 0 */
    const double* trans;    /* transmissibilityBoundary, >= 0 and finite */
    const double* depth;    /* depth of the face centre */
    const double* rate;     /* [3 num_faces]: RATE faces' mass rate per area (oil, water, gas), positive out of the domain; a FREE face's
                             * entries are ignored */
} opmhip_boundary_conditions;
/* Call it after opmhip_set_static and opmhip_set_state: the exterior state of the FREE faces is captured here, on the device, from
 * the intensive-quantity cache; a second call captures again.  NULL or num_faces == 0 clears the list.
 * OPMHIP_NOT_READY before static / state; OPMHIP_INVALID_ARGUMENT (the text names the reason) for a null array, a cell outside
 * [0, Nb), a direction outside 0..5, the same (cell, direction) twice, an area that is not positive, a transmissibility that is
 * negative or not finite, an unknown type, a decomposed context, a FREE face in a context with relative-permeability hysteresis,
 * a context with water-induced compaction tables.  A refused call leaves no list set.
 * With a list set, every opmhip_assemble forms the faces' rates from the state now present and SUBTRACTS them (the source is a rate
 * into the cell) from the source and its derivative of the boundary cells, behind the wells' and the aquifers' terms; the caller's
 * source arrays hold exactly what the caller put there afterwards (12 doubles per distinct boundary cell are saved and restored
 * around the assembly kernel).  Without a list nothing is launched. */
int opmhip_set_boundary_conditions(opmhip_ctx* ctx, const opmhip_boundary_conditions* bc);
/* for tests and reports: per face the last assemble's contribution to the interior cell's residual, area included, positive out of
 * the cell: q12[12 f + e] the three equations (oil, water, gas), q12[12 f + 3 + 3 e + v] their derivatives with respect to the cell's
 * primary variables */
int opmhip_get_boundary_rates(opmhip_ctx* ctx, double* q12);

/* ---- passive tracers, resident on the device.  Additive to ABI 11 ------------------------------------------------------------
 * EclTracerModel (ebos/ecltracermodel.hh:113-134, 156-439; ebos/eclgenerictracermodel.cc:86-281): tracers carried by one phase each,
 * advanced once per time step by one scalar transport solve per phase from the converged state - the cached intensive quantities, the
 * transmissibilities, areas, THPRES, depths and volumes of opmhip_set_static, all of them in HBM already.  The tracers of one phase share
 * their matrix and differ in their right-hand sides (ecltracermodel.hh:476-479); the reference solves them one after the other
 * (eclgenerictracermodel.cc:272-277), here they advance in lock step, their vectors interleaved per cell, so that every product and
 * sweep reads a matrix or factor entry once for all of them.
 * The equations, per phase and cell I (assembleTracerEquations_, :216-337), every sum sequential in this order:
 *   storage  r_t[I] = ((vol c_t[I] - storage1_t[I]) V) / dt,  M[I][I] = (vol V) / dt,  vol = max(S b porosity, 1e-10) (computeVolume_, :158-179);
 *   faces in ascending natural column index (the stencil's own face order is opm-grid's and not in the reference tree: UNVERIFIED):
 *            f = A v b_up with v the phase's volumeFlux evaluated with I as the interior cell - the value arithmetic of the assembly's
 *            face flux (ebos/eclfluxmodule.hh:212-357) -, r_t[I] += f c_t[up]; where I is upstream M[I][I] += f and M[J][I] = -f
 *            (:285-288), the entry (I, J) being filled from a second evaluation with J as the interior cell;
 *   wells    per connection, in list order, with q the phase's component surface rate, positive into the reservoir
 *            (volumetricSurfaceRateForConnection, wells/WellInterface_impl.hpp:434-445): q > 0: r_t[I] -= q c_inj[t]; q < 0:
 *            r_t[I] -= q c_t[I] and M[I][I] -= q (:293-336).
 * The solver (eclgenerictracermodel.cc:248-281): ILU0 with relaxation 1 and BiCGStab from x = 0, defect reduction 1e-2, at most 100
 * iterations.  Dune's BiCGSTABSolver and SeqILU are not in the reference tree: the recurrence is the block solver's (right-preconditioned,
 * the stopping test at each half iteration, bda/cusparseSolverBackend.cu:60-184) and the factorisation an exact ILU0 of the matrix in the
 * context's ordering, scheduled by the level sets of its lower triangle.  Iteration counts are UNVERIFIED against Dune's.
 * NOT covered: gas tracers (refused: the library's fluid always carries dissolved gas and the reference refuses gas tracers under DISGAS,
 * ecltracermodel.hh:465-467), oil tracers on a fluid with PVTG (refused, :455-457), decomposed contexts (refused, as doInit gives up
 * on parallel runs, eclgenerictracermodel.cc:105-111), restart output, partitioned or adsorbing tracers, the TBLK / TVDPF parsing
 * (opm-common's: the caller hands in concentrations). */
#define OPMHIP_TRACERS_MAX_PER_PHASE 32
typedef struct opmhip_tracer_result {
    int converged;      /* 0: the stopping rule was not met within maxit iterations, or a pivot of the ILU0 was zero or not finite */
    double iterations;  /* half iterations count 0.5 (bda/cusparseSolverBackend.cu:90, 131, 172) */
    double reduction;   /* norm / norm_0 (:173); 0 where the right-hand side was zero */
} opmhip_tracer_result;
/* replaces: EclTracerModel::init -> doInit + prepareTracerBatches (eclgenerictracermodel.cc:86-245, ecltracermodel.hh:441-479).
 * phase[t]: 0 water, 1 oil, 2 gas; concentration[t * Nb + cell], natural cell order.  num_tracers = 0 clears.  Also computes, on the
 * host, the level sets of the ordering's lower triangle and the rows' faces in natural column order.  OPMHIP_NOT_READY before
 * opmhip_set_static; OPMHIP_INVALID_ARGUMENT (the text names the reason) for a gas tracer, an oil tracer on a PVTG fluid, a decomposed
 * context or one with ghost cells, a phase outside 0 .. 2, more than OPMHIP_TRACERS_MAX_PER_PHASE tracers of one phase, a null array,
 * a concentration that is not finite.  A refused call leaves no tracers set. */
int opmhip_set_tracers(opmhip_ctx* ctx, int num_tracers, const int* phase, const double* concentration);
/* replaces: the constants of linearSolve_ (eclgenerictracermodel.cc:256-262).  Defaults 1e-2, 100.  tolerance > 0 and finite, maxit >= 1 */
int opmhip_set_tracer_solver(opmhip_ctx* ctx, double tolerance, int maxit);
/* replaces: the well loop's inputs of assembleTracerEquations_ (:293-336).  cell[i]: natural cell of connection i (a cell may appear
 * several times: its connections are applied in list order); rate[3 i + phase]: the component surface rate of water, oil, gas, positive
 * into the reservoir; injected[t * n + i]: the concentration of tracer t in what connection i injects (WTRACER).  n = 0 clears; the list
 * stays until it is replaced.  Needs opmhip_set_tracers.  OPMHIP_INVALID_ARGUMENT for a cell outside [0, Nb), a null array, a value that
 * is not finite. */
int opmhip_set_tracer_connections(opmhip_ctx* ctx, int n, const int* cell, const double* rate, const double* injected);
/* replaces: EclTracerModel::beginTimeStep -> updateStorageCache (:340-359): c_initial = c, storage1 = vol(state now present) c_initial.
 * Calling it again without an end (a chopped step) reproduces the first call's values from the rolled-back state.
 * OPMHIP_NOT_READY before opmhip_set_state.  A no-op without tracers. */
int opmhip_tracers_begin_time_step(opmhip_ctx* ctx);
/* replaces: EclTracerModel::endTimeStep -> advanceTracerFields (:362-383) with linearSolveBatchwise_ (eclgenerictracermodel.cc:264-281):
 * assembles at the state now present (the converged one: the record cache is current after the last opmhip_update), solves
 * M dx_t = r_t for every tracer from x = 0 and sets c_t -= dx_t.  A solve that did not converge is applied all the same and reported,
 * as the reference does.  res: NULL or num_tracers records.  A zero or non-finite pivot of the ILU0 is replaced by 1, reported as
 * converged = 0 on every tracer of the phase and named in opmhip_last_error (the call still returns OPMHIP_SUCCESS).
 * OPMHIP_NOT_READY before the first opmhip_tracers_begin_time_step; OPMHIP_INVALID_ARGUMENT unless dt > 0.  A no-op without tracers. */
int opmhip_tracers_end_time_step(opmhip_ctx* ctx, double dt, opmhip_tracer_result* res);
/* what EclTracerModel::tracerConcentration reports: concentration[t * Nb + cell], natural order */
int opmhip_get_tracers(opmhip_ctx* ctx, double* concentration);
/* for tests: the system assembleTracerEquations_ forms for one phase at the state now present - matrix[nnzb] in the order of the
 * pattern handed to opmhip_set_pattern, residual[j * Nb + cell] for the phase's j-th tracer - nothing solved, nothing changed.
 * OPMHIP_NOT_READY before the first opmhip_tracers_begin_time_step */
int opmhip_get_tracer_system(opmhip_ctx* ctx, int phase, double dt, double* matrix, double* residual);
/* for tests: storageOfTimeIndex1_ and concentrationInitial_ of the last opmhip_tracers_begin_time_step, [t * Nb + cell] each (either may be NULL) */
int opmhip_get_tracer_storage(opmhip_ctx* ctx, double* storage1, double* concentration_initial);
/* for measurements: device milliseconds of the last opmhip_tracers_end_time_step, summed over the phases (HIP events on the context's
 * stream): ms[0] system, ms[1] ILU0 factorisation, ms[2] BiCGStab; info[0] levels of the sweeps' schedule, info[1] BiCGStab launches */
int opmhip_get_tracer_timings(opmhip_ctx* ctx, double* ms, int* info);

/* ---- standard wells, resident on the device.  Additive to ABI 11 -----------------------------------------------------------
 * The well model the Python package states on the host (wells.py StandardWells: vertical standard wells, 4 unknowns per well - the
 * surface rates of oil, water and gas INTO the reservoir and the bottom-hole pressure -, rate or BHP control with one BHP limit,
 * crossflow in producers on request (opmhip_set_std_wells_crossflow, below; off by default: a perforation that would flow against
 * its well's kind is closed), no storage term, an explicit head per completion from the perforated cell's oil density), formed on the device from
 * the cached intensive quantities: nothing of a Newton iteration crosses to the host but one read-back of 10 doubles per well.
 * The arithmetic is wells.py's arithmetic="stated", operation by operation (the library is built without floating-point
 * contraction): the per-well sums run over the perforations in perforation order, D^-1 is Gauss-Jordan on [D | I] with partial
 * pivoting (largest |entry| of the column, lowest row on ties), D^-1 r a row-times-vector product in ascending column order.
 * The head is, on request, the reference's: from the density of the mixture in the well bore above every completion
 * (opmhip_set_std_wells_head_model, below).
 * A tubing-head-pressure limit through VFPPROD / VFPINJ tables is a third control (opmhip_set_vfp_tables, opmhip_set_std_wells_thp, below).
 * Further rate limits - ORAT, WRAT, GRAT, LRAT, RESV beside the list's own target - are controls 3 .. 7 (opmhip_set_std_wells_limits, below).
 * Group production control - GCONPROD targets shared by guide rate, control 8 (GRUP) - is opmhip_set_std_wells_groups, below.
 * NOT covered: nested groups, a control on FIELD, group guide rates, efficiency factors, GCONINJE, GCONSALE / GCONSUMP and exceed actions other
 * than RATE (the groups' section below); CRAT; history-mode RESV; gas lift (ALQ is a constant per well); bhpwithflo and the robust BHP-THP intersection of
 * computeBhpAtThpLimitProd; well potentials; THP for multisegment wells; the deck-level parsing and unit conversion of VFPPROD / VFPINJ
 * (opm-common's: it stays with the caller); crossflow in injectors (refused: in the reference an injector re-injects what crosses into it,
 * because its composition - WFrac, GFrac - is an unknown while getQs pins the other components to zero; this parametrisation fixes
 * the injected composition, and a half-measure would let oil leave through an injector's wellhead), decomposed contexts (refused).
 * The matrix-add form - the wells written into the Jacobian - is opmhip_set_std_wells_matrix_add, below.
 * Phases: 0 water, 1 oil, 2 gas (the intensive-quantity record's order); components: 0 oil, 1 water, 2 gas (the equations' order). */
typedef struct opmhip_std_wells {
    int num_wells;
    const int* perf_pointers;      /* [num_wells + 1] perforation ranges, every well at least one perforation */
    const int* cell;               /* per perforation: natural id of the perforated cell; a cell may be named by several wells */
    const double* tw;              /* per perforation: connection transmissibility factor */
    const double* dz;              /* per perforation: cell depth - the well's reference depth; head = (rho_o * g) * dz */
    const int* producer;           /* per well: 1 producer, 0 injector */
    const int* inj_phase;          /* per well: the injected phase (ignored for a producer) */
    const int* rate_component;     /* per well: the component the rate target is about */
    const double* rate_target;     /* per well: surface volume rate, positive */
    const double* bhp_limit;       /* per well: lower (producer) / upper (injector) limit, the target under BHP control */
    const int* control;            /* per well: 0 rate, 1 bhp */
    const double* x;               /* optional [num_wells * 4]: q_o, q_w, q_g, bhp to start from; NULL = zeros.  (The first
                                    * opmhip_std_wells_begin_iteration(0) sets the bottom-hole pressures anew, as the host form does.) */
} opmhip_std_wells;
/* Call it once, after opmhip_set_static and opmhip_set_state; NULL or num_wells == 0 clears the list.  The list is validated, the
 * cells are permuted to the internal order, and every distinct perforated cell gets the list of its perforations in perforation
 * order.  OPMHIP_NOT_READY before static / state; OPMHIP_INVALID_ARGUMENT (the text names the reason) for a null array, inconsistent
 * pointers, a cell outside [0, Nb), an unknown phase or component, a control other than 0 / 1, a decomposed context.  A refused call
 * leaves no list set. */
int opmhip_set_std_wells(opmhip_ctx* ctx, const opmhip_std_wells* wells);
/* replaces: wellModel().beginIteration (wells/BlackoilWellModel_impl.hpp:148-171).  iteration == 0: the completions' pressure
 * differences (calculateExplicitQuantities, :824-827), then the wells alone against the frozen reservoir (prepareTimeStep /
 * solveWellEqUntilConverged: at most 20 Newton iterations of StandardWell_impl.hpp:195-420, 516-640 per well, each well stopping
 * on its own); on the first call ever the bottom-hole pressures start 1 bar below (producer) / above (injector) the first
 * perforated cell's oil pressure.  Every iteration: updateWellControls - a rate target whose BHP leaves its limit goes under BHP
 * control, under BHP control the well returns to its target once the rate exceeds it.  Asynchronous: no read-back.  A no-op without
 * a list. */
int opmhip_std_wells_begin_iteration(opmhip_ctx* ctx, int iteration);
/* replaces: StandardWell::apply(r) (wells/StandardWell_impl.hpp:1283-1296): r -= C^T D^-1 r_w with the resident r_w, B, C, D^-1 of
 * the last opmhip_assemble.  Asynchronous.  OPMHIP_NOT_READY without a list or before an assembly. */
int opmhip_std_wells_apply_residual(opmhip_ctx* ctx);
/* replaces: recoverWellSolutionAndUpdateWellState (wells/StandardWell_impl.hpp:1298-1311, BlackoilWellModel_impl.hpp:1033-1042):
 * x_w = D^-1 (r_w - B x) from the resident solution of the last solve, then the well unknowns -= relax * x_w.  Asynchronous. */
int opmhip_std_wells_update(opmhip_ctx* ctx, double relax);
/* the one read-back of a Newton iteration (any pointer may be NULL): x [num_wells * 4], control [num_wells], res_well
 * [num_wells * 4] (r_w of the last assemble: what getWellConvergence looks at).  Waits for the stream; a D that met a zero pivot
 * since the last look is reported here (see below). */
int opmhip_get_std_wells(opmhip_ctx* ctx, double* x, int* control, double* res_well);
/* WCONPROD / WCONINJE events, restart, tests (any pointer may be NULL: that part stays): the well unknowns, the controls in force,
 * the rate targets.  What the last assemble formed is stale afterwards: opmhip_solve_system wants a new assemble first. */
int opmhip_set_std_wells_state(opmhip_ctx* ctx, const double* x, const int* control, const double* rate_target);
/* for tests (any pointer may be NULL), what the last begin_iteration / assemble / update left: head [nperf], D and D^-1
 * [num_wells * 16], B and C [nperf * 12] in opmhip_wells' layout, rates [nperf * 15] (3 components x value, d/dSw, d/dp, d/dX,
 * d/dbhp), x_w [num_wells * 4] */
int opmhip_get_std_wells_blocks(opmhip_ctx* ctx, double* head, double* D, double* Dinv, double* B, double* C, double* rates, double* xw);
/* ---- crossflow in producers.  Additive to ABI 11 ----------------------------------------------------------------------------
 * replaces: the injecting branch of StandardWellEval::computePerfRate with allow_cf (wells/StandardWellEval.cpp:1023-1090; WELSPECS
 * item 10, which Flow defaults to YES) for producers, in the operation order of wells.py StandardWells(arithmetic="stated").
 * q = (q_o, q_w, q_g) are the well's rate unknowns; bhp, head, tw, b = 1/B, mob and rs those of the perforation as above.  A
 * perforation of a producer with the switch whose drawdown dd = p_o - (bhp + head) is NOT > 0 flows
 *   p_c = -q_c where q_c < 0, else 0;  P = (p_o + p_w) + p_g;  cmix_c = p_c / P      (wellSurfaceVolumeFraction, :233-243; the clamp
 *   d cmix_c / d q_j = -((delta_cj - cmix_c) / P) where q_j < 0, else 0                is processFractions' on WFrac / GFrac)
 *   cqt_i = -tw * (((mob_w + mob_o) + mob_g) * dd)
 *   volumeRatio = (cmix_w / b_w + cmix_o / b_o) + (cmix_g - rs * cmix_o) / b_g
 *   cqt_is = cqt_i / volumeRatio;  rate_c = cmix_c * cqt_is
 * Every quantity carries its value and seven derivatives: d/dSw, d/dp, d/dX of the cell, d/dbhp, d/dq_o, d/dq_w, d/dq_g.  A product
 * is (a0 b0; a0 b_i + b0 a_i), a quotient (v = a0 / b0; (a_i - v b_i) / b0), sums and differences entry by entry in the order
 * written.  If P is not > 0 (a well that has not flowed yet: the first iteration of the wells alone) or volumeRatio is not > 0, the
 * perforation stays closed for that evaluation: nothing is divided by zero or a negative, no NaN is formed.
 * Assembly: r_w[c] = q_c - sum rate_c as before; D[c][j] = delta_cj - sum_p d rate_c / d q_j for j < 3, D[c][3] as before;
 * C[j][c] = 0 - d rate_c / d q_j for j < 3 - the rows that are zero without crossflow; C[3][c], B, the source rows as before; every
 * per-well sum is added by one lane in perforation order; the guard of a well none of whose completions flows keeps its condition.
 * Perforations with dd > 0, and every perforation of a well without the switch, take the expressions of the list above in their
 * order: a well with the switch and no reversed perforation gives the same bits as without.  With the well-bore heads the stored
 * perforation rates are whatever the assembly formed, injecting signs included.
 * By default the rate model is the dry-gas one (rv = 0, d = 1, tmp_oil = cmix_o: the producing branch adds rs q_o to the gas and nothing
 * to the oil, and crossflow keeps that); opmhip_set_std_wells_vaporised_oil switches the wet-gas model on.  Left out:
 * openCrossFlowAvoidSingularity.
 * allow: per well, 0 or 1; NULL or all zeros: off.  Call it after opmhip_set_std_wells; replacing or clearing the list clears it.
 * OPMHIP_NOT_READY without a list; OPMHIP_INVALID_ARGUMENT for a value other than 0 / 1 or for an injector (the text says so).  A
 * refused call leaves the flags as they were.  What the last assemble formed is stale afterwards, as with
 * opmhip_set_std_wells_state.  A list none of whose wells has the switch launches exactly the kernels it launched before; with a
 * switch on, the wells alone and the assembly run a second instantiation of the same kernel in place of the first (15 sums per lane
 * instead of 6): the number of launches does not change.  The switch adds no state to save or restore. */
int opmhip_set_std_wells_crossflow(opmhip_ctx* ctx, const int* allow);
/* for tests: dq [nperf * 9] = d rate_c / d q_j of the last assemble, [perforation][component c][unknown j]; zeros without the
 * switch.  (opmhip_get_std_wells_blocks keeps its rates [nperf * 15] layout.) */
int opmhip_get_std_wells_rate_dq(opmhip_ctx* ctx, double* dq);
/* ---- vaporised oil in the connection rates.  Additive to ABI 11 ------------------------------------------------------------------
 * replaces: the rs / rv terms of StandardWellEval::computePerfRate (wells/StandardWellEval.cpp:999-1021 the producing branch, :1055-1073
 * the injecting / crossflow branch with d = 1 - rv rs, :1092-1112 the split into dissolved gas and vaporised oil), the per-well sums of
 * wells/StandardWell_impl.hpp:313-336 and the rates of wells/WellState.cpp:562-563, in the operation order of wells.py
 * StandardWells(arithmetic="stated", vaporised_oil=True).  Per list, off by default: the default is the dry-gas model above, on a wet-gas
 * context too - a producer in a gas cap then reports no oil for the condensate its gas carries.  With the switch on,
 * surf[ph] = b_ph * (-tw * (mob_ph * dd)), rs and rv the record's Rs and Rv with their three cell derivatives:
 *   producing perforation (dd > 0):  rate_o = surf_o + rv * surf_g;  rate_g = surf_g + rs * surf_o;  rate_w = surf_w  (both products
 *     from the surf values before either sum); for a producer perf_dis_gas = (rs * surf_o).value, perf_vap_oil = (rv * surf_g).value;
 *   reversed perforation of a producer with the crossflow switch:  d = 1 - rv * rs;  tmp_oil = (cmix_o - rv * cmix_g) / d;
 *     tmp_gas = (cmix_g - rs * cmix_o) / d;  volumeRatio = (cmix_w / b_w + tmp_oil / b_o) + tmp_gas / b_g;  cqt_is and rate_c as above.
 *     A perforation whose d is not > 0 stays closed for that evaluation, like one whose volumeRatio is not > 0 (the reference throws a
 *     NumericalIssue where d == 0).  On values only: perf_vap_oil = rv * (q_g - rs * q_o) / d, perf_dis_gas = rs * (q_o - rv * q_g) / d
 *     with q = rate_c;
 *   injectors: unchanged - the injected composition is fixed and nothing of rv enters.
 * The two split values are added per well by one lane in perforation order, like every other sum.
 * on: 0 or 1.  Call it after opmhip_set_std_wells; replacing or clearing the list clears it.  OPMHIP_NOT_READY without a list;
 * OPMHIP_INVALID_ARGUMENT (the text names the reason) for another value and for a context whose fluid has no PVTG.  A refused call
 * leaves the switch as it was.  What the last assemble formed is stale afterwards, as with opmhip_set_std_wells_crossflow.  A list
 * without the switch launches exactly the kernels it launched before; with it, the wells alone and the assembly run another
 * instantiation of the same kernel in place of the first (two more sums per lane): the number of launches does not change.  The switch
 * adds no state to save or restore.
 * UNVERIFIED in the usual sense: the reference tree holds no number for a well's rates. */
int opmhip_set_std_wells_vaporised_oil(opmhip_ctx* ctx, int on);
/* per well [num_wells] each, either pointer may be NULL: the sums of perf_dis_gas and perf_vap_oil over a producer's perforations that
 * the last opmhip_assemble formed, in the module's sign - rates into the reservoir, production negative.  Zeros for injectors, without
 * a list and with the switch off - dissolved_gas too: the default model runs the kernels it ran before, which form neither.  Waits for
 * the stream. */
int opmhip_get_std_wells_solution_rates(opmhip_ctx* ctx, double* dissolved_gas, double* vaporised_oil);
/* ---- the matrix-add form of the resident standard wells.  Additive to ABI 11 -------------------------------------------------
 * replaces: StandardWell::addWellContributions (wells/StandardWell_impl.hpp:1688-1712) on the pattern ISTLSolverEbos builds with
 * --matrix-add-well-contributions=true (flow/flow_blackoil_dunecpr.cpp:36), which holds a block (cell_a, cell_b) for every ordered pair of
 * one well's perforated cells (its clique, the diagonal included): A -= C^T D^-1 B is written into the Jacobian, so that ILU0 factors the
 * wells, the CPR pressure matrix carries them and the products run without an operator form.  Per list, off by default: a list that does
 * not ask reaches the solver as the operator A - C^T D^-1 B and launches what it launched before.
 * opmhip_set_std_wells_matrix_add, on = 1: every pair (a, b) of every well is looked up in the pattern given to opmhip_set_pattern and
 * the schedule - per DISTINCT block its contributions (well, a, b), ordered by well and then by a * np + b - is built and uploaded once;
 * the pattern and the perforated cells are fixed, nothing is rebuilt per iteration.  on = 0 frees it.  Call it after
 * opmhip_set_std_wells; replacing or clearing the list clears it.  OPMHIP_NOT_READY without a list; OPMHIP_INVALID_ARGUMENT for a value
 * other than 0 / 1 and for a block that is not in the pattern (the text names the well and the two natural cell ids).  A refused call
 * leaves the switch as it was.  The switch adds no state to save or restore.
 * opmhip_std_wells_add_to_matrix: once per Newton iteration, after opmhip_assemble (and, in the reference's order, after
 * opmhip_std_wells_apply_residual).  Asynchronous: one launch on the context's stream, no read-back, no host array.  One lane per distinct
 * block adds its contributions in list order, each blk[i][j] += -(sum_k C_a[k][i] * (sum_l D^-1[k][l] * B_b[l][j])), both sums ascending
 * from 0.0 - the expressions and, block by block, the order of opmhip_add_well_contributions on the same B, C, D^-1: the same bits.  Two
 * wells in one cell and a well that perforates a cell twice are ordinary entries of one list.  OPMHIP_NOT_READY without a list, without
 * the switch, before an assemble, and when the last assemble's wells are in the matrix already (a second call would subtract them twice).
 * Afterwards the factorisation is stale, and until the next opmhip_assemble (or an uploaded matrix) opmhip_solve_system installs no
 * operator form for the list: the plain products run, scalar products riding in them.  It still copies and checks the zero-pivot flags: a
 * flagged D^-1 is stored as zeros, so that the add is harmless and the error is reported where it is reported otherwise.
 * opmhip_std_wells_apply_residual and opmhip_std_wells_update are unchanged: both need only the resident blocks.
 * info: [0] the switch, [1] distinct target blocks, [2] contributions (pairs), [3] 1 while the last assemble's wells are in the matrix.
 * NOT covered: building the clique pattern (the caller's: grid.with_well_cliques in the Python package; a row may hold at most 64 blocks,
 * opmhip_set_static's limit); decomposed contexts (the list is refused there). */
int opmhip_set_std_wells_matrix_add(opmhip_ctx* ctx, int on);
int opmhip_std_wells_add_to_matrix(opmhip_ctx* ctx);
int opmhip_get_std_wells_matrix_add(opmhip_ctx* ctx, int info[4]);
/* ---- the heads from the well-bore density.  Additive to ABI 11 -------------------------------------------------------------
 * replaces: StandardWell::computeWellConnectionPressures (wells/StandardWell_impl.hpp:1195-1210), that is
 * computePropertiesForWellConnectionPressures (:899-1012), computeWellConnectionDensitesPressures (:1124-1189),
 * StandardWellEval::computeConnectionDensities (wells/StandardWellEval.cpp:814-960) and
 * StandardWellGeneric::computeConnectionPressureDelta (wells/StandardWellGeneric.cpp:158-193), in the statement order of
 * wells.py StandardWells(head_model="wellbore", arithmetic="stated").  Per perforation the list then also keeps the pressure in the
 * well bore there (it starts as the perforated cell's oil pressure, wells/WellState.cpp:298, and every opmhip_assemble sets it to
 * bhp + head, StandardWell_impl.hpp:468) and the three component rates of the last opmhip_assemble (zero at the start).  At
 * opmhip_std_wells_begin_iteration(0), in front of the wells alone, one wavefront per well forms
 *   p_avg = (p_perf + p_above) / 2, p_above = bhp for the first perforation, else the pressure of the perforation above;
 *   1/B_w(p_avg), RsSat(p_avg), RvSat(p_avg), 1/B_g at rv = min(|q_o| / |q_g|, RvSat) (the saturated curve where the well's oil
 *     rate is zero, rv = 0 where its gas rate is not positive), 1/B_o at rs = min(|q_g| / |q_o|, RsSat) likewise - the well rates
 *     are the well unknowns now present, the functions those of opmhip_fluid_probe / opmhip_gas_probe to the bit, the PVT region
 *     and the surface densities the perforated cell's;
 *   the flow past every perforation: the stored rates summed from the last perforation to the first; a producer all of whose
 *     stored rates are exactly zero takes tw / sum(tw) * mobility_phase / sum_phases(1/B * mobility) of the perforated cell (every
 *     phase in its own component's place.  KNOWN DIFFERENCE FROM FLOW: the reference writes the fractions in phase order - water,
 *     oil, gas - into the component slots - oil, water, gas -, so that a producer at rest in oil-bearing cells starts with a column
 *     of water; here oil mobility counts as oil.  The heads of a producer's first time step therefore differ from Flow's);
 *   the mixture |q / ((q_o + q_w) + q_g)|; without flow an injector takes its injected phase, a producer's first perforation its
 *     preferred phase and its later ones the corrected mixture x of the perforation above; the rs / rv correction with its 1e-12
 *     guards and 1 - rs rv; density = (rho_o mix_o + rho_w mix_w + rho_g mix_g) / (x_o / b_o + x_w / b_w + x_g / b_g);
 *   head = running sum of (dz * density) * g, dz = depth - depth of the perforation above (the reference depth for the first).
 * Left out: solvent, salt, temperature, distributed wells' global perforation order, InjectorType::MULTI. */
typedef struct opmhip_std_wells_wellbore {
    const double* perf_depth;      /* per perforation: its depth */
    const double* ref_depth;       /* per well: the depth the bottom-hole pressure refers to */
    const int* preferred_phase;    /* per well: 0 water, 1 oil, 2 gas (read for producers) */
} opmhip_std_wells_wellbore;
/* Call it after opmhip_set_std_wells; NULL: back to the head from the perforated cell's oil density.  Replacing or clearing the
 * list clears it.  OPMHIP_NOT_READY without a list; OPMHIP_INVALID_ARGUMENT (the text names the reason) for a null array, a depth
 * that is not finite, an unknown phase.  A refused call leaves the model as it was.  The perforation pressures are taken from
 * the perforated cells at the first opmhip_std_wells_begin_iteration(0) that follows, unless opmhip_set_std_wells_perf_state
 * came first. */
int opmhip_set_std_wells_head_model(opmhip_ctx* ctx, const opmhip_std_wells_wellbore* wellbore);
/* for tests and restart files (any pointer may be NULL), per perforation, what the last begin_iteration(0) / assemble left: density,
 * p_avg [nperf], mixture [nperf * 3] (components), perf_pressure [nperf], perf_rates [nperf * 3] (components); *perf_state_set: 1 once
 * the perforation pressures exist (taken from the cells or handed in), 0 before and without the model.  Otherwise a no-op without
 * the model. */
int opmhip_get_std_wells_wellbore(opmhip_ctx* ctx, double* density, double* p_avg, double* mixture, double* perf_pressure, double* perf_rates,
                                  int* perf_state_set);
/* restart, tests (either pointer may be NULL: that part stays; both NULL: nothing happens): the perforation pressures [nperf] and
 * the stored component rates [nperf * 3].  OPMHIP_NOT_READY without the model; OPMHIP_INVALID_ARGUMENT for rates alone while no
 * pressures exist yet.  There is no call that takes the pressures away again: opmhip_set_std_wells_head_model anew starts over. */
int opmhip_set_std_wells_perf_state(opmhip_ctx* ctx, const double* perf_pressure, const double* perf_rates);
/* With the model in force opmhip_assemble also stores bhp + head and the rates' values per perforation (no launch is added to a
 * Newton iteration), and opmhip_advance_time_level / opmhip_update_failed save / restore them with the well unknowns: the
 * reference rolls back the whole well state.  Under this model the bottom-hole pressure is an input of the heads, so the roll-back
 * also covers "the bottom-hole pressures have not been set yet": after a first time step that was given up, the next
 * opmhip_std_wells_begin_iteration(0) takes them from the cells again and yields the heads of a context that never tried the step.
 * Without it no call launches, copies or decides anything else than before. */

/* ---- VFP tables and the THP limit of the resident standard wells.  Additive to ABI 11 --------------------------------------------
 * replaces: VFPProdProperties / VFPInjProperties with wells/VFPHelpers.cpp - findInterpData (:81-145), interpolate (:181-287 VFPPROD,
 * :289-341 VFPINJ), bhp (:343-385), findTHP (:387-499) with findX (:40-66), getFlo / getWFR / getGFR (:501-590) -, the AD forms of bhp
 * (VFPProdProperties.cpp:142-172, VFPInjProperties.cpp:88-112) and the inverse look-ups thp (VFPProdProperties.cpp:37-82,
 * VFPInjProperties.cpp:47-74), in the statement order of the Python package's vfp.py, operation by operation and without contraction.
 * Everything is SI: rates m^3/s (positive on the flo axis; the rates handed to the functions are INTO the reservoir, a producer's are
 * negative - the reference's sign), pressures Pa.
 * UNVERIFIED (opm-material is not in the reference tree): the derivative of Opm::max on evaluations, stated as "a chop max(0, .) or a
 * threshold max(1e-12, .) that binds, ties included, has derivative zero".  Where the reference leaves the result undefined it is defined:
 * a NaN looked up on an axis takes the last interval, an inverse look-up that finds nothing returns the -1e100 it starts from.  An
 * injector's dwfr, dgfr, dalq are not carried (0).
 * Per table: kind (0 VFPPROD, 1 VFPINJ); the deck's table number (> 0, unique per kind); flo type (VFPPROD 0 OIL, 1 LIQ, 2 GAS; VFPINJ
 * 0 OIL, 1 WAT, 2 GAS), wfr type (0 WOR, 1 WCT, 2 WGR) and gfr type (0 GOR, 1 GLR, 2 OGR; both ignored for VFPINJ); the datum depth; five
 * axis sizes in the order flo, thp, wfr, gfr, alq (an injector's last three are ignored) and the axes themselves in that order (an
 * injector has the first two), non-decreasing; the BHP values with flo fastest: [thp][wfr][gfr][alq][flo], [thp][flo]. */
typedef struct opmhip_vfp_tables {
    int num_tables;
    const int* kind;               /* per table */
    const int* table_num;          /* per table */
    const int* flo_type;           /* per table */
    const int* wfr_type;           /* per table */
    const int* gfr_type;           /* per table */
    const double* datum_depth;     /* per table */
    const int* axis_sizes;         /* [num_tables * 5] */
    const int* axis_pointers;      /* [num_tables + 1] ranges into axes: a table's axes one after the other */
    const double* axes;
    const int* value_pointers;     /* [num_tables + 1] ranges into values */
    const double* values;
} opmhip_vfp_tables;
/* The tables are packed once into one double array and an int descriptor per table and stay resident for the context's life.  NULL or
 * num_tables == 0 clears the set.  Needs no fluid, static data or state.
 * OPMHIP_INVALID_ARGUMENT (the text names the reason) for a null array, an empty axis, an axis that decreases or is not finite, a value
 * that is not finite, an unknown kind or type, a table number <= 0, a duplicate number, inconsistent pointers.  A refused call leaves the
 * previous set in force.  Replacing or clearing the set while wells hold THP limits (which name its tables) is refused likewise: switch
 * the limits off first. */
int opmhip_set_vfp_tables(opmhip_ctx* ctx, const opmhip_vfp_tables* tables);
/* The counterpart of opmhip_fluid_probe: the functions the well kernels call, ON THE DEVICE, to the bit.  For each of n points (host
 * arrays; one lane per point): out[10 i + 0..9] = bhp, d/dthp, d/dwfr, d/dgfr, d/dalq, d/dflo of the table at (aqua, liquid, vapour, thp,
 * alq) - producers search the flo axis with -flo, injectors with flo -; d bhp / d aqua, d liquid, d vapour = (dwfr * wfr') + (dgfr * gfr')
 * - (dflo * flo') (injectors: dflo * flo'), wfr' and gfr' by the quotient rule (a' - v * b') / b with v = a / b; and
 * thp(aqua, liquid, vapour, bhp_target, alq), the inverse look-up (a producer with all-zero rates takes the first entry of the flo axis
 * and zero fractions; 0 for a table whose THP axis has fewer than two entries).  alq is ignored for an injector (NULL allowed);
 * bhp_target NULL leaves the tenth slot 0.  OPMHIP_NOT_READY without tables, OPMHIP_INVALID_ARGUMENT for a table that does not exist. */
int opmhip_vfp_probe(opmhip_ctx* ctx, int kind, int table_num, int n, const double* aqua, const double* liquid, const double* vapour, const double* thp,
                     const double* alq, const double* bhp_target, double* out);
/* The THP limit of the resident wells.  Per well: vfp_table, the deck number of a VFPPROD (producer) / VFPINJ (injector) table, 0: the
 * well has no THP limit; thp_limit; alq; dh = the table's datum depth - the well's reference depth. */
typedef struct opmhip_std_wells_thp {
    const int* vfp_table;
    const double* thp_limit;
    const double* alq;
    const double* dh;
} opmhip_std_wells_thp;
/* Call it after opmhip_set_std_wells; NULL switches it off; replacing or clearing the list clears it, as with the crossflow flags.
 * OPMHIP_NOT_READY without a list or without tables; OPMHIP_INVALID_ARGUMENT for a null array, a table number that does not exist for
 * the well's kind, a THP axis of fewer than two entries, a limit, alq or dh that is not finite, and for taking the limit from a well
 * that is under THP control.  A refused call leaves the previous values in force.  With limits in force:
 *   control value 2 (THP) exists beside 0 and 1 in opmhip_set_std_wells_state and opmhip_get_std_wells; 2 for a well without a limit is
 *     refused.  opmhip_set_std_wells' own control field keeps refusing anything but 0 / 1: a well starts under its deck mode and reaches
 *     THP through the state call or by switching;
 *   opmhip_std_wells_begin_iteration(0) sets, after the heads, dp = (rho * g) * dh per well (wells/WellHelpers.hpp:149-155), rho what the
 *     head model uses for the first perforation: the well-bore density there under the well-bore head model (perf_densities_[0], getRho()),
 *     the perforated cell's oil density otherwise; constant through the Newton iterations, as the heads are;
 *   the control equation under control 2, in the wells alone and in opmhip_assemble (replaces control_eq = bhp - bhp_from_thp,
 *     wells/WellInterfaceEval.cpp:351-354, 433-436, calculateBhpFromThp :463-504): V = bhp(table, q_w, q_o, q_g, thp_limit, alq);
 *     r_w[3] = bhp - (V - dp); D[3][j] = 0.0 - dV/dq_j for the three rate unknowns in their order (oil, water, gas); D[3][3] = 1.0.  The
 *     guard of a well without a flowing completion keeps its condition and cannot fire with D[3][3] = 1;
 *   updateWellControls (every opmhip_std_wells_begin_iteration) checks the limits in the reference's order
 *     (wells/WellInterfaceFluidSystem.cpp:170-268 producers, :100-166 injectors); the first that is violated and is not the control in
 *     force wins: 1. BHP (bhp beyond bhp_limit) -> control 1, bhp = bhp_limit; 2. the rate target exceeded -> control 0; 3. THP: current =
 *     thp(table, q_w, q_o, q_g, bhp + dp, alq) (wells/StandardWellGeneric.cpp:116-156, wells/StandardWellEval.cpp:546-583); a producer
 *     switches when thp_limit > current, an injector when thp_limit < current, to control 2 with bhp = V - dp at the rates at hand
 *     (updateWellStateWithTarget's THP case, wells/WellInterface_impl.hpp:659-667 injectors, :882-890 producers: the bhp from
 *     calculateBhpFromThp).  A well without a limit
 *     takes exactly the two branches it took before.
 * The control rides along in what opmhip_advance_time_level / opmhip_update_failed save and restore; dp is formed anew at the next
 * opmhip_std_wells_begin_iteration(0): no new state.  A list without a limit launches the kernels it launched before; with a limit the
 * wells alone, the assembly and the controls run another instantiation of the same kernels in place of the first: the number of launches
 * of a Newton iteration does not change. */
int opmhip_set_std_wells_thp(opmhip_ctx* ctx, const opmhip_std_wells_thp* thp);
/* Per well (any pointer may be NULL; waits for the stream): the tubing-head pressure the last opmhip_std_wells_begin_iteration formed
 * from the well's state (before it switched anything), this time step's hydrostatic correction dp, and V - dp of the last
 * opmhip_assemble (formed for every well with a limit, whatever its control).  Zeros for wells without a limit. */
int opmhip_get_std_wells_thp(opmhip_ctx* ctx, double* thp, double* dp, double* bhp_from_thp);

/* ---- several rate limits per resident well: ORAT, WRAT, GRAT, LRAT, RESV (WCONPROD), RESV (WCONINJE).  Additive to ABI 11 ------------
 * Per well, beside the list's own (rate_component, rate_target), its bhp_limit and its THP limit: positive surface volume rates [m^3/s],
 * resv_rate a reservoir volume rate; +infinity: no such limit; a NULL array: none of that kind.  use_list_target per well (NULL: all 1):
 * with 0 the list's own (rate_component, rate_target) is not a limit of that well - a deck record without a limit on a single component.
 * For an injector only resv_rate is read; the others must be absent. */
typedef struct opmhip_std_wells_limits {
    const double* oil_rate;
    const double* water_rate;
    const double* gas_rate;
    const double* liquid_rate;
    const double* resv_rate;
    const int* use_list_target;
} opmhip_std_wells_limits;
/* Call it after opmhip_set_std_wells; NULL switches it off; replacing or clearing the list clears it.  OPMHIP_NOT_READY without a list;
 * OPMHIP_INVALID_ARGUMENT, the text naming the reason, for: a limit that is NaN, -infinity or not > 0; a finite limit on the component
 * the list's own target names while use_list_target is 1; use_list_target = 0 for a well under control 0; taking away the limit a well is
 * under control of; a producer's limit on an injector; use_list_target other than 0 / 1.  A refused call leaves the previous values in
 * force.  With limits in force:
 *   control values 3 ORAT, 4 WRAT, 5 GRAT, 6 LRAT, 7 RESV exist beside 0 (the list's own target), 1 (BHP), 2 (THP) in
 *     opmhip_set_std_wells_state and opmhip_get_std_wells; a value whose limit the well does not have is refused.  opmhip_set_std_wells
 *     keeps refusing anything but 0 / 1: a well reaches the new modes by switching or through the state call;
 *   the control row, unknowns being rates into the reservoir (a producer's are negative), components in the order oil, water, gas:
 *     3 - 5: r_w[3] = x[c] + limit, D[3][c] = 1;  6: r_w[3] = (x_o + x_w) + limit, D[3][o] = D[3][w] = 1;
 *     7, producer (prediction mode, wells/WellInterfaceEval.cpp:320-331): r_w[3] = ((c_w x_w + c_o x_o) + c_g x_g) + limit, D[3][j] = c_j,
 *        c = RateConverter::calcCoeff (wells/RateConverter.hpp:592-646);
 *     7, injector (:215-228): r_w[3] = c_inj x[inj] - limit, D[3][inj] = c_inj, c = calcInjCoeff (:648-683);
 *     the guard of a well without a flowing completion keeps its condition;
 *   opmhip_std_wells_begin_iteration(0) forms, only when some well has a RESV limit, the field's averages (opmhip_reservoir_averages'
 *     kernels) and every such well's coefficients at the PVT region of its first perforated cell (wells/BlackoilWellModel_impl.hpp:748-759),
 *     1/B through the functions opmhip_fluid_probe / opmhip_gas_probe run: constant through the time step's Newton iterations, as the
 *     heads are; a field without pore volume leaves zeros and is reported by opmhip_reservoir_averages;
 *   updateWellControls (every opmhip_std_wells_begin_iteration) in the reference's order (wells/WellInterfaceFluidSystem.cpp:100-268):
 *     producers BHP, ORAT, WRAT, GRAT, LRAT, RESV, THP; injectors BHP, RATE, RESV, THP; the list's own target at its component's place;
 *     the first limit that is violated and is not the control in force wins.  RESV's current rate is the sum of
 *     calcReservoirVoidageRates (:702-777) at the well's present rates (:66-81, 217-231).  On a switch to a rate-type mode the well's
 *     state is left as it is (updateWellStateWithTarget's rescaling is left out, as under control 0).
 * KNOWN DIFFERENCE FROM FLOW: the reference's injector RESV and THP branches assign a local copy of the control and return true without
 * changing the well state (:140-166); here the well switches.
 * A list without limits launches the instantiations it launched before; with limits another instantiation runs in their place: the
 * number of launches of a Newton iteration does not change, and a time step gains the averages and coefficients only with a RESV limit.
 * Left out: CRAT, history-mode RESV (form WCONHIST's target from the averages and hand it in as resv_rate), FIP regions
 * other than the whole field, salt and temperature in the converter, decomposed contexts. */
int opmhip_set_std_wells_limits(opmhip_ctx* ctx, const opmhip_std_wells_limits* limits);
/* averages[5] as opmhip_reservoir_averages gives them, of the last opmhip_std_wells_begin_iteration(0) that formed them; coeff[num_wells * 3]
 * (oil, water, gas): the control equation's coefficients of every well with a RESV limit (calcCoeff for a producer, calcInjCoeff for an
 * injector), zeros otherwise; resv_current[num_wells]: the voidage rate the last controls pass formed.  Any pointer may be NULL; waits for
 * the stream.  Zeros without limits and without groups (a producer of a group with a RESV target has its calcCoeff here too). */
int opmhip_get_std_wells_resv(opmhip_ctx* ctx, double* averages, double* coeff, double* resv_current);

/* ---- group production control of the resident wells: GCONPROD / GRUP.  Additive to ABI 11 ------------------------------------------
 * A flat list of production groups, each a direct child of FIELD; every well is in at most one (well_group -1: directly under FIELD, no
 * group control).  Per group five targets - oil, water, gas, liquid surface rates and a reservoir voidage rate [m^3/s], positive,
 * +infinity: none, a NULL array: none of that kind - with the exceed action RATE, and a production control mode: 0 NONE, 1 ORAT, 2 WRAT,
 * 3 GRAT, 4 LRAT, 5 RESV.  Per well one guide rate per target mode, in that order (>= 0, finite: GuideRate::get and its phase conversion
 * are opm-common's, the converted values stay with the caller), and `available` (WGRUPCON item 2; NULL: all 1).  nupcol: the deck's NUPCOL.
 * The arithmetic is wells.py StandardWells(groups=, arithmetic="stated")'s, operation by operation; like every well rate here it is
 * UNVERIFIED against Flow's numbers (the reference tree holds no output of a deck with groups).  With groups in force:
 *   control value 8 (GRUP) exists in opmhip_set_std_wells_state - for an available producer in a group - and opmhip_get_std_wells;
 *   opmhip_std_wells_begin_iteration(iteration), iteration being the reference's iterationIdx, runs BlackoilWellModel::updateWellControls
 *     (wells/BlackoilWellModel_impl.hpp:1239-1287): group data, the groups' check, group data, every well's group check, group data, the
 *     individual check of the wells that did not just switch, group data (the first group data is elided: the groups' check reads the present
 *     rates only, and the NUPCOL copy and the record that pass would leave are overwritten by the second, under the same condition);
 *   group data (BlackoilWellModelGeneric.cpp:1494-1539, WellGroupHelpers.cpp:300-427): while iteration < nupcol the rates of the groups'
 *     producers are copied to the NUPCOL rates; per group and component reduction = 0 - the NUPCOL rates of its producers not under GRUP,
 *     guide_sum = the mode's guide rates of its producers under GRUP, rates = 0 - the present rates of its producers, voidage = the sum of
 *     their voidage rates (calcReservoirVoidageRates; groups with a RESV target), every sum over the group's wells in list order starting
 *     from 0.  This record stays as it is until the next group data: the wells' checks and the control rows read it frozen;
 *   the group's check (BlackoilWellModelGeneric.cpp:537-650, 888-943) runs only while iteration <= nupcol (the asymmetry with the copy's <
 *     is the reference's): ORAT, WRAT, GRAT, LRAT, RESV in that order, the first target that is < current and is not the mode in force
 *     wins; current from the present rates (LRAT: the oil sum + the water sum; RESV: the voidage sum); on a switch the rates of the group's
 *     wells under GRUP are multiplied by target / current when current > 1e-12 (updateWellRatesFromGroupTargetScale, WellGroupHelpers.cpp:429-);
 *   a well's group check (WellInterfaceFluidSystem.cpp:363-432, WellGroupHelpers.cpp:1055-1180) - a producer not under GRUP, available, in a
 *     group whose mode is not NONE: mode(v) = v[c] (ORAT, WRAT, GRAT), v_o + v_w (LRAT), (c_w v_w + c_o v_o) + c_g v_g with the well's calcCoeff
 *     (RESV; TargetCalculator::calcModeRateFromRates, TargetCalculator.cpp:53-90); current = -mode(x); fraction = g_w / (guide_sum + g_w), 0
 *     where that sum is <= 1e-12; target_rate = max(1e-12, ((target - mode(reduction)) + current) * fraction); where current > target_rate
 *     the control becomes 8 and the three rates are multiplied by target_rate / current;
 *   the control row under 8 (WellInterfaceEval.cpp:178-266): target_rate = max(0, (target - mode(reduction)) * (g_w / guide_sum)), the
 *     fraction 0 where guide_sum <= 1e-12; r_w[3] = mode(x) + target_rate with D[3] the mode's derivatives (the rows of controls 3 .. 7 with
 *     target_rate in the limit's place); a group of mode NONE gives the BHP row bhp - bhp_limit (:189-221);
 *   a well leaves control 8 only through its individual limits, by the rule it had;
 *   opmhip_std_wells_begin_iteration(0) forms the averages and calcCoeff for every producer of a group with a RESV target, and the group
 *     data before the wells alone are solved; during that solve the record is frozen, as the reference's group state is;
 *   opmhip_advance_time_level / opmhip_update_failed save and restore the groups' modes and the NUPCOL rates with the controls.
 * A list without groups launches exactly the kernels it launched before.  With groups a begin_iteration launches the group kernel in front of
 * and behind the controls (and, at iteration 0, in front of the wells-alone solve): a number that depends neither on the wells nor on the groups.
 * KNOWN DIFFERENCE FROM FLOW: updateWellStateWithTarget's second rescaling on a switch to GRUP (wells/WellInterface_impl.hpp:902-921) is left
 * out, as the rescaling is for every other mode here.
 * The averages and calcCoeff are formed at opmhip_std_wells_begin_iteration(0) only.  A group's first RESV target handed in by
 * opmhip_set_std_wells_group_targets, and opmhip_set_std_wells_limits called with groups in force (the coefficients then move to the limits'
 * array, which starts from zeros), therefore take effect at the next time step's first iteration: until then the voidage rates and RESV rows
 * are evaluated at zero averages and coefficients.  Both calls are events of a report or time step, in front of begin_iteration(0).
 * The NUPCOL rates are the library's own: opmhip_get_std_wells_groups reads them, no entry point sets them.
 * NOT covered: nested groups and a control on FIELD (updateGroupHigherControls); group guide rates; group and well efficiency factors (all 1);
 * GCONINJE (RATE / RESV / REIN / VREP); GCONSALE / GCONSUMP; exceed actions other than RATE; CRAT / PRBL; injectors in a group's arithmetic
 * (an injector may name a group and is ignored by it); well potentials; decomposed contexts (refused as the list itself is). */
typedef struct opmhip_std_wells_groups {
    int num_groups;
    const int* well_group;         /* [num_wells] the well's group, -1: directly under FIELD */
    const double* oil_target;      /* [num_groups] each; +infinity: no such target; NULL: none of that kind */
    const double* water_target;
    const double* gas_target;
    const double* liquid_target;
    const double* resv_target;
    const int* mode;               /* [num_groups] 0 NONE, 1 ORAT, 2 WRAT, 3 GRAT, 4 LRAT, 5 RESV; NULL: all NONE */
    const double* guide_rate;      /* [num_wells * 5] per well ORAT, WRAT, GRAT, LRAT, RESV */
    const int* available;          /* [num_wells] 0 / 1; NULL: all 1 */
    int nupcol;
} opmhip_std_wells_groups;
/* Call it after opmhip_set_std_wells; NULL (or num_groups == 0) clears; replacing or clearing the list clears.  OPMHIP_NOT_READY without
 * a list; OPMHIP_INVALID_ARGUMENT, the text naming the reason, for: a decomposed context (checked first); num_groups < 0; a NULL well_group or guide_rate; a group index outside
 * [-1, num_groups); a target that is NaN, -infinity or not > 0; a mode outside 0 .. 5 or one whose target the group lacks; a guide rate that
 * is negative or not finite; an available other than 0 / 1; nupcol < 0; a well under control 8 that is an injector, has no group or is not
 * available; removing the groups while a well is under control 8.  A refused call leaves the previous values in force.  The NUPCOL rates
 * start from zero. */
int opmhip_set_std_wells_groups(opmhip_ctx* ctx, const opmhip_std_wells_groups* groups);
/* Events at a report or time step, with groups in force (OPMHIP_NOT_READY otherwise): new guide rates [num_wells * 5]; new targets
 * (a NULL array: that kind stays) and modes (NULL: stay).  Checked as above; a refused call leaves the previous values in force.  Both wait
 * for the stream and mark the last assembly stale, as opmhip_set_std_wells_state does. */
int opmhip_set_std_wells_guide_rates(opmhip_ctx* ctx, const double* guide_rate);
int opmhip_set_std_wells_group_targets(opmhip_ctx* ctx, const double* oil_target, const double* water_target, const double* gas_target,
                                       const double* liquid_target, const double* resv_target, const int* mode);
/* Per group, as the last group data left them (any pointer may be NULL; waits for the stream): mode [num_groups], rates [num_groups * 3]
 * (oil, water, gas produced), voidage [num_groups], reduction [num_groups * 3], guide_sum [num_groups]; per well nupcol_rates
 * [num_wells * 3].  Nothing is written without groups. */
int opmhip_get_std_wells_groups(opmhip_ctx* ctx, int* mode, double* rates, double* voidage, double* reduction, double* guide_sum, double* nupcol_rates);

/* With a list set:
 * opmhip_assemble forms, in front of the assembly kernel and of the aquifers' influx (the host order: wells' rates first), the
 * perforation rates with their five derivatives, r_w, D, D^-1, B and C (computePerfRate, assembleWellEqWithoutIteration:
 * StandardWell_impl.hpp:195-420, 516-640) and adds the rates of every distinct perforated cell, in perforation order, to its rows of
 * the source arrays (computeTotalRatesForDof, BlackoilWellModel_impl.hpp:496-512); behind the assembly kernel the caller's rows are
 * put back.  It stays a pure function of the device state: the controls change in opmhip_std_wells_begin_iteration only.  A well
 * none of whose completions flows keeps its bottom-hole pressure (its control row becomes bhp-update = 0).  A D that meets a zero
 * pivot sets a flag on the device; the next opmhip_get_std_wells or opmhip_solve_system reports OPMHIP_INVALID_ARGUMENT (well and
 * column are named) and the list is cleared - its D^-1 is stored as zeros, never as NaNs.
 * opmhip_solve_system(wells = NULL) takes the resident B / C / D^-1 as its operator form; a host list with num_wells > 0 is
 * refused by every call that takes one (the operator would be applied twice); OPMHIP_NOT_READY before the first assemble.
 * opmhip_advance_time_level / opmhip_update_failed also save / restore the well unknowns and the controls (control 2, THP, included).
 * Two wells in one cell: the new kernels add in perforation order, but the existing operator kernels (y -= C^T D^-1 B x, r -= C^T D^-1
 * r_w) add two wells' contributions to a shared cell atomically, in either order - with a host list as with the resident one.  A run
 * with such a cell is therefore not reproducible to the bit from run to run, nor against the host path; every other run is.
 * With no list set, no existing call launches, copies or decides anything else than before. */

/* replaces: model().linearizer().linearizeDomain() (flow/BlackoilModelEbos.hpp:424), then .jacobian() /
 * .residual() (:339-340, :526-527).  iteration == 0 also (re)fills the cached old-time-level storage term
 * (recycleFirstIterationStorage, ebos/eclproblem.hh:1758-1765).  Jacobian and residual stay on the device for
 * opmhip_solve_system(vals = NULL, b = NULL); jac (nnzb*9) / residual (Nb*3) are optional host copies in natural
 * order. */
int opmhip_assemble(opmhip_ctx* ctx, double dt, int iteration, double* jac, double* residual);

/* cached intensive quantities, for parity tests: per cell 17 fields x (value, d/dSw, d/dp, d/dX):
 * S_w S_o S_g | p_w p_o p_g | b_w b_o b_g | mob_w mob_o mob_g | rho_w rho_o rho_g | Rs | porosity
 * With a PVTG or ROCKTAB fluid the record has 19 fields: ... | Rs | Rv | transmissibility multiplier | porosity
 * (opmhip_iq_fields tells which). */
int opmhip_iq_fields(opmhip_ctx* ctx);
int opmhip_get_iq(opmhip_ctx* ctx, double* out);
/* the records of `n` cells (natural local ids, any order, repeats allowed), out[n * fields * 4]: what a well model reads per Newton
 * iteration - BlackoilWellModel::updatePerforationIntensiveQuantities evaluates the perforated cells only
 * (wells/BlackoilWellModel_impl.hpp:1606-1630) - gathered on the device, so that the copy is 544 bytes per perforation.  ABI 11 */
int opmhip_get_iq_cells(opmhip_ctx* ctx, int n, const int* cells, double* out);

/* replaces: BlackoilModelEbos::localConvergenceData + computeCnvErrorPv + the CNV/MB formulas of
 * getReservoirConvergence (flow/BlackoilModelEbos.hpp:628-904).  out[17]: R_sum[3], maxCoeff[3], B_avg[3], pvSum,
 * cnvErrorPv, CNV[3], MB[3]; component order oil, water, gas. */
int opmhip_convergence(opmhip_ctx* ctx, double dt, double tol_cnv, double* out);

/* replaces: RateConverter::SurfaceToReservoirVoidage::defineState (wells/RateConverter.hpp:433-554) for the one region Flow's well model
 * uses (every cell in region 0, wells/BlackoilWellModel_impl.hpp:206-208, 460): the averages the surface-to-reservoir conversion of a
 * RESV limit is evaluated at, from the intensive quantities of the state now present.  Per cell pv_cell = V * porosity (the record's,
 * at the cell's pressure), hpv = pv_cell * (1 - S_w); sums of hpv, p_o hpv, Rs hpv, Rv hpv over the cells with hpv > 0, the same with
 * pv_cell over the cells with pv_cell > 0 (Rv = 0 in the 17-field record).  out[5] = pressure, rs, rv, pv, weights: the hydrocarbon
 * sums divided by sum hpv where that is > 0 (weights = 1.0, pv = sum hpv), otherwise the pore-volume sums divided by sum pv_cell
 * (weights = 0.0, pv = sum pv_cell).  Two kernels on the context's stream, no floating-point atomics: the same state gives the same
 * bits from call to call; the call waits for the stream to read the result back.
 * OPMHIP_NOT_READY before set_state; OPMHIP_INVALID_ARGUMENT for out == NULL, for a decomposed context (comm.sum over the ranks is
 * not part of this) and for a field whose pore volume is not > 0 (nothing is divided; out stays untouched).  Additive to ABI 11 */
int opmhip_reservoir_averages(opmhip_ctx* ctx, double* out);

/* ---- fluids in place and region pressures per FIP region, reduced on the device.  Additive to ABI 11 ---------------------------
 * The fluid-in-place report Flow forms at every report step (ebos/ecloutputblackoilmodule.hh:610-697 updateFluidInPlace_;
 * ebos/eclgenericoutputblackoilmodule.cc:712-737 regionSum, :1240-1250 pressureAverage_, :1412-1571 update / makeRegionSum /
 * accumulateRegionSums / updateSummaryRegionValues), from the cached intensive quantities, the cell volumes and the reference porosity
 * of opmhip_set_static - all in HBM already - instead of a copy of every record (opmhip_get_iq) and a loop on the host.
 * Per cell twelve terms, values only, in this order (the OPMHIP_FIP_* slots) and with these statements:
 *    0 DynamicPoreVolume      pv = volume * porosity(record)
 *    1 PoreVolume             volume * reference porosity
 *    2 HydroCarbonPV          pv * hc,  hc = S_o + S_g   (not 1 - S_w)
 *    3 PressurePV             p_o * pv
 *    4 PressureHydroCarbonPV  PressurePV * hc
 *    5 OilInLiquidPhase       fip_o = (b_o * S_o) * pv
 *    6 GasInGasPhase          fip_g = (b_g * S_g) * pv
 *    7 GasInLiquidPhase       Rs * fip_o
 *    8 OilInGasPhase          Rv * fip_g   (Rv = 0 in the 17-field record)
 *    9 WATER                  (b_w * S_w) * pv
 *   10 OIL                    fip_o + OilInGasPhase
 *   11 GAS                    fip_g + GasInLiquidPhase
 * Per region the twelve sums over its cells; cells with an id <= 0 belong to no region and are left out everywhere, field totals
 * included (regionSum, :724-727).  The sums use no floating-point atomics and have ONE stated order, which depends on the region
 * array and the natural cell numbering alone (not on the context's ordering, a launch's grid or the call): a region's cells by
 * ascending natural index, cut into chunks of 256 consecutive items (a missing item of the last chunk counts as 0.0); in a chunk
 * lane l of one wavefront forms (((0.0 + x[l]) + x[l + 64]) + x[l + 128]) + x[l + 192], the 64 lanes are combined by the tree
 * v[l] += v[l + o], o = 32, 16, ..., 1; the chunk results of a region, ascending, form a new list under the same rule until one
 * value is left.  (The reference adds in cell order; the two differ by rounding.)  Field totals: the regions' totals added from 0.0
 * in ascending id, as `update` does (:1420-1426).  An id in 1 .. max that no cell carries gives zeros.
 * A row of results has OPMHIP_FIP_ROW = 14 doubles: the twelve sums, then pressureAverage_ with hydrocarbon = true (RPR / FPR) and
 * with hydrocarbon = false (RPRP / FPRP): hydrocarbon && HydroCarbonPV > 1e-10 ? PressureHydroCarbonPV / HydroCarbonPV :
 * PressurePV / PoreVolume.  A region or field without pore volume gives the reference's 0.0 / 0.0, a NaN, and no status.
 * UNVERIFIED: Inplace::add(phase, sum) is opm-common's and not in the reference tree - whether Flow's field value accumulates over
 * several region sets cannot be read there.  Here every set has field totals of its own, and set 0's are "the field's".
 * NOT covered: decomposed contexts (the region sums are comm.sums over the ranks, :733-734), the text layout of the report
 * (outputRegionFluidInPlace_) and unit conversion - the caller's -, inter-region flows (the reference at this version has none). */
#define OPMHIP_FIP_MAX_SETS 16
#define OPMHIP_FIP_TERMS 12
#define OPMHIP_FIP_ROW 14
/* replaces: createLocalRegion_ / regionMax and the region arrays of EclGenericOutputBlackoilModule (regions_, :1405-1410).
 * region[s][cell], s < num_sets, Nb ids each in the natural cell order; set 0 is FIPNUM.  num_sets = 0 releases everything.  The host
 * builds per set the list of its cells by (id, natural index) and the chunk descriptors of every level, and uploads them.
 * OPMHIP_NOT_READY before set_static.  OPMHIP_INVALID_ARGUMENT with a text, before anything is uploaded and with the sets in force
 * untouched: a NULL array, num_sets outside 0 .. OPMHIP_FIP_MAX_SETS, a largest id above Nb, a decomposed context (the sums over
 * the ranks are not formed). */
int opmhip_set_fip_regions(opmhip_ctx* ctx, int num_sets, const int* const* region);
/* replaces: the element loop of EclWriter::evalSummaryState over updateFluidInPlace_, accumulateRegionSums and the pressure part of
 * updateSummaryRegionValues, for one set, from the state now present.  regions[max_id * OPMHIP_FIP_ROW] (row r - 1 = region r; nullable),
 * field[OPMHIP_FIP_ROW] (nullable).  One launch for the per-cell terms, one per level of the reduction, one for the totals; the call
 * waits for the stream to read (max_id + 1) * 12 doubles back.  The same state gives the same bits from call to call and in every
 * ordering of the context.  The first evaluation of a set after opmhip_set_fip_regions is kept as its "originally in place", as
 * initialInplace_ is (:1487-1488) - with the flaws the reference's own comment lists: it is the first REPORTED state, not the initial one.
 * OPMHIP_NOT_READY before set_state or before regions are set; OPMHIP_INVALID_ARGUMENT for a set out of range. */
int opmhip_fluid_in_place(opmhip_ctx* ctx, int set, double* regions, double* field);
/* that record (what FOE divides by, :1514-1517); OPMHIP_NOT_READY before the set's first opmhip_fluid_in_place */
int opmhip_get_fluid_in_place_initial(opmhip_ctx* ctx, int set, double* regions, double* field);
/* the per-cell arrays Flow writes to the restart file (ecloutputblackoilmodule.hh:632-637, 666-693) at the state now present:
 * out[slot * Nb + cell], natural cell order.  Needs regions to be set (the arrays are allocated with them). */
int opmhip_get_fluid_in_place_cells(opmhip_ctx* ctx, double* out);
/* info[4]: the set's largest id, its cells in regions, its chunks at level 0, its levels (launches of the reduction) */
int opmhip_get_fip_info(opmhip_ctx* ctx, int set, int* info);
/* device milliseconds of the last opmhip_fluid_in_place, by HIP events on the context's stream: ms[0] the per-cell terms, ms[1] the
 * reduction's launches and the totals */
int opmhip_get_fip_timings(opmhip_ctx* ctx, double* ms);

/* replaces: BlackoilModelEbos::updateSolution (flow/BlackoilModelEbos.hpp:549-563) = BlackOilNewtonMethod::update_
 * (dp <= 0.3 p, dS <= 0.2, primary-variable switching) + invalidateAndUpdateIntensiveQuantities, preceded by
 * NonlinearSolverEbos::stabilizeNonlinearUpdate "dampen" (flow/NonlinearSolverEbos.hpp:307-353): dx *= relax.
 * dx == NULL uses the solution of the last opmhip_solve_system, which is still on the device.
 * num_switched (nullable) receives the number of cells whose meaning changed. */
int opmhip_update(opmhip_ctx* ctx, const double* dx, double relax, int* num_switched);

/* ---- domain decomposition over the GPUs of a node (restricted additive Schwarz) --------------------------------- */
/* The reference's parallel runs are MPI domain decomposition with block-Jacobi/overlapping ILU0 and halo updates
 * through Dune::OwnerOverlapCopyCommunication (linalg/ISTLSolverEbos.hpp:101-105, 171-178;
 * linalg/ParallelOverlappingILU0.hpp:857-860, 897; flow/BlackoilModelEbos.hpp:599-603); its accelerator back-ends are
 * switched off under MPI (linalg/ISTLSolverEbos.hpp:136-141), so this surface is new.  One process per GPU, one context
 * per process; set_pattern_dd describes the subdomain.  Communication runs on the context's stream with RCCL
 * (ncclSend/ncclRecv per neighbour for halos, ncclAllReduce for the fused scalars).
 *   rank 0: opmhip_comm_unique_id(id) -> broadcast the 128 bytes by any means (MPI_Bcast, torch.distributed, a file)
 *   every rank: opmhip_comm_init_rccl(ctx, nranks, rank, id) ; opmhip_set_halo(...) */
int opmhip_comm_unique_id(char* id128);
int opmhip_comm_init_rccl(opmhip_ctx* ctx, int nranks, int rank, const char* id128);
/* several contexts inside ONE process (each driven by its own host thread, all on one GPU), connected by device copies
 * and a host barrier: test vehicle for the decomposition logic on a single GPU */
int opmhip_comm_init_loopback(opmhip_ctx* ctx, int nranks, int rank, const char* group_name);
/* diagnostics: one RCCL all-reduce of {1 + rank, 2} on the context's stream; sum_out[2] */
int opmhip_comm_selftest(opmhip_ctx* ctx, double* sum_out);
/* what the communicator itself reports: info[0] = ncclCommCount, [1] = ncclCommUserRank, [2] = ncclCommCuDevice (the HIP
 * device RCCL bound this rank to), [3] = kind (0 none, 1 loopback, 2 RCCL).  Loopback / no communicator: the context's own
 * numbers.  bench.py prints them so that a multi-GPU record shows how many ranks RCCL actually connected. */
int opmhip_comm_info(opmhip_ctx* ctx, int* info4);
/* optional, before opmhip_set_static: the global id of every local cell (Nb + Nghost entries).  The assembly then adds a
 * row's face fluxes in ascending GLOBAL neighbour order, i.e. exactly the sum an undecomposed run forms, so that
 * residual and Jacobian do not depend on the decomposition down to the last bit. */
int opmhip_set_cell_global_ids(opmhip_ctx* ctx, const long long* gids);
/* halo description: for neighbour q (rank neigh_rank[q]) the owned cells send_cells[send_ptr[q] .. send_ptr[q+1])
 * (local natural ids, in the order the neighbour numbers its ghosts) are sent, and ghost cells
 * Nb + recv_ptr[q] .. Nb + recv_ptr[q+1] are received.  global_cells = number of cells of the whole grid (B_avg is a
 * mean over all cells, flow/BlackoilModelEbos.hpp:722-727). */
int opmhip_set_halo(opmhip_ctx* ctx, long long global_cells, int nneigh, const int* neigh_rank, const int* send_ptr,
                    const int* send_cells, const int* recv_ptr);

/* ---- measurement -------------------------------------------------------------------------------------------- */
/* Device-side timing per kernel class with HIP events recorded on the context's own stream, so that bench.py can
 * state the average launch duration of a kernel over its timed region (the reference prints the same split at
 * verbosity >= 3/4: bda/cusparseSolverBackend.cu:303-308, bda/openclSolverBackend.cpp:451-459).
 * classes: 0 SpMV, 1 ILU0 apply (all sweeps of one M^-1; with the line-coloured ordering the first sweep also carries
 * the BiCGStab p- / (r, x)-update), 2 ILU0 factorisation, 3 the remaining BiCGStab vector / reduction kernels (one
 * scope between two operator applications), 4 assembly kernel, 5 intensive-quantity update, 6 convergence, 7 the pressure
 * AMG cycle of CPR, 8 decomposed runs: the second launch of an operator application (the boundary tiles, multiplied after
 * the halo exchange that ran beside the interior tiles of class 0).
 * Communication spans of decomposed runs (ABI 8; they OVERLAP the kernel classes - a halo exchange runs beside class 0, an
 * all-reduce inside class 3 - and are what the reference's back-ends have no counterpart for, being single-process): 9 one halo
 * exchange, pack -> send / receive -> ghosts in place, on the stream it runs on (Dune's copyOwnerToAll in front of the operator,
 * linalg/ParallelOverlappingILU0.hpp:897, WellOperators.hpp:127-138); 10 one global reduction, local sums' kernel -> all-reduce ->
 * result on the device (BiCGStab's scalar products; the convergence sums of BlackoilModelEbos.hpp:599-603); 11 CPR across the ranks:
 * the all-gather of the joined level's right-hand side plus the cycle every rank runs on it. */
#define OPMHIP_PROF_CLASSES 12
/* on = 0: off; 1: every scope; k > 1: the linear-solver classes (0, 1, 3) are recorded in every k-th solve_system call
 * only - an event record costs a few microseconds of bubble on the stream and a BiCGStab iteration holds seven of
 * them.  Also resets the accumulated numbers. */
int opmhip_profile_enable(opmhip_ctx* ctx, int on);
/* waits for the stream, folds all pending event pairs in, returns launches and total milliseconds of one class */
int opmhip_profile_get(opmhip_ctx* ctx, int cls, long long* launches, double* total_ms);

#ifdef __cplusplus
}
#endif
#endif /* OPMHIP_H */
