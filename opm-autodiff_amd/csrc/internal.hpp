// libopmhip internals: context, device buffers, error plumbing.  Product code — never includes oracle/.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <climits>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/opmhip.h"
#include "cpr_setup.hpp"
#include "vfp_tables.hpp"
#include "source_lists.hpp"
#include "ms_wells_setup.hpp"

namespace opmhip {

constexpr int BS = 3;
constexpr int BB = 9;

// ---- tiling constants (see DESIGN.md "tile kernels") -------------------------------------------------
// One workgroup = one wavefront (64 lanes) = one tile of at most TILE_ROWS block rows, one row per lane.
// A tile's blocks are streamed into LDS with coalesced 16-byte loads, then each lane walks its own row in
// the CPU's sequential order.  TILE_CAP_BLOCKS bounds the LDS image (72 B per block + 4 B column).
#ifndef OPMHIP_TILE_ROWS
#define OPMHIP_TILE_ROWS 32
#endif
constexpr int TILE_ROWS = OPMHIP_TILE_ROWS;
constexpr int TILE_CAP_BLOCKS = 7 * TILE_ROWS;  // a full tile of a Cartesian 7-point stencil
// ---- what reorder.cpp builds and the kernels of solver.hip read: the limits both sides go by ----
constexpr int CHAIN_MAX_STEPS = 128;       // steps of a chain-tile (its descriptor record lives in LDS)
constexpr int STENCIL_ROW_ENTRIES = 8;     // the stencil form (StencilForm): 4-bit table indices in a row's word = entries of a row
constexpr int STENCIL_MAX_OFFSETS = 15;    // ... offsets in a tile's table; the index 15 says "no entry"
constexpr int STENCIL_TABLE_SLOTS = 16;    // ... numbers a tile's table takes in StencilForm::table
constexpr int STENCIL_MAX_KOFF = 255;      // ... a row's first entry behind its tile's first entry (one byte)
constexpr int DESC_HEAD = 4;               // descriptor record of a chain kernel's launch position (TileSet::ctDesc): numbers in front of its three lists
constexpr int desc_stride(int S1) { return 4 * ((DESC_HEAD + 3 * S1 + 3) / 4); }   // ... its size with three lists of S1 numbers, a multiple of 16 bytes

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    template <class T> T* as() const { return static_cast<T*>(p); }
};

// Stencil form of a block-CSR's index streams (reorder.cpp: encode_stencil): the rows of a tile share their column offsets, so a tile carries
// a table of <= 15 offsets (col - row) and a row one word of eight 4-bit table indices (15 = no entry) and one byte (first entry - the
// tile's first entry) - 5 bytes per row instead of 28 + 16 for column indices and row bounds.  Read by k_spmv_pipe_st and the chain sweeps.
struct StencilForm {
    std::vector<unsigned> word;        // per row
    std::vector<unsigned char> koff;   // per row
    std::vector<int> table;            // [16 * tiles]
    unsigned* d_word = nullptr;
    unsigned char* d_koff = nullptr;
    int* d_table = nullptr;
};
// the form of one tile (reorder.cpp): reset_stencil sizes it for Nb rows and `tables` tables (every word 15s, every table 0s); encode_stencil
// writes rows [r0, r1) of a block-CSR with their offsets in table `slot`.  False where the tile has more than 15 offsets (nothing written) or a
// row more than 8 entries or a first entry more than 255 blocks in (the table and the rows before that one are written): the form does not fit.
void reset_stencil(StencilForm& S, int Nb, size_t tables);
bool encode_stencil(const std::vector<int>& rowptr, const std::vector<int>& col, int r0, int r1, int slot, StencilForm& S);

struct TileSet {            // tiles over one block-CSR row-pointer array, never crossing a colour boundary
    std::vector<int> row0;  // [ntiles+1]
    std::vector<int> colorTile;  // [numColors+1] first tile of each colour
    std::vector<int> ctFirst;    // [nChainTiles+1] first sub-tile of each chain-tile (steps of <= TILE_ROWS chains)
    std::vector<int> colorCT;    // [numColors+1] first chain-tile of each colour
    // launch schedules (reorder.cpp: build_schedules): position -> work item, dealt so that position % 8 (= the XCD a
    // workgroup lands on) walks through one spatial stretch of the grid at a time
    std::vector<int> spmvSched;  // [4 * nsched] (r0, r1, rowptr[r0], rowptr[r1]) of every SpMV launch position; r1 <= r0 = padding
    int nsched = 0;
    // decomposed runs: positions [0, nschedInt) hold the INTERIOR tiles (no row of theirs has a ghost column: they can be
    // multiplied while the halo exchange is under way), [nschedInt, nsched) the boundary tiles; else nschedInt == nsched
    int nschedInt = 0;
    std::vector<int> ctSched;    // per colour, padded to a multiple of 8: chain-tile of every launch position or -1
    std::vector<int> ctSchedOff; // [numColors+1] offsets into ctSched
    int* d_row0 = nullptr;
    int* d_ctFirst = nullptr;
    // per schedule position of the chain kernels: [steps, chain-tile, -, -, first row of step 0..steps, first L entry of
    // those rows, first U entry of those rows], descS1 numbers each, record stride descStride (solver.hip: load_desc)
    std::vector<int> ctDesc;
    int descStride = 0, descS1 = 0;
    int* d_spmvSched = nullptr;
    // stencil form of the SpMV's index streams, one table per launch position.  stencil = false: a tile needs more than 15 offsets or a
    // row more than eight entries; the explicit index streams are used
    bool stencil = false;           // some part of the schedule has it
    bool stencilPart[2] = {false, false};   // [0] positions [0, nschedInt), [1] the boundary tiles of a decomposed run
    StencilForm st;
    int* d_ctSched = nullptr;
    int* d_ctDesc = nullptr;
    int ntiles() const { return (int)row0.size() - 1; }
};

// Launch schedule of the "rest product" (Pattern::ualias): the tiles of y = R x + s u over the block-CSR of the matrix entries that are NOT
// in the factor's U part - lower entries, diagonal, ghost columns.  Same record formats as the SpMV's (TileSet::spmvSched and a stencil form
// with one table per launch position, read by k_spmv_pipe_st); tiles hold up to 64 rows (one per lane) and TILE_CAP_BLOCKS blocks.
struct RestSched : StencilForm {
    bool on = false;
    int nsched = 0, nschedInt = 0;            // launch positions; [0, nschedInt) interior tiles, the rest boundary tiles (decomposed runs)
    std::vector<int> sched;                   // [4 * nsched] (r0, r1, rrowptr[r0], rrowptr[r1]); r1 <= r0 = padding
    int* d_sched = nullptr;
};

struct Pattern {
    int Nb = 0, nnzb = 0, numColors = 0, nl = 0, nu = 0;  // Nb = owned block rows
    int Nghost = 0, Nloc = 0;                            // ghost cells numbered Nb..Nloc-1 (vectors have Nloc entries)
    int maxRowBlocks = 0;                                // longest row, in blocks
    bool chained = false;  // line colouring: rows of one colour may depend on earlier rows of their own chain
    int kindInForce = 0, chainLen = 0;  // the opmhip_reorder the pattern was ordered with (OPMHIP_REORDER_AUTO resolved) and its rows per chain (0: no chains)
    // per colour: every row's L (U) part is at most the row's own chain predecessor (successor) - the sweep is then a
    // lane-private recurrence and runs in the light kernel (no LDS staging, deep prefetch)
    std::vector<char> lightL, lightU;
    // natural order (as handed over)
    std::vector<int> nat_rowptr, nat_col;
    // ordering
    std::vector<int> toOrder, fromOrder, colorPrefix;  // colorPrefix[numColors+1] in rows
    // internal (reordered) pattern
    std::vector<int> rowptr, col, diag, nnzMap;  // nnzMap[k_internal] = k_natural
    std::vector<int> lrowptr, lcol, urowptr, ucol;   // the factors' L / U split (ILU(n): of the filled pattern, see fillLevel)
    std::vector<long long> gids;  // optional: global id of every local cell (decomposed runs), natural local order
    TileSet tiles;
    // device copies
    int *d_rowptr = nullptr, *d_col = nullptr, *d_diag = nullptr, *d_nnzMap = nullptr;
    int *d_toOrder = nullptr, *d_fromOrder = nullptr;
    int *d_lrowptr = nullptr, *d_lcol = nullptr, *d_urowptr = nullptr, *d_ucol = nullptr;
    std::vector<int> fdest;      // per matrix entry: where the factorisation puts it - L index (>= 0), -2 - U index, -1 (diagonal / dropped ghost column)
    int* d_fdest = nullptr;
    // stencil form of the sweeps' index streams (solver.hip: SweepStencil), per factor part (L, U), one table per tile of `tiles`;
    // sweepStencil = false: some tile needs more than 15 offsets or a row more than CGCH entries - explicit streams
    bool sweepStencil = false;
    StencilForm sw[2];
    // per L entry (i, j) what its elimination step touches: the ONE entry of row i that meets the U part of row j (a 7-point grid has no
    // triangles: it is the diagonal) as U index * 64 + offset of the target in row i; -1: none; -2: several (the general search)
    std::vector<int> lmatch;
    int* d_lmatch = nullptr;
    // "U is upper(A)": no elimination step of the block ILU0 touches an entry right of the diagonal (linalg/ParallelOverlappingILU0.hpp:466-481
    // modifies A_ik only where (i,j), (j,k) and (i,k) all exist: on a pattern without triangles that is k == i alone), so the factor's U part
    // equals the matrix's own upper part bit for bit and the backward sweep's row sums u_i = sum_{j>i} U_ij x_j ARE the upper part of A x.
    // The product that follows an M^-1 application inside BiCGStab then needs only the REST of the matrix (lower entries, diagonal, ghost
    // columns): y_i = sum_rest A_ik x_k + u_i.  rrowptr / rcol: that rest as a block-CSR of its own, ascending columns; rdest: per matrix entry
    // its place there or -1; its values (d_R in the context) are written by the factorisation from the rows it has staged.
    bool ualias = false;
    int nr = 0;
    std::vector<int> rrowptr, rcol, rdest;
    int *d_rdest = nullptr, *d_rrowptr = nullptr;
    RestSched rest;
    // ILU(n), n >= 1 (opmhip_set_ilu_fillin_level; reorder.cpp: build_fill_split): lrowptr / lcol / urowptr / ucol / fdest / nl / nu describe
    // the factors' own pattern - the matrix's owned pattern plus the level-of-fill entries, computed in the ordering's elimination order; fill
    // entries start at zero.  The ordering is then a schedule of the FILLED pattern: colours (levels) are its independent sets, colorPrefix
    // their row ranges.  ftiles: the sweeps' tiles over the filled rows (row0 / colorTile / d_row0 only; `tiles` still cuts the SpMV).
    // lmatch and the chain kernels' records (TileSet::ctDesc) belong to ILU0 and are not built; ualias is false.
    int fillLevel = 0;
    std::vector<int> fillBase;   // natural row -> its place in the elimination order the fill was computed in (tests: the fill rule restated)
    TileSet ftiles;
};
// ILU(n) memory guard: the filled factors (L, U and the diagonal, in blocks) may hold at most this many times the blocks of the matrix
constexpr int ILUN_BUDGET_FACTOR = 8;

// Multisegment wells in their device-resident form (opmhip_set_ms_wells): a list that stays until it is replaced or cleared, beside the
// per-solve WellsDev.  Per well one descriptor (MsWellDesc, MsTreeDesc: ms_wells_setup.hpp).
struct MsWellsDev {
    int num = 0, maxM = 0;
    int form = 0;                // OPMHIP_MS_WELLS_DENSE / _TREE / _AUTO: applies to the lists set after opmhip_set_ms_wells_form
    int num_dense = 0, num_tree = 0;     // the list's wells by form: d_desc holds the dense ones, d_tdesc the others
    int tree_max_seg = 0, tree_max_depth = 0;
    size_t tree_bytes = 0;       // of `bytes`: the tree wells' blocks
    int tree_lds_doubles = 0;    // dynamic LDS of k_ms_wells_tree_apply for this list (ms_wells_tree_plan)
    bool have_structure = false; // the index arrays on the device belong to h_Mbp ... h_Dnzp
    MsTreeDesc* d_tdesc = nullptr;
    int* d_tint = nullptr;
    double* d_fac = nullptr;
    std::vector<int> h_form;     // per well of the list: 0 dense, 1 tree
    bool atomic = false;         // some cell is shared between two blocks of the list: y is updated by atomic adds
    bool flag_pending = false;   // an inversion was enqueued whose pivot flags have not been looked at yet
    int factorisations = 0;
    size_t bytes = 0;            // device memory held
    MsWellDesc* d_desc = nullptr;
    int *d_Brows = nullptr, *d_cell = nullptr, *d_blkrow = nullptr, *d_Dcolp = nullptr, *d_Drows = nullptr, *d_flag = nullptr;
    double *d_B = nullptr, *d_C = nullptr, *d_Dvals = nullptr, *d_inv = nullptr;
    int* h_flag = nullptr;       // pinned, one int per well: 0, or 1 + the column (dense form) / the segment (tree form) whose pivot was zero
    size_t cap_flag = 0;
    // the list as handed over last time (natural cell numbers): what arrives unchanged is not copied again
    std::vector<int> h_Mbp, h_Brows, h_blkp, h_Bcols, h_Dcolp, h_Drows, h_Dnzp;
    std::vector<double> h_Bvals, h_Cvals, h_Dvals;
};

// Standard wells resident on the device (opmhip_set_std_wells): the well equations of wells.py's StandardWells, formed by kernels
// into WellsDev's d_B / d_C / d_D (= D^-1) / d_val_pointers / d_Ccols / d_Bcols, which the existing operator kernels then read.
// d_pack, one array so that a Newton iteration reads back once: x [4 num] | control [num] (0.0 rate, 1.0 bhp) | r_w [4 num] |
// flag [num] (0.0, or 1 + the column whose pivot was zero; sticky until the host has looked).  d_saved: x | control of the last
// opmhip_advance_time_level.  h_wi / h_wd: what d_wi / d_wd hold.
constexpr int SW_X = 0, SW_CONTROL = 4, SW_RW = 5, SW_FLAG = 9, SW_PACK = 10;   // where d_pack's fields begin and its length, in doubles per well
constexpr int SW_SAVED = SW_RW;                                                 // d_saved's length: the fields in front of r_w
// The list's features, one part each: its flags, its host copies and its device arrays.  A part is a plain aggregate whose device
// arrays are named ONCE, in each_dev; dev_part_release and dev_part_install (below, beside dev_free) free, discard and install by that
// list.  Nothing here owns memory: every array is registered in opmhip_ctx::allocs, which opmhip_destroy frees wholesale.
// The heads from the well-bore density (opmhip_set_std_wells_head_model).  d_state: per perforation p_perf | q_o | q_w | q_g (4 nperf
// doubles, field-major), d_saved its copy of the last opmhip_advance_time_level; d_out: density | p_avg | mixture (5 nperf, the
// mixture 3 per perforation); d_scratch: 8 doubles per perforation for the two dependent passes of wells that do not fit the LDS
struct SwWellboreDev {
    bool on = false;
    bool state_set = false, state_saved = false;   // p_perf has been taken from the cells (or handed in); ... at the last advance_time_level
    bool initialised_saved = false;                // StdWellsDev::initialised at the last advance_time_level: under this model the bottom-hole pressure is an input of the heads, so a given-up first step goes back to 'not yet set'
    double *d_depth = nullptr, *d_ref = nullptr, *d_state = nullptr, *d_saved = nullptr, *d_out = nullptr, *d_scratch = nullptr;
    int* d_pref = nullptr;       // per well: the preferred phase
    template <class F> void each_dev(F f) { f(&d_depth); f(&d_ref); f(&d_state); f(&d_saved); f(&d_out); f(&d_scratch); f(&d_pref); }
};
// Crossflow in producers (opmhip_set_std_wells_crossflow): on only while some well of the list has the switch; d_allow: per well 0 / 1,
// d_dq: per perforation d rate_c / d q_j of the last assemble (9 doubles)
struct SwCrossflowDev {
    bool on = false;
    int* d_allow = nullptr;
    double* d_dq = nullptr;
    template <class F> void each_dev(F f) { f(&d_allow); f(&d_dq); }
};
// Vaporised oil in the rate model (opmhip_set_std_wells_vaporised_oil): d_sol: per well the dissolved gas [num] | the vaporised oil
// [num] of the last assemble; allocated while the switch is on
struct SwVaporisedOilDev {
    bool on = false;
    double* d_sol = nullptr;
    template <class F> void each_dev(F f) { f(&d_sol); }
};
// THP limits (opmhip_set_std_wells_thp): on only while some well of the list has one.  d_table: per well the index of its VFP table
// (-1: no limit), h_table its host copy; d_wd: per well limit, alq, dh; d_out: thp of the last controls | dp of this time step |
// V - dp of the last assemble (3 num doubles, field-major)
struct SwThpDev {
    bool on = false;
    std::vector<int> h_table;
    int* d_table = nullptr;
    double *d_wd = nullptr, *d_out = nullptr;
    template <class F> void each_dev(F f) { f(&d_table); f(&d_wd); f(&d_out); }
};
// Further rate limits (opmhip_set_std_wells_limits): on only while some well of the list has one (or use_list_target = 0).  d_lim: per
// well oil, water, gas, liquid, resv (+infinity: none), h_lim its host copy; d_use / h_use: per well use_list_target; d_out:
// coeff [3 num] | resv_current [num] | the averages the coefficients were formed at [5]; resv: some well has a RESV limit
struct SwLimitsDev {
    bool on = false, resv = false;
    std::vector<double> h_lim;
    std::vector<int> h_use;
    double *d_lim = nullptr, *d_out = nullptr;
    int* d_use = nullptr;
    template <class F> void each_dev(F f) { f(&d_lim); f(&d_use); f(&d_out); }
};
// The matrix-add form (opmhip_set_std_wells_matrix_add): d_target [targets]: the distinct blocks of the device's block-CSR the pairs
// write; d_tptr [targets + 1] / d_contrib [3 pairs]: per block its contributions (well, a, b) in the order of the host path; h_*: what
// they hold.  (Whether the wells ARE in the matrix is a fact about the matrix, not about this part: StdWellsDev::in_matrix.)
struct SwMatrixAddDev {
    bool on = false;
    int targets = 0, pairs = 0;
    int *d_target = nullptr, *d_tptr = nullptr, *d_contrib = nullptr;
    std::vector<int> h_target, h_tptr, h_contrib;
    template <class F> void each_dev(F f) { f(&d_target); f(&d_tptr); f(&d_contrib); }
};
// Group production control (opmhip_set_std_wells_groups): on only while groups are in force.  d_ptr [num + 1] / d_idx: per group its
// producers, wells ascending; d_of / d_avail / d_resv: per well its group (-1: none), available, a producer in a group with a RESV
// target; d_guide: 5 per well; d_target: 5 per group; d_state: mode [num] | NUPCOL rates [3 wells], d_saved its copy of the last
// opmhip_advance_time_level; d_rec: per group rates [3], voidage, reduction [3], guide_sum of the last group data; d_out: what
// SwLimitsDev::d_out holds (coeff | resv_current | averages), for a list without further limits; h: the host's copy
struct SwGroupsDev {
    bool on = false, resv = false;
    int num = 0, nupcol = 0;
    int *d_ptr = nullptr, *d_idx = nullptr, *d_of = nullptr, *d_avail = nullptr, *d_resv = nullptr;
    double *d_guide = nullptr, *d_target = nullptr, *d_state = nullptr, *d_saved = nullptr, *d_rec = nullptr, *d_out = nullptr;
    StdWellsGroupsLists h;
    template <class F> void each_dev(F f) {
        f(&d_ptr); f(&d_idx); f(&d_of); f(&d_avail); f(&d_resv); f(&d_guide); f(&d_target); f(&d_state); f(&d_saved); f(&d_rec); f(&d_out);
    }
};
struct StdWellsDev {
    int num = 0, nperf = 0, nd = 0;
    bool initialised = false;    // the first begin_iteration(0) has set the bottom-hole pressures
    bool assembled = false;      // B, C, D^-1, r_w belong to the well unknowns now present
    int* d_wi = nullptr;         // per well: producer, injected phase, rate component
    double* d_wd = nullptr;      // per well: rate target, bhp limit
    std::vector<int> h_wi;
    std::vector<double> h_wd;
    double *d_tw = nullptr, *d_dz = nullptr, *d_head = nullptr, *d_pr = nullptr;   // per perforation; d_pr: 15 doubles, [component][value, d/dSw, d/dp, d/dX, d/dbhp]
    double *d_pack = nullptr, *d_saved = nullptr, *d_Dmat = nullptr;
    int *d_cpos = nullptr, *d_cptr = nullptr, *d_cperf = nullptr;   // distinct perforated cells: position, range into d_cperf, their perforations in perforation order
    double* d_save = nullptr;    // per distinct cell: the caller's 3 source and 9 dsource entries
    std::vector<double> h_flag;  // opmhip_solve_system: the flags' copy, queued in front of the synchronisation it does anyway
    std::vector<int> h_vp, h_pos;   // the list's ranges and the internal positions of its perforated cells (the matrix-add schedule is built from them)
    bool in_matrix = false;      // opmhip_std_wells_add_to_matrix has run since the last assemble - the solve then installs no operator form
    SwWellboreDev wb;
    SwCrossflowDev cf;
    SwVaporisedOilDev vo;
    SwThpDev thp;
    SwLimitsDev lim;
    SwMatrixAddDev ma;
    SwGroupsDev grp;
    double* x() const { return d_pack + (size_t)SW_X * num; }
    double* control() const { return d_pack + (size_t)SW_CONTROL * num; }
    double* rw() const { return d_pack + (size_t)SW_RW * num; }
    double* flag() const { return d_pack + (size_t)SW_FLAG * num; }
};

struct WellsDev {
    StdWellsDev sw;
    int num_wells = 0, nperf = 0;
    int *d_val_pointers = nullptr, *d_Ccols = nullptr, *d_Bcols = nullptr;
    double *d_C = nullptr, *d_D = nullptr, *d_B = nullptr;
    double *d_res = nullptr, *d_xw = nullptr;   // 4 doubles per well each (residual in, well solution out)
    // decomposed runs, wells whose perforations lie in several subdomains (opmhip_wells.distributed): every rank holds the list, B x is
    // summed over the ranks (wells/WellHelpers.hpp:68-123)
    bool distributed = false;
    double* d_bx = nullptr;   // 4 doubles per well: this rank's part of B x, then the sum
    size_t cap_wells = 0, cap_perf = 0;
    // what the device arrays hold, as handed over last time: a Newton iteration passes the same list three times (residual, solve, well
    // solution) and the perforated cells never change - an array that arrives unchanged is not copied again (upload_wells_local)
    std::vector<int> h_vp, h_cc, h_bc;
    std::vector<double> h_D, h_C, h_B;
    // multisegment wells: applied on the host between the product and the standard wells (opmhip_wells.ms_apply)
    int num_ms = 0;
    opmhip_ms_apply_fn ms_apply = nullptr;
    void* ms_user = nullptr;
    double *h_x = nullptr, *h_y = nullptr;   // pinned, Nb * 3 doubles each, natural order
    MsWellsDev ms;   // ... or on the device, in the same place (opmhip_set_ms_wells)
    bool any() const { return num_wells > 0 || num_ms > 0 || ms.num > 0; }
};
// The resident standard wells in operator form - B, C, D^-1 as the last assemble formed them, read by the wells kernels of the solver -
// for as long as this lives: the form is set per call, none is left behind for later products
struct StdWellsOperatorForm {
    WellsDev& W;
    explicit StdWellsOperatorForm(WellsDev& w) : W(w) { W.num_wells = W.sw.num; W.nperf = W.sw.nperf; W.distributed = false; }
    ~StdWellsOperatorForm() { W.num_wells = 0; }
    StdWellsOperatorForm(const StdWellsOperatorForm&) = delete;
    StdWellsOperatorForm& operator=(const StdWellsOperatorForm&) = delete;
};

// The intensive-quantity record (fluid_device.hpp): fields of value + 3 derivatives, the first of each group; phases, equations, gravity
enum { F_S = 0, F_P = 3, F_B = 6, F_MOB = 9, F_RHO = 12, F_RS = 15 };
enum { WATER = 0, OIL = 1, GAS = 2 };
enum { EQ_OIL = 0, EQ_WATER = 1, EQ_GAS = 2 };
constexpr double GRAVITY = 9.80665;

// Analytic aquifers on the device (opmhip_set_aquifers).  nc connections (aquifers concatenated, Carter-Tracy first), nd distinct connected
// cells.  Per aquifer: AQ_PAR constants, AQ_STEP scalars of the time step under way (host-computed, opmhip_aquifers_begin_time_step), AQ_STATE
// state doubles that live from time step to time step.
enum { AQ_TYPE = 0, AQ_TC, AQ_RHOW, AQ_DATUM, AQ_PA0, AQ_BETA, AQ_PI, AQ_CV, AQ_PAR };   // AQ_CV = total_compr * initial_watvolume
enum { AQ_TD = 0, AQ_PITD, AQ_PITDPRIME, AQ_COEF, AQ_STEP };                            // Carter-Tracy: td, PI(td + dt), PI'(td + dt); Fetkovich: coef
enum { AQ_WFLUX = 0, AQ_AUX, AQ_STATE };                                                // AQ_AUX: fluxValue_ (Carter-Tracy) / aquifer_pressure_ (Fetkovich)
struct AquifersDev {
    int num = 0, nc = 0, nd = 0;
    bool stepped = false;       // an opmhip_aquifers_begin_time_step has been seen
    double step_dt = 0.0;
    std::vector<int> h_ptr, h_id, h_tabptr;
    std::vector<double> h_par, h_td, h_pd;
    int *d_ptr = nullptr, *d_of = nullptr, *d_pos = nullptr;          // [num + 1]; per connection: its aquifer, its cell (internal position)
    double *d_alpha = nullptr, *d_pprev = nullptr, *d_q = nullptr;    // per connection: alphai_, pressure_previous_, Qai_ (value + 3 derivatives)
    double *d_par = nullptr, *d_step = nullptr, *d_state = nullptr;
    int *d_cpos = nullptr, *d_cptr = nullptr, *d_cconn = nullptr;     // distinct cells: position, range into d_cconn, their connections in aquifer order
    double* d_save = nullptr;                                         // per distinct cell: the caller's source water row and its three derivatives
    double* h_step = nullptr;                                         // pinned staging of d_step
    hipEvent_t ev_step = nullptr;                                     // "h_step has been read"
    template <class F> void each_dev(F f) {
        f(&d_ptr); f(&d_of); f(&d_pos); f(&d_alpha); f(&d_pprev); f(&d_q); f(&d_par); f(&d_step); f(&d_state); f(&d_cpos); f(&d_cptr); f(&d_cconn); f(&d_save);
    }
};

// Open boundaries on the device (opmhip_set_boundary_conditions; kernels: boundary.hip, entry points: capi_boundary.cpp, host set-up:
// boundary_setup.hpp).  nf faces, nd distinct boundary cells, nfc of them with a FREE face.  Per face BC_GEO doubles (area,
// transmissibility, depth of the face centre) and the RATE faces' three rates; per distinct cell with a FREE face one captured
// exterior record of BC_EXT doubles: p, rho, mobility, 1/B of the three phases, Rs, Rv.
enum { BC_AREA = 0, BC_TRANS, BC_DEPTH, BC_GEO };
enum { BX_P = 0, BX_RHO = 3, BX_MOB = 6, BX_B = 9, BX_RS = 12, BX_RV = 13, BC_EXT = 14 };
constexpr int BC_Q = 12;   // a face's residual contribution: three equations and their 3 x 3 derivative
struct BoundaryDev {
    int nf = 0, nd = 0, nfc = 0;
    int *d_type = nullptr;                                            // per face
    double *d_geo = nullptr, *d_rate = nullptr, *d_q = nullptr;       // per face: BC_GEO, 3, BC_Q
    int *d_cpos = nullptr, *d_cptr = nullptr, *d_cconn = nullptr;     // distinct cells: position, range into d_cconn, their faces in list order
    int *d_slot = nullptr, *d_fcell = nullptr;                        // per distinct cell: its exterior record or -1; per record: its distinct cell
    double *d_ext = nullptr, *d_save = nullptr;                       // [nfc * BC_EXT]; per distinct cell: the caller's source row and dsource block
    template <class F> void each_dev(F f) {
        f(&d_type); f(&d_geo); f(&d_rate); f(&d_q); f(&d_cpos); f(&d_cptr); f(&d_cconn); f(&d_slot); f(&d_fcell); f(&d_ext); f(&d_save);
    }
};

// Passive tracers on the device (opmhip_set_tracers; kernels and the solve: tracers.hip, entry points: capi_tracers.cpp, host set-up:
// tracers_setup.hpp).  One batch per phase; a batch's per-cell arrays are interleaved [cell][tracer of the batch], internal cell order.
// The matrix, the factors and the solver's vectors are shared by the batches (they are solved one after the other) and sized for the
// largest one.
constexpr int TRACER_PHASES = 3;
struct TracerMembers { int g[OPMHIP_TRACERS_MAX_PER_PHASE]; };   // a batch's tracers by their number in the caller's list (kernel argument)
struct TracerBatchDev {
    int nt = 0;
    TracerMembers members{};
    double *d_c = nullptr, *d_c0 = nullptr, *d_s1 = nullptr;   // concentration_, concentrationInitial_, storageOfTimeIndex1_
    template <class F> void each_dev(F f) { f(&d_c); f(&d_c0); f(&d_s1); }
};
struct TracersDev {
    int num = 0, maxnt = 0;
    bool begun = false;          // an opmhip_tracers_begin_time_step has been seen
    double tol = 1e-2;           // eclgenerictracermodel.cc:256-262
    int maxit = 100;
    std::vector<int> phase, slot;   // per tracer: its batch, its place there
    TracerBatchDev b[TRACER_PHASES];
    // the sweeps' schedule: rows of level l = d_lvrows[lvptr[l] .. lvptr[l + 1]); d_ford: per row its entries in ascending natural column order
    std::vector<int> lvptr;
    int *d_lvrows = nullptr, *d_ford = nullptr, *d_flag = nullptr;
    double *d_M = nullptr, *d_LU = nullptr, *d_invd = nullptr;                  // [nnzb], [nnzb], [Nb]
    double *d_res = nullptr, *d_x = nullptr, *d_r = nullptr, *d_rw = nullptr, *d_p = nullptr, *d_v = nullptr, *d_s = nullptr, *d_t = nullptr,
           *d_y = nullptr, *d_pw = nullptr;                                     // [Nb * maxnt]
    double *d_sc = nullptr, *d_part = nullptr;                                  // per-tracer BiCGStab scalars; the reductions' partial sums
    int nblk = 0, cellsPerBlock = 0;                                            // first stage of a reduction: workgroups, cells of each
    double *h_rec = nullptr, *d_rec = nullptr;                                  // pinned: tracers done, -, -, sequence number (written last); the same through the device's eyes
    double seq = 0.0;
    // connections (opmhip_set_tracer_connections): grouped by distinct cell as the aquifers' are
    int nconn = 0, nd = 0;
    int *d_cpos = nullptr, *d_cptr = nullptr, *d_cconn = nullptr;
    double *d_rate = nullptr, *d_inj = nullptr;                                 // [3 nconn], [num * nconn]
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    double ms[3] = {0.0, 0.0, 0.0};
    int launches = 0;
    template <class F> void each_conn(F f) { f(&d_cpos); f(&d_cptr); f(&d_cconn); f(&d_rate); f(&d_inj); }
    template <class F> void each_dev(F f) {
        f(&d_lvrows); f(&d_ford); f(&d_flag); f(&d_M); f(&d_LU); f(&d_invd); f(&d_res); f(&d_x); f(&d_r); f(&d_rw); f(&d_p); f(&d_v); f(&d_s); f(&d_t);
        f(&d_y); f(&d_pw); f(&d_sc); f(&d_part);
    }
};

// Fluids in place per FIP region (opmhip_set_fip_regions; kernels: fip.hip, entry points: capi_fip.cpp, host set-up: fip_setup.hpp).
// The twelve per-cell terms and region sums, in the order of the reference's statements (include/opmhip.h "fluids in place")
enum { FIP_DYNAMIC_PV = 0, FIP_PORE_VOLUME, FIP_HC_PV, FIP_PRESSURE_PV, FIP_PRESSURE_HC_PV, FIP_OIL_IN_LIQUID, FIP_GAS_IN_GAS, FIP_GAS_IN_LIQUID,
       FIP_OIL_IN_GAS, FIP_WATER, FIP_OIL, FIP_GAS, FIP_TERMS };
static_assert(FIP_TERMS == OPMHIP_FIP_TERMS && FIP_TERMS + 2 == OPMHIP_FIP_ROW, "the header's row of results");
// One region set: its plan's arrays on the device (FipPlan: items, chunk descriptors, the regions' result slots), the plan's numbers,
// and the first evaluation's rows ((max_id + 1) x OPMHIP_FIP_ROW, the field's last)
struct FipSetDev {
    int max_id = 0, ncells = 0, npart = 0;
    std::vector<int> level_ptr;
    int *d_items = nullptr, *d_desc = nullptr, *d_result = nullptr;
    std::vector<double> initial;
    template <class F> void each_dev(F f) { f(&d_items); f(&d_desc); f(&d_result); }
};
// d_terms [FIP_TERMS][Nloc] field-major, internal cell order; d_part [FIP_TERMS][npart] the chunk results of the set under way, d_out
// [(max_id + 1)][FIP_TERMS] its regions' and field's sums - both sized for the largest set
struct FipDev {
    std::vector<FipSetDev> sets;
    int npart = 0, max_id = 0;
    double *d_terms = nullptr, *d_part = nullptr, *d_out = nullptr;
    bool timed = false;          // the events of AsmDev::fip_ev belong to a finished opmhip_fluid_in_place
    template <class F> void each_dev(F f) {
        for (FipSetDev& s : sets) s.each_dev(f);
        f(&d_terms); f(&d_part); f(&d_out);
    }
};

// VFP tables (opmhip_set_vfp_tables): the packed host form (vfp_tables.hpp) and its two device arrays, resident for the context's life
// (a part as the standard wells' are: its device arrays named once, in each_dev)
struct VfpDev {
    VfpPacked h;
    int* d_desc = nullptr;
    double* d_dbl = nullptr;
    template <class F> void each_dev(F f) { f(&d_desc); f(&d_dbl); }
};

// opmhip_reservoir_averages (assemble.hip, k_resv_avg_part / k_resv_avg_final): the first stage runs cdiv(cells, 256) workgroups of 256 lanes,
// at most RESV_MAX_PARTS (beyond that its lanes stride over the grid); the one workgroup of the final stage has RESV_FINAL_THREADS lanes,
// so more than RESV_FINAL_THREADS x 256 cells take a second pass over the partials
constexpr int RESV_MAX_PARTS = 1024, RESV_FINAL_THREADS = 256, RESV_OUT = 6;

// assembly-side device state (all per-cell / per-entry arrays in the INTERNAL order)
struct AsmDev {
    AquifersDev aq;
    BoundaryDev bc;
    TracersDev tr;
    VfpDev vfp;
    FipDev fip;
    hipEvent_t fip_ev[3] = {nullptr, nullptr, nullptr};   // opmhip_fluid_in_place: start, the per-cell terms done, the totals done (created with the first regions)
    bool fluid_set = false, static_set = false, state_set = false, assembled = false;
    double *d_tab_dbl = nullptr;
    int* d_tab_idx = nullptr;
    int tab_ndbl = 0, tab_nidx = 0;   // lengths of the two table blobs
    double rock_pref = 1e5, rock_cr = 0.0;
    int num_pvt = 0, num_sat = 0, num_rock = 0, rock_desc = 0;
    bool wet_gas = false;   // PVTG: vaporised oil, third primary-variable meaning
    bool ext = false;       // extended intensive-quantity record (wet gas and / or ROCKTAB): 19 fields instead of 17
    double *d_rvmax = nullptr, *d_overburden = nullptr;   // per cell: DRVDT cap, overburden pressure (optional)
    int* d_rocknum = nullptr;                             // per cell rock-table index (optional)
    bool pc_scaling = false;                              // the fluid allows a per-cell end point of pcow (PCW / SWATINIT)
    double* d_pcw = nullptr;                              // per cell: scaled maximum of the oil-water capillary pressure (optional)
    double* d_eps = nullptr;                              // per cell scaled saturation end points, field-major [EPS_COUNT][Nloc] (optional)
    int epscfg = 0;                                       // packed EclEpsConfig (assemble.hip CellStatic::epscfg)
    std::vector<double> sat_eps;                          // host copy: the tables' own end points, EPS_COUNT per saturation region
    // DRSDT / DRVDT bookkeeping (EclProblem::lastRs_ / lastRv_ / maxDRs_ / maxDRv_) and ROCKCOMP IRREVERS (minOilPressure_)
    bool drsdt_on = false, drvdt_on = false;
    double *d_drsdt = nullptr, *d_drvdt = nullptr;        // rates per PVT region [1/s], negative = none
    int* d_drsdt_all = nullptr;                           // per PVT region: the limit binds all cells (OILVAP option)
    double *d_lastRs = nullptr, *d_lastRv = nullptr;      // per cell
    double* d_minpo = nullptr;                            // per cell minimum oil pressure so far (irreversible compaction); NULL = reversible
    double* d_maxso = nullptr;                            // per cell largest oil saturation at the start of a time step (VAPPARS); NULL = not in force
    double vap1 = 0.0, vap2 = 0.0;                        // VAPPARS exponents: on RvSat, on RsSat
    double *d_maxsw = nullptr, *d_sw0 = nullptr;          // water-induced compaction: largest S_w at the start of a time step, initial S_w; NULL = off
    // relative-permeability hysteresis (SATOPTS HYSTER; EHYSTR item 2 = hyst_model 0 | 1, -1 = off): turning points and shifts
    // [4][Nloc], imbibition region per cell, scaled end points of the imbibition curves [EPS_COUNT][Nloc] (optional)
    int hyst_model = -1;
    double* d_hyst = nullptr;
    int* d_imbnum = nullptr;
    double* d_eps_imb = nullptr;
    double* d_rc = nullptr;                               // relativeChange: 2 x 256 partial sums + (delta, denominator)
    double* d_resv = nullptr;                             // opmhip_reservoir_averages: RESV_MAX_PARTS x 8 partial sums + the 6 results (allocated at the first call)
    int num_wc = 0, h_rocknum_max = -1;                   // water-compaction tables; largest rock-table index handed in (-1: none)
    int* d_wcdesc = nullptr;                              // per table {np, nsw, pressure at, S_w at, pore-volume multipliers at, transmissibility multipliers at | -1}
    double* d_wcdata = nullptr;
    bool storage_frozen = false;                          // begin_time_step formed the old time level's storage: iteration 0 must not refill it
    double* d_invb = nullptr;                             // packed 1/b per cell and phase (Nloc x 3), for the convergence check
    double *d_trans = nullptr, *d_area = nullptr, *d_thpres = nullptr;                      // per entry
    double *d_poro = nullptr, *d_volume = nullptr, *d_depth = nullptr, *d_rsmax = nullptr;  // per cell
    int *d_pvtnum = nullptr, *d_satnum = nullptr;
    double *d_pv = nullptr, *d_iq = nullptr, *d_storageOld = nullptr, *d_source = nullptr, *d_dsource = nullptr;
    unsigned char *d_meaning = nullptr, *d_wasSwitched = nullptr, *d_stage_u8 = nullptr;
    int last_iteration = -1;                // Newton iteration index of the last opmhip_assemble (--cpr-reuse-setup=1)
    double last_dt = 0.0;                   // time step of the last opmhip_assemble (true-IMPES weights scale the storage term by V / dt)
    double* d_drift = nullptr;              // residual * dt of the last accepted time step (drift compensation), Nloc x 3
    bool drift_enabled = true;              // EclEnableDriftCompensation defaults to true (ebos/eclproblem.hh:496-498)
    double max_compensation = 0.1;          // 10 * NewtonTolerance (ebos/eclproblem.hh:352-356, 1854)
    double* d_pv_prev = nullptr;            // solution(1): primary variables at the start of the time step
    unsigned char* d_meaning_prev = nullptr;
    bool prev_set = false;
    int* d_nswitched = nullptr;
    int* d_asm_sched = nullptr;            // per workgroup of k_assemble: first row, end row, first entry, end entry of its tile
    int* d_asm_desc = nullptr;             // per workgroup and lane: column and entry word (row inside the tile, upwind tie-break flag, natural summation order, place in the rest / U stream)
    bool split_ok = false;                 // every entry word carries its block's place in the tile's run of the rest or the U stream (ILU0 patterns without ghost columns)
    int ntiles = 0, nsched = 0;
    double *d_conv_part = nullptr, *d_conv_out = nullptr;
    double* d_stage_cell = nullptr;   // staging for per-cell doubles (natural order), Nb * max(9, IQS)
    int* d_cell_pos = nullptr;        // opmhip_get_iq_cells / opmhip_set_source_cells: internal positions of the cells named, grown on demand
    size_t cell_pos_cap = 0;
    double* d_stage_entry = nullptr;  // staging for per-entry doubles (natural order), nnzb
};

// domain decomposition: communicator + halo lists (comm.hip)
enum CommKind { COMM_NONE = 0, COMM_LOOPBACK = 1, COMM_RCCL = 2 };
struct CommDev {
    int kind = COMM_NONE, nranks = 1, rank = 0;
    void* nccl = nullptr;    // ncclComm_t
    void* group = nullptr;   // LoopGroup*
    long long global_cells = 0;
    bool halo_set = false;
    int nneigh = 0;
    std::vector<int> neigh, send_ptr, recv_ptr;  // per neighbour: rank, send range (into d_send_idx), ghost range
    int* d_send_idx = nullptr;                   // owned cells (internal positions) to send, grouped by neighbour
    double* d_sendbuf = nullptr;                 // 3 doubles per send cell
    unsigned char* d_sendbuf_u8 = nullptr;
    double* d_red = nullptr;                     // 16 doubles: all-reduce buffer
    // the halo exchange in front of an operator application runs on a stream of its own, beside the product of the interior
    // tiles: ev_x = "the input vector is complete" (main stream), ev_h = "ghost entries are in place" (halo stream)
    hipStream_t hstream = nullptr;
    hipEvent_t ev_x = nullptr, ev_h = nullptr;
    double* halo_vec = nullptr;                  // loopback: the vector whose exchange comm_halo_end still has to drive
    const double* ag_send = nullptr;             // loopback: this rank's contribution to the all-gather under way
    bool reduce_span_open = false;               // a caller of comm_allreduce times the reduction itself (its local sums included)
};

// CPR preconditioner (cpr.hip): pressure-AMG hierarchy, level 0 = the block pattern with scalar values
struct CprLevelDev {
    int n = 0, nnz = 0, nc = 0, W = 0;                              // W: longest row = width of the ELL image
    bool rm = false;                                                // row-major image [i * W + j] (coarse levels, lane groups per row) instead of [j * n + i]
    int *d_ecol = nullptr, *d_rlen = nullptr, *d_diag = nullptr;    // ELL columns [W x n], row lengths, ELL position of the diagonal
    int* d_cpos = nullptr;                                          // ELL position (next level) of every coarse entry
    double *d_val = nullptr, *d_dinv = nullptr, *d_x2 = nullptr;    // ELL values [W x n]
    int *d_agg = nullptr, *d_mptr = nullptr, *d_midx = nullptr;   // node -> aggregate, members of every aggregate
    int* d_mem4 = nullptr;                                         // members of every aggregate as four ints (-1: none), NULL if an aggregate has more: the coarse level then forms its right-hand side itself
    int *d_gptr = nullptr, *d_gidx = nullptr;                      // Galerkin gather lists for the next level's entries
    double *d_b = nullptr, *d_x = nullptr, *d_r = nullptr;         // level vectors
    // level 0 of a single domain on a regular pattern: the ELL columns in stencil form (cpr.hip: EllStencil) - per row a word of 4-bit indices
    // into the table of <= 15 column offsets its aligned group of 32 rows shares; NULL: the explicit column image d_ecol is read
    unsigned* d_sword = nullptr;
    int* d_stable = nullptr;
    // ILU0 smoothing (opmhip_config.cpr_amg_ilu_levels; cpr_setup.hpp: CprIluHost): scalar factors in the level's own image (strict lower = L,
    // diagonal = 1 / U_ii, strict upper = U), per row the words that say which slots are lower / upper entries in the level's elimination
    // order, the lower slots in the order the factorisation visits them, and a launch schedule: colour by colour, one thread per SEQUENCE
    // of rows that depend on each other inside the colour (level 0 of a line-coloured pattern: the chains; otherwise single rows)
    bool ilu = false;
    int iluMW = 0, iluWL = 0, iluWU = 0;                           // mask words per kind, lower / upper entries per row at most
    double *d_fval = nullptr, *d_t = nullptr;
    double *d_ilv = nullptr, *d_iuv = nullptr, *d_iud = nullptr;   // what the sweeps read: lower entries [iluWL][n], upper entries [iluWU][n], 1 / U_ii
    int *d_ilc = nullptr, *d_iuc = nullptr;                        // their columns (-1: none)
    bool iluSimple = false;                                        // no elimination step touches anything but a diagonal: k_cpr_ilu_factor_simple
    int* d_tpos = nullptr;                                         // simple levels: per lower entry the place of the transposed entry in the level's image
    std::vector<int> iluWl, iluWu;                                 // per colour: lower / upper entries per row at most
    unsigned* d_imask = nullptr;                                   // [2 * iluMW][n]: lower words, then upper words
    unsigned char* d_lorder = nullptr;                             // [iluWL][n], 255 = none
    int* d_rowAt = nullptr;                                        // per colour [steps][sequences]: row or -1
    std::vector<int> iluNseq, iluNsteps, iluOff;                   // per colour
    std::vector<char> iluFast;                                     // per colour: same-colour couplings are the sequence's neighbours only (register forwarding)
};
struct CprAsyncJob;   // cpr.hip: a structure being built on a host thread (--cpr-reuse-setup=2 with cpr_async_setup)
struct CprDev;
// Decomposed runs (opmhip_config.cpr_gather_rows): the LAST level of a rank's own hierarchy is not solved by the rank - its right-hand
// sides are gathered over the ranks, every rank runs the rest of the cycle on the joined system (`glob`: a hierarchy of its own whose
// level 0 is the joined level, the couplings between the subdomains included) and takes its slice of the result (cpr.hip: cpr_gather_*)
struct CprGatherDev {
    bool on = false;
    int nloc = 0, off = 0, NG = 0, maxn = 0;                       // my rows of the joined level, where they start, its size, the largest slice
    int nnzloc = 0, maxnnz = 0, nnzG = 0;                          // the same for its entries
    double *d_recv = nullptr, *d_vsend = nullptr, *d_vrecv = nullptr;   // gathered right-hand sides [nranks x maxn]; my entries' values, everybody's [nranks x maxnnz]
    int* d_cagg = nullptr;                                         // aggregate (on my last level) of every owned cell
    double* d_send = nullptr;                                      // my slice of the joined level's right-hand side [maxn]
    int *d_unpad = nullptr, *d_vunpad = nullptr, *d_vpos = nullptr;    // joined row -> place in d_recv; joined entry -> place in d_vrecv and in level 0's image of `glob`
    int *d_src = nullptr, *d_xptr = nullptr, *d_xidx = nullptr;    // my entries: place in my last level's image, or (-1 - q) the q-th coupling between subdomains = sum over d_apg[d_xidx[d_xptr[q] ..)]
    int nq = 0;                                                    // fine couplings to ghost cells
    int *d_qrow = nullptr, *d_qentry = nullptr;                    // their row and block-matrix entry
    double* d_apg = nullptr;                                       // their pressure values (k_cpr_ghost_pvals)
    std::shared_ptr<CprDev> glob;
};
struct CprDev {
    bool structured = false, coarse_direct = true;
    bool level0 = false;                                           // level 0's image (it belongs to the pattern) is on the device
    std::shared_ptr<CprAsyncJob> job;
    bool recreate = false;                                         // opmhip_cpr_recreate: the next cpr_update builds the structure anew
    std::vector<CprLevelDev> lv;
    double *d_w = nullptr, *d_lu = nullptr;
    double* d_pcol = nullptr;                                      // level 0: the pressure column of every block, ELL, component-major [3][W x Nb]
    bool w_given = false;                                          // d_w holds weights handed in (opmhip_set_cpr_weights): not recomputed
    double *d_r = nullptr, *d_y = nullptr, *d_z = nullptr;         // fine-level block vectors
    double omega = 2.0 / 3.0, damp = 1.6, beta = 0.25;             // Jacobi damping, prolongation damping, strength threshold
    CprGatherDev gather;
    int apply_rc = 0;                                              // first failure of a collective inside an application (the BiCGStab driver looks at it)
    bool pvals_fresh = false;                                      // the factorisation of this solve left weights and level 0's values behind (FactorRider): cpr_update skips its own pass
};
// What the block ILU0 factorisation does for the CPR on its way through the matrix (k_ilu_factor's rider): every row is in LDS, fixed up,
// before its elimination starts - the pressure-column image of its blocks and its entries of the pressure matrix
// a_p[k] = sum_r A_k[r][p] w_row[r] (PressureTransferPolicy::calculateCoarseEntries, PressureTransferPolicy.hpp:116-139) are written from
// there (k_cpr_pvals' statements on the same values: the same bits) instead of by a second pass over the Jacobian.
struct FactorRider {
    int mode = 0;                 // 0: none; 1: weights read from w (true-IMPES or handed in); 2: quasi-IMPES weights formed from the row's diagonal block (k_cpr_weights' statements) and stored to w
    double* w = nullptr;          // [Nb x 3]
    double* ap = nullptr;         // level 0's ELL values [W x Nb]
    double* pcol = nullptr;       // pressure columns, component-major [3][W x Nb]
    int W = 0;
    int ghostFrom = INT_MAX;      // columns >= this are left out (a subdomain's own pressure system): value 0
};

// per-kernel-class device timing with HIP events on the context's stream (opmhip_profile_*)
enum ProfClass { PROF_SPMV = 0, PROF_ILU_APPLY, PROF_ILU_FACTOR, PROF_VECTOR, PROF_ASSEMBLE, PROF_IQ_UPDATE, PROF_CONVERGENCE, PROF_CPR_AMG,
                 PROF_SPMV_BOUNDARY,   // decomposed runs: the second launch of a product (boundary tiles, after the halo exchange)
                 // communication spans of decomposed runs (prof_span_*): event pairs on the stream the step runs on, outside the chain of
                 // the kernel scopes above and overlapping them - the per-phase timers of the reference's back-ends
                 // (bda/cusparseSolverBackend.cu:303-308, 412-417; bda/openclSolverBackend.cpp:451-459) for what it has no kernels for
                 PROF_HALO,            // one halo exchange: pack -> send / receive -> the ghosts are in (copyOwnerToAll, ParallelOverlappingILU0.hpp:897), on the stream it runs on
                 PROF_ALLREDUCE,       // one global reduction: the local sums' kernel -> the all-reduce -> its result on the device (the sums behind BlackoilModelEbos.hpp:599-603 and the scalar products of BiCGStab)
                 PROF_CPR_GATHER,      // CPR across the ranks: the all-gather of the joined level's right-hand side and the cycle every rank runs on it
                 PROF_COUNT };
struct Profiler {
    bool enabled = false;
    int every = 1;                            // solver scopes are recorded in every `every`-th linear solve (1 = all)
    long solve_no = 0;
    bool suspended = false;                   // inside a linear solve that is not sampled
    std::vector<hipEvent_t> ev;               // event pool, allocated on demand
    size_t ev_used = 0;
    std::vector<int> cls, e0, e1;             // per scope: class (-1: voided - a speculative launch past the stopping
    size_t used = 0;                          //   point), start and end event
    int pending = -1;                         // scope whose end event is still to be recorded (shared with the next begin)
    bool lazy = false;                        // prof_end leaves the end to the next prof_begin (inside a linear solve)
    int handoff = -1;                         // stop event of a kernel launched with its own events: starts the next scope
    static constexpr size_t CAP = 1 << 15;
    double total_ms[PROF_COUNT] = {0};
    long count[PROF_COUNT] = {0};
};

enum Scal {  // device-resident BiCGStab scalars (double d_scal[SC_COUNT])
    SC_RHO = 0, SC_RHOP, SC_ALPHA, SC_OMEGA, SC_BETA, SC_TMP1, SC_TMP2, SC_NORM, SC_NORM0,
    SC_DONE,   // 1.0 once the stopping rule held: every later kernel of the solve returns at once (speculative launches)
    SC_ZERO,   // never written: the "not done" flag of launches outside a solve
    SC_RR,     // opmhip_config.fused_reductions: r.r carried from half iteration to half iteration
    SC_RHOH,   //   rw.r after the first half (rho - alpha v.rw)
    SC_DONEH,  //   number of the half iteration that met the stopping rule (its own update kernels still run), -1: none
    SC_COUNT = 16
};

}  // namespace opmhip

struct opmhip_ctx {
    opmhip_config cfg;
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    std::string err;
    bool pattern_set = false, system_loaded = false, factored = false, have_result = false;
    int ilu_fillin = 0;                         // opmhip_set_ilu_fillin_level (--ilu-fillin-level); ignored with a CPR preconditioner
    opmhip::Pattern pat;
    // values, internal order
    double *d_A = nullptr, *d_L = nullptr, *d_U = nullptr, *d_invD = nullptr;
    double *d_R = nullptr, *d_usum = nullptr;   // Pattern::ualias: the rest of the matrix beside U (values), the backward sweeps' row sums (3 per row)
    bool half_product = false;                  // BiCGStab forms the product after an ILU0 application from d_R and d_usum (opmhip_config.half_product)
    // Split assembly: k_assemble writes the Jacobian straight into d_R (lower entries, diagonal) and d_U (upper entries), the
    // streams the sweeps and the rest product read, and k_ilu_factor forms L and D^-1 from d_R without copying anything.  d_A is then NOT
    // written: A_stale says so, and whoever reads d_A calls ensure_A first (one gather, counted in split_gathers).
    bool split_asm = false;                     // the context can assemble that way (split_asm_wanted, resolved with half_product)
    bool A_stale = false;                       // the matrix in force lives in d_R / d_U; d_A holds an older one
    long long split_gathers = 0, split_assemblies = 0;
    // vectors, internal order, 3*Nb each
    double *d_b = nullptr, *d_x = nullptr, *d_r = nullptr, *d_rw = nullptr, *d_p = nullptr, *d_v = nullptr,
           *d_s = nullptr, *d_t = nullptr, *d_pw = nullptr, *d_vu = nullptr;
    // staging (natural order): matrix values and one vector
    double *d_stageA = nullptr, *d_stageV = nullptr;
    double* d_scal = nullptr;   // SC_COUNT doubles
    double* d_part = nullptr;   // partial sums: 2 x npart
    double minv_scale = 1.0;    // during a solve: the factor the preconditioned vectors (d_pw, d_s) are still to be multiplied by
    double* d_part2 = nullptr;  // second-level partials: 2 x RED1_BLOCKS
    int npart = 0;
    int last_solve_iterations = 0;   // BiCGStab iterations of the last opmhip_solve_system (--cpr-reuse-setup=2)
    int last_dot_count = 0;     // partial sums the last launch_spmv left in d_part (per list)
    double* h_pinned = nullptr;  // SC_COUNT doubles, pinned
    // read-back ring of the BiCGStab stopping rule: the finalize kernel writes (norm, norm_0, done) of half iteration h
    // straight into pinned host slot h % RB_SLOTS and then, system-scope release, the slot's sequence number, which the
    // host polls (no event, no copy, no stream bubble); the host runs one half iteration ahead of the device
    static constexpr int RB_SLOTS = 4, RB_DOUBLES = 4;   // slot: norm, norm_0, done, sequence number (written last)
    double* h_ring = nullptr;    // pinned, RB_SLOTS x RB_DOUBLES
    double* d_ring = nullptr;    // the same memory through the device's eyes
    double rb_seq = 0.0;         // last sequence number handed to a stopping-rule kernel (exact integers in a double)
    double rb_want[RB_SLOTS] = {0, 0, 0, 0};
    const double* d_done = nullptr;  // flag the tile kernels test first: &d_scal[SC_ZERO] outside a solve, &d_scal[SC_DONE] inside
    opmhip::WellsDev wells;
    opmhip::AsmDev asmb;
    opmhip::CommDev comm;
    opmhip::CprDev cpr;
    opmhip::Profiler prof;
    std::vector<void*> allocs;
    // opmhip_config.pin_host_arrays: host ranges of the caller registered for DMA (first address seen -> hipHostRegister; bytes == 0: refused, not tried again)
    struct HostRange { const void* p; size_t bytes; };
    std::vector<HostRange> pinned;
};

namespace opmhip {

// The library's measurement switches (tools/README.md: two forms that give the same bits, chosen by an environment variable so that a
// change can be judged by alternating runs inside one GPU session) are read only under the master switch OPMHIP_TUNING=1: a stray
// variable in a user's environment changes nothing, and every switch that is in force says so on stderr (once per call site).
inline const char* tuning_env(const char* name) {
    static const bool on = [] { const char* e = std::getenv("OPMHIP_TUNING"); return e && e[0] == '1'; }();
    const char* v = std::getenv(name);
    if (!v) return nullptr;
    if (!on) {
        std::fprintf(stderr, "opmhip: %s is set but OPMHIP_TUNING=1 is not - ignored\n", name);
        return nullptr;
    }
    std::fprintf(stderr, "opmhip: measurement switch %s=%s is in force\n", name, v);
    return v;
}

inline int fail(opmhip_ctx* c, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf;
    return code;
}

#define OPMHIP_HIP(ctx, call)                                                                       \
    do {                                                                                            \
        hipError_t e_ = (call);                                                                     \
        if (e_ != hipSuccess)                                                                       \
            return opmhip::fail(ctx, OPMHIP_DEVICE_ERROR, "%s failed: %s (%s:%d)", #call,           \
                                hipGetErrorString(e_), __FILE__, __LINE__);                         \
    } while (0)

// OPMHIP_POISON_ALLOC=1 (under OPMHIP_TUNING=1; a debugging aid): every floating-point array starts as NaNs, every other array as
// zeros - an entry that is read before it was written then shows in every run instead of in the runs in which hipMalloc hands
// back memory some earlier context left its numbers in
inline bool poison_allocations() {
    static const bool on = [] { const char* e = tuning_env("OPMHIP_POISON_ALLOC"); return e && e[0] == '1'; }();
    return on;
}
template <class T>
int dev_alloc(opmhip_ctx* c, T** p, size_t count) {
    void* q = nullptr;
    size_t bytes = (count ? count : 1) * sizeof(T);
    hipError_t e = hipMalloc(&q, bytes);
    if (e != hipSuccess)
        return fail(c, OPMHIP_DEVICE_ERROR, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
    // (the contexts' streams do not wait for the null stream: the fill is complete before anybody can enqueue a kernel that writes the array)
    if (poison_allocations() && ((e = hipMemset(q, std::is_floating_point<T>::value ? 0xFF : 0x00, bytes)) != hipSuccess || (e = hipDeviceSynchronize()) != hipSuccess)) {
        (void)hipFree(q);
        return fail(c, OPMHIP_DEVICE_ERROR, "hipMemset(%zu) failed: %s", bytes, hipGetErrorString(e));
    }
    c->allocs.push_back(q);
    *p = static_cast<T*>(q);
    return OPMHIP_SUCCESS;
}
// gives one tracked allocation back (buffers that are re-allocated larger: the old one must not pile up until destroy)
template <class T>
void dev_free(opmhip_ctx* c, T** p) {
    if (!*p) return;
    for (size_t i = 0; i < c->allocs.size(); ++i)
        if (c->allocs[i] == (void*)*p) { c->allocs[i] = c->allocs.back(); c->allocs.pop_back(); break; }
    (void)hipFree((void*)*p);
    *p = nullptr;
}
// A part of the device state (SwThpDev, VfpDev, ...: its device arrays are what its each_dev names).  Release: every array given back,
// the part as default-constructed - also how a half-built replacement is discarded.  Install: the part in force released, the
// finished one moved in; a replacement is built apart first, so that a refused call leaves the previous setting in force.
template <class P>
void dev_part_release(opmhip_ctx* c, P& part) {
    part.each_dev([c](auto** p) { dev_free(c, p); });
    part = P();
}
template <class P>
void dev_part_install(opmhip_ctx* c, P& in_force, P& fresh) {
    dev_part_release(c, in_force);
    in_force = std::move(fresh);
}
template <class T>
int dev_upload(opmhip_ctx* c, T** p, const T* h, size_t n) {
    int rc = dev_alloc(c, p, n);
    if (rc) return rc;
    if (n > 0) OPMHIP_HIP(c, hipMemcpy(*p, h, n * sizeof(T), hipMemcpyHostToDevice));
    return OPMHIP_SUCCESS;
}
template <class T>
int dev_upload(opmhip_ctx* c, T** p, const std::vector<T>& h) {
    return dev_upload(c, p, h.data(), h.size());
}
// A list that is handed over again and again (the wells of a Newton iteration): the host keeps a record of what each device array holds, and
// what arrives unchanged is not copied.  record_same: the record holds exactly the caller's n entries.  dev_put_recorded: the caller's
// array to the device and into the record; a failed copy leaves the record empty, so that the next call copies it again.
template <class T>
bool record_same(const std::vector<T>& h, const T* p, size_t n) {
    return h.size() == n && (n == 0 || std::memcmp(h.data(), p, n * sizeof(T)) == 0);
}
template <class T>
int dev_put_recorded(opmhip_ctx* c, T* d, std::vector<T>& h, const T* p, size_t n) {
    h.clear();
    if (n > 0) OPMHIP_HIP(c, hipMemcpy(d, p, n * sizeof(T), hipMemcpyHostToDevice));
    h.assign(p, p + n);
    return OPMHIP_SUCCESS;
}

// RAII-less profiling scope: prof_begin returns a slot (or -1), prof_end closes it.  An event record costs a few
// microseconds of bubble on the stream, so back-to-back scopes share one: prof_end(lazy) leaves the end open and the next
// prof_begin's event closes it (prof_flush closes it where nothing follows).
inline int prof_event(opmhip_ctx* c, hipStream_t s = nullptr) {
    Profiler& P = c->prof;
    if (P.ev.size() <= P.ev_used) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return -1;
        P.ev.push_back(e);
    }
    const int i = (int)P.ev_used++;
    (void)hipEventRecord(P.ev[i], s ? s : c->stream);
    return i;
}
// an event slot without recording it (for hipExtLaunchKernelGGL, which stamps kernel begin / end itself)
inline int prof_event_slot(opmhip_ctx* c) {
    Profiler& P = c->prof;
    if (P.ev.size() <= P.ev_used) {
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return -1;
        P.ev.push_back(e);
    }
    return (int)P.ev_used++;
}
inline void prof_flush(opmhip_ctx* c) {
    Profiler& P = c->prof;
    P.handoff = -1;
    if (P.pending < 0) return;
    const int e = prof_event(c);
    if (e >= 0) P.e1[P.pending] = e; else P.cls[P.pending] = -1;
    P.pending = -1;
}
inline int prof_begin(opmhip_ctx* c, int cls) {
    Profiler& P = c->prof;
    if (!P.enabled || P.suspended || P.used >= Profiler::CAP) { prof_flush(c); return -1; }
    int e;
    if (P.handoff >= 0) { e = P.handoff; P.handoff = -1; }   // the previous kernel's own stop event: no record needed
    else e = prof_event(c);
    if (e < 0) return -1;
    if (P.pending >= 0) { P.e1[P.pending] = e; P.pending = -1; }
    if (P.cls.size() <= P.used) { P.cls.push_back(cls); P.e0.push_back(e); P.e1.push_back(-1); }
    const int slot = (int)P.used++;
    P.cls[slot] = cls; P.e0[slot] = e; P.e1[slot] = -1;
    return slot;
}
// A single kernel timed by its own dispatch (hipExtLaunchKernelGGL start / stop events: no extra packets on the stream,
// kernel-exact like rocprofv3).  Returns false when profiling is off; else es / ee are the event slots to hand to the
// launch.  The start event also closes a pending scope; the stop event will open the next one.
inline bool prof_kernel_scope(opmhip_ctx* c, int cls, int* es, int* ee) {
    Profiler& P = c->prof;
    if (!P.enabled || P.suspended || P.used >= Profiler::CAP) return false;
    *es = prof_event_slot(c);
    *ee = prof_event_slot(c);
    if (*es < 0 || *ee < 0) return false;
    if (P.pending >= 0) { P.e1[P.pending] = *es; P.pending = -1; }
    if (P.cls.size() <= P.used) { P.cls.push_back(cls); P.e0.push_back(*es); P.e1.push_back(*ee); }
    const int slot = (int)P.used++;
    P.cls[slot] = cls; P.e0[slot] = *es; P.e1[slot] = *ee;
    P.handoff = P.lazy ? *ee : -1;
    return true;
}
inline void prof_end(opmhip_ctx* c, int slot) {
    if (slot < 0) return;
    c->prof.pending = slot;
    if (!c->prof.lazy) prof_flush(c);
}
// A span: two events of its own on stream s (default: the context's), independent of the kernel scopes' chain - it may enclose or
// overlap them and may run on the halo stream.  Costs two event records, only in the solves the profiler samples.
inline int prof_span_begin(opmhip_ctx* c, int cls, hipStream_t s = nullptr) {
    Profiler& P = c->prof;
    if (!P.enabled || P.suspended || P.used >= Profiler::CAP) return -1;
    const int e = prof_event(c, s);
    if (e < 0) return -1;
    if (P.cls.size() <= P.used) { P.cls.push_back(cls); P.e0.push_back(e); P.e1.push_back(-1); }
    const int slot = (int)P.used++;
    P.cls[slot] = cls; P.e0[slot] = e; P.e1[slot] = -1;
    return slot;
}
inline void prof_span_end(opmhip_ctx* c, int slot, hipStream_t s = nullptr) {
    if (slot < 0) return;
    const int e = prof_event(c, s);
    if (e >= 0) c->prof.e1[slot] = e; else c->prof.cls[slot] = -1;
}

// reorder.cpp (host): level scheduling / colouring, internal pattern, L/U split, tiles
int build_pattern(opmhip_ctx* c, int Nb, int Nghost, int nnzb, const int* rows, const int* cols);

// kernels.hip launchers (all on c->stream)
void launch_permute_blocks(opmhip_ctx* c, const double* nat, double* internal);
void launch_unpermute_blocks(opmhip_ctx* c, const double* internal, double* nat);  // for lu_out
void launch_vec_to_internal(opmhip_ctx* c, const double* nat, double* internal, int cells = -1);
void launch_vec_to_natural(opmhip_ctx* c, const double* internal, double* nat, int cells = -1);
void launch_zero_diag_fix(opmhip_ctx* c);
// y = A x (+ wells) with the partial sums of ndot scalar products.  exchange: x's ghost entries are brought up to date first
// (copyOwnerToAll) - on the halo stream, beside the product of the interior tiles; x is then written (its ghost part)
int launch_spmv(opmhip_ctx* c, double* x, double* y, int ndot, const double* w0, double xs = 1.0, bool exchange = false, const double* uadd = nullptr, const double* w1 = nullptr);
bool split_asm_wanted(const opmhip_ctx* c);      // solver.hip: half_product in force, ILU0 without CPR, no ghost columns, the assembly's entry records carry the places; OPMHIP_SPLIT_ASM=0 (tuning) forces it off
void ensure_A(opmhip_ctx* c);                    // solver.hip: A_stale -> d_A gathered from d_R / d_U on the context's stream; in front of every reader of d_A
bool half_product_wanted(const opmhip_ctx* c);   // solver.hip: opmhip_config.half_product resolved for the pattern in hand (asked once, when the system's buffers are allocated)
void launch_ilu_factor(opmhip_ctx* c, bool fix_zero_diagonal = false, const FactorRider* rider = nullptr);
int cpr_factor_rider(opmhip_ctx* c, FactorRider* r);   // cpr.hip: level 0 in place, this solve's weights where they do not come from the matrix; r->mode = 0: no rider this time
void launch_ilu_apply(opmhip_ctx* c, const double* d, double* v, double w_override = -1.0, double* unscaled = nullptr, const double* addp = nullptr, double* work = nullptr, double* usum = nullptr);
// cpr.hip
// solveBoundary: the --cpr-reuse-setup rules are looked at (a structure may be rebuilt, started or swapped in); false (opmhip_cpr_apply:
// a look at the preconditioner between two solves): values only, the structure stays as the last solve left it
int cpr_update(opmhip_ctx* c, bool solveBoundary = true);
void launch_cpr_apply(opmhip_ctx* c, const double* d, double* v);
int cpr_set_weights(opmhip_ctx* c, const double* w);
int cpr_level_sizes(const opmhip_ctx* c, int* n, int* nnz, int cap);
void cpr_shutdown(opmhip_ctx* c);   // joins a structure build in flight (before the context goes)
bool cpr_coarse_pivot_failed(opmhip_ctx* c);
int cpr_ilu_levels_in_force(const opmhip_ctx* c);   // opmhip_config.cpr_amg_ilu_levels with "< 0: the library's choice" resolved (0 without CPR)
inline bool use_cpr(const opmhip_ctx* c) { return c->cfg.preconditioner == OPMHIP_PRECOND_CPR_QUASIIMPES || c->cfg.preconditioner == OPMHIP_PRECOND_CPR_TRUEIMPES; }
void launch_lu_to_natural(opmhip_ctx* c, double* d_out_internal_layout);
int bicgstab(opmhip_ctx* c, opmhip_result* res);
// comm.hip
int comm_allreduce(opmhip_ctx* c, double* d_buf, int n, int op /*0 sum, 1 max*/);
int comm_allgather(opmhip_ctx* c, const double* d_send, double* d_recv, size_t count);   // count doubles per rank -> nranks * count on every rank
int comm_halo_f64(opmhip_ctx* c, double* vec, int w, hipStream_t s = nullptr);   // s: the stream it runs on (default: the context's)
int comm_halo_begin(opmhip_ctx* c, double* vec);   // 3 doubles per cell: the exchange on the halo stream, ordered behind the main stream's work so far
int comm_halo_end(opmhip_ctx* c);                  // the main stream waits for it
int comm_halo_u8(opmhip_ctx* c, unsigned char* vec);
void comm_halo_bystander(opmhip_ctx* c);           // a rank without neighbours, where its peers exchange (loopback: their barriers count every rank)
void comm_release(opmhip_ctx* c);
// assemble.hip launchers
void launch_iq_update(opmhip_ctx* c);
int launch_ghost_refresh(opmhip_ctx* c);
void launch_newton_update(opmhip_ctx* c, const double* d_dx_internal, double relax);
void launch_assemble(opmhip_ctx* c, double dt, int iteration);
void launch_drift_update(opmhip_ctx* c, double dt);
void launch_aquifer_begin(opmhip_ctx* c);    // pressure_previous_ = p_w of the connected cells
void launch_aquifer_apply(opmhip_ctx* c);    // Qai_ of every connection; saved and raised source rows of the connected cells (in front of k_assemble)
void launch_aquifer_restore(opmhip_ctx* c);  // the caller's source rows back (behind k_assemble)
void launch_aquifer_end(opmhip_ctx* c, double dt);
// open boundaries (boundary.hip)
void launch_boundary_capture(opmhip_ctx* c);  // the exterior records of the cells with a FREE face, from the intensive-quantity cache
void launch_boundary_apply(opmhip_ctx* c);    // every face's rates; saved and lowered source rows / dsource blocks of the boundary cells (in front of k_assemble)
void launch_boundary_restore(opmhip_ctx* c);  // the caller's rows and blocks back (behind k_assemble)
// standard wells on the device (opmhip_set_std_wells; kernels and launchers: std_wells.hip, entry points: capi_std_wells.cpp)
int std_wells_check(opmhip_ctx* c, const double* flags);   // capi_std_wells.cpp: the zero-pivot flags as the caller has just read them back; a singular D clears the list
// capi_std_wells.cpp: the list's part of opmhip_advance_time_level / opmhip_update_failed, on the context's stream
int std_wells_save_state(opmhip_ctx* c);
int std_wells_restore_state(opmhip_ctx* c);
void launch_std_wells_solve(opmhip_ctx* c, bool first);   // heads, then the wells alone against the frozen reservoir (iteration 0)
void launch_std_wells_wellbore(opmhip_ctx* c, bool first, bool init);   // the heads from the well-bore density, in front of launch_std_wells_solve
void launch_std_wells_controls(opmhip_ctx* c);            // updateWellControls
void launch_std_wells_groups(opmhip_ctx* c, int iteration, bool check);   // lists with groups: [the groups' check,] the NUPCOL copy and the group data
void launch_std_wells_resv(opmhip_ctx* c);                // the field's averages and the RESV wells' coefficients (iteration 0, lists with a RESV limit)
void launch_std_wells_assemble(opmhip_ctx* c);            // rates, r_w, D, D^-1, B, C; saved and raised source rows (in front of k_assemble)
void launch_std_wells_restore(opmhip_ctx* c);             // the caller's source rows back (behind k_assemble)
void launch_std_wells_axpy(opmhip_ctx* c, double relax);  // x -= relax * x_w
// wells_operator.hip: the well operator y -= C^T (D^-1 (B (xs x))) behind launch_spmv's product, and the wells added to the matrix
int launch_wells_apply(opmhip_ctx* c, const double* x, double* y, double xs = 1.0);   // the solve's standard wells; distributed wells: one all-reduce inside
void launch_ms_wells_apply(opmhip_ctx* c, const double* x, double* y, double xs);     // the device-resident multisegment list: no copy, no synchronisation
int ms_wells_apply_callback(opmhip_ctx* c, const double* x, double* y, double xs);    // multisegment wells behind opmhip_wells.ms_apply: the host round trip
void launch_wells_residual(opmhip_ctx* c, const double* d_resWell, double* r);
int launch_wells_recover(opmhip_ctx* c, const double* d_resWell, const double* x, double* d_xw);   // distributed wells: one all-reduce inside
void launch_wells_add_to_matrix(opmhip_ctx* c, int w0, int nw, int serial, const int* d_pair_ptr, const int* d_entry);
void launch_std_wells_add_to_matrix(opmhip_ctx* c);       // A -= C^T D^-1 B by StdWellsDev's schedule (the matrix-add form), one launch
void ms_wells_tree_plan(opmhip_ctx* c, const std::vector<MsTreeDesc>& tdesc);   // MsWellsDev::tree_lds_doubles of a new list: the dynamic LDS of k_ms_wells_tree_apply
void launch_ms_wells_factor(opmhip_ctx* c);   // D -> D^-1 of every well of the device-resident multisegment list; pivot flags to MsWellsDev::d_flag
int ms_wells_check(opmhip_ctx* c);   // capi_ms_wells.cpp: the pivot flags of the last inversion, looked at where the host waits for the stream; a singular D clears the list
void launch_last_rs_rv(opmhip_ctx* c);
void launch_set_limits(opmhip_ctx* c, double dt);
void launch_min_pressure(opmhip_ctx* c, bool init);
void launch_storage_old(opmhip_ctx* c);
void launch_max_oil_saturation(opmhip_ctx* c, bool init);
void launch_max_water_saturation(opmhip_ctx* c, bool init);
void launch_hyst_update(opmhip_ctx* c, const double* d_sw_ow = nullptr, const double* d_sw_go = nullptr);
int launch_relative_change(opmhip_ctx* c);   // -> asmb.d_rc[512 .. 514)
int launch_convergence(opmhip_ctx* c, double dt, double tol_cnv);
void launch_reservoir_averages(opmhip_ctx* c);   // -> asmb.d_resv[RESV_MAX_PARTS * 8 .. + RESV_OUT)
double* resv_avg_kernels(opmhip_ctx* c);         // its two kernels without a profiling scope of their own (launch_std_wells_resv); returns where the RESV_OUT results go
void launch_u8_to_internal(opmhip_ctx* c, const unsigned char* nat, unsigned char* internal);
void launch_u8_to_natural(opmhip_ctx* c, const unsigned char* internal, unsigned char* nat);
void launch_iq_to_natural(opmhip_ctx* c, double* d_nat);
void launch_iq_gather(opmhip_ctx* c, int n, const int* d_pos, double* d_out);                                    // records of n cells (internal positions)
void launch_source_scatter(opmhip_ctx* c, int n, const int* d_pos, const double* d_src, const double* d_dsrc);   // d_dsrc nullable
// capi_asm.cpp: internal positions of n named cells on the device (AsmDev::d_cell_pos, grown on demand); the host copy stays valid until the caller's synchronise
int stage_cell_positions(opmhip_ctx* c, const std::vector<int>& pos);
// `pos` staged, then what `enqueue` puts on the stream - copies that read host vectors of the caller among it.  The stream is drained on
// the way out whatever happened: those vectors (and `pos`) may end with the caller's scope, no copy may still be reading them
template <class F>
int with_cell_positions(opmhip_ctx* c, const char* who, const std::vector<int>& pos, F&& enqueue) {
    int rc = stage_cell_positions(c, pos);
    if (!rc) rc = enqueue();
    if (hipStreamSynchronize(c->stream) != hipSuccess && !rc) return fail(c, OPMHIP_DEVICE_ERROR, "%s: hipStreamSynchronize failed", who);
    return rc;
}
// passive tracers (tracers.hip)
void launch_tracer_begin(opmhip_ctx* c, int phase);                        // updateStorageCache of one batch
void launch_tracer_system(opmhip_ctx* c, int phase, double dt);            // assembleTracerEquations_ of one batch -> TracersDev::d_M, d_res
int tracer_solve_batch(opmhip_ctx* c, int phase, opmhip_tracer_result* res_batch, bool* pivot_failed);   // ILU0, BiCGStab -> d_x; c -= x
// fluids in place (fip.hip)
void launch_fip_cells(opmhip_ctx* c);                      // the twelve per-cell terms of the state now present -> FipDev::d_terms
void launch_fip_reduce(opmhip_ctx* c, const FipSetDev& S);   // every level of the set's reduction, then the regions' and the field's sums -> FipDev::d_out
int iq_doubles_per_cell(const opmhip_ctx* c);
int asm_max_rows();
int launch_fluid_probe(opmhip_ctx* c, int pr, int sr, int n, const double* d_in, double* d_out);
// opmhip_vfp_probe (std_wells.hip): table = the index into the packed set; d_in = aqua | liquid | vapour | thp | alq | bhp_target (n each), d_out 10 per point
int launch_vfp_probe(opmhip_ctx* c, int table, int n, const double* d_in, bool has_target, double* d_out);
int launch_gas_probe(opmhip_ctx* c, int pr, int n, const double* d_in, double* d_out);
int launch_sat_probe(opmhip_ctx* c, int sr, int cfg, const double* d_eps, int n, const double* d_in, double* d_out);
int asm_threads();
void launch_vector_kernels_once(opmhip_ctx* c);
void launch_stream_read(opmhip_ctx* c);

}  // namespace opmhip
