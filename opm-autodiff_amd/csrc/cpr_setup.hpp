// Host side of the CPR pressure-AMG set-up (cpr_setup.cpp): the hierarchy's matching, Galerkin gather lists, ELL images, ILU0
// smoothing schedules and colourings - pure host work on copies, no HIP call, so that it can run on a thread of its own beside the
// solves (cpr.hip: --cpr-reuse-setup=2 with opmhip_config.cpr_async_setup) and be built and checked without a device
// (tests/san/cpr_setup_san.cpp).  cpr.hip uploads what it produces.  The joined level of a decomposed run (cpr.hip: cpr_gather_setup) has its
// index work here as well - aggregates composed down the levels, a rank's rows, their values, everybody's rows into one matrix - as
// functions of plain vectors: no context, no communicator; a refusal comes back as an error string.
#pragma once
#include <climits>
#include <string>
#include <vector>

namespace opmhip {

struct Pattern;

constexpr int CPR_COARSE_DIRECT = 128;   // coarsest level: dense LU up to this many rows
constexpr int CPR_MAX_LEVELS = 15;
constexpr int CPR_MAX_W = 96;            // longest row an ELL level may have
constexpr int CPR_LPR_ROWS = 32768;      // levels of up to this many rows are kept row-major (the default of lprRows)

struct HCsr {
    int n = 0;
    std::vector<int> rowptr, col;
    std::vector<double> val;
};
// Host-side description of the hierarchy (cpr_build_coarse_host): everything the device arrays of a level are uploaded from.
// The set-up is split in two so that its expensive half - matching, Galerkin lists, level images: pure host work on copies -
// can run on a thread of its own beside the solves (--cpr-reuse-setup=2 with opmhip_config.cpr_async_setup), and only the uploads
// touch the context.
// ILU0 smoothing schedule of one level, from its image: which slots of a row are lower / upper entries in the elimination order
// `pos`, the lower slots in ascending position, and per colour the sequences of rows a thread walks.  colour[i] ascending = the
// order of the launches; rows of one colour may depend on each other only along a sequence (a chain of level 0's line colouring).
struct CprIluHost {
    int ncol = 0, MW = 0, WL = 0, WU = 0;
    std::vector<int> nseq, nsteps, off, rowAt, wl, wu;   // wl / wu: lower / upper entries per row of a colour at most
    std::vector<char> fast;
    std::vector<unsigned> mask;
    std::vector<unsigned char> lorder;
    // simple: a level whose elimination steps touch nothing but the diagonal (no triangles in its graph: step (i, j) finds of row j's
    // upper entries only (j, i) in row i - a seven-point grid in any of the orderings here), whose couplings inside a colour join
    // neighbours of a sequence and whose rows hold their lower entries in elimination order: U keeps the matrix's own values,
    // l_ij = a_ij / u_jj, u_ii = a_ii - sum_j l_ij a_ji - a recurrence along the sequences with loads that depend on nothing it computes
    // (k_cpr_ilu_factor_simple).  tpos: per lower entry (slot order) the place of the transposed entry (j, i) in the level's image
    bool simple = false;
    std::vector<int> tpos;
    std::string error;
};
struct CprHostLevel {
    int n = 0, nnz = 0, nc = 0, W = 0;
    bool rm = false;
    std::vector<int> ecol, rlen, diag;                           // ELL image of the level's pattern
    std::vector<int> agg, mptr, midx, mem4, gptr, gidx, cpos;    // transfer to the next level (empty on the coarsest)
    CprIluHost ilu;                                              // ncol > 0: the level's ILU0 smoothing schedule
};
struct CprHostCoarse {
    CprHostLevel l0;                 // of level 0 only the transfer part (its image belongs to the pattern: cpr_setup_level0)
    std::vector<CprHostLevel> lv;    // levels 1 ..
    double tAgg = 0.0, tGal = 0.0, tImg = 0.0;
    std::string error;               // non-empty: the build failed
    HCsr lastA;                      // the last level's matrix and the place of its entries in that level's image
    std::vector<int> lastPos;
};

// ELL image of a level's pattern: columns (padding: the row itself), row lengths, position of the diagonal, position of every
// CSR entry
bool ell_image(const HCsr& A, CprHostLevel& L, std::vector<int>& pos, bool rowMajor, int ncols = INT_MAX);
void cpr_ilu_schedule(const CprHostLevel& L, const std::vector<int>& pos, const std::vector<int>& colour, int ncol, CprIluHost& S);
// greedy multi-colouring of a level's graph in index order, colour-major elimination positions (oracle/cpr.hpp: ilu_factor, colour = true)
int cpr_greedy_colours(const CprHostLevel& L, std::vector<int>& colour, std::vector<int>& pos);
// The coarsening itself: A = the finest level of the hierarchy being built (CSR with values), pos = the place of every entry of A in
// that level's image on the device; natOf / atNat: see pairwise (level 0 of a reordered system, else NULL).  stopRows: a level of at
// most this many rows is the last one (CPR_COARSE_DIRECT: it is solved directly; a rank whose hierarchy is continued across the ranks
// stops at opmhip_config.cpr_gather_rows).  The last level's matrix stays in out.lastA / lastPos.
void cpr_coarsen_host(HCsr A, std::vector<int> pos, const int* natOf, const int* atNat, double beta, int lprRows, int iluLevels, int stopRows, CprHostCoarse& out);
// Everything below level 0's image, on the host: two passes of pairwise matching per level, Galerkin lists, level images.
// Pure host work on its arguments (no context, no HIP call): may run on a thread of its own.  ell0: level 0's value image
// (W0 x Nb, as on the device) of the pressure matrix the structure is built from.
void cpr_build_coarse_host(const Pattern& P, const std::vector<double>& ell0, double beta, int lprRows, int iluLevels, int stopRows, CprHostCoarse& out);
// Level 0's ILU0 smoothing schedule in the stored order: the block ILU0's colours (rows of colour c: [colourPrefix[c], colourPrefix[c + 1]))
// are this one's, the elimination position of a row is its index
void cpr_level0_ilu_schedule(const CprHostLevel& L0, const std::vector<int>& colourPrefix, int ncol, CprIluHost& S);

// ---- the joined level of a decomposed run: the index work between cpr_gather_setup's exchanges (cpr.hip) --------------------------------
// Rank r's last level (n_r rows) becomes rows [offs[r], offs[r + 1]) of ONE matrix that every rank holds.  Its entries: the last
// level's own (columns shifted by offs[r]), and per pair (my aggregate, an aggregate of another rank) that fine couplings to ghost
// cells join the sum of their pressure values.
// The aggregate, on the rank's last level, of every owned cell: H.l0.agg and H.lv[*].agg composed (the identity where level 0 is the last)
std::vector<int> cpr_joined_aggregates(int nb, const CprHostCoarse& H);
struct CprJoinedRows {
    std::vector<int> qrow, qentry;   // the pattern's couplings to ghost cells in entry order: owned row, entry (k_cpr_ghost_pvals forms apg from them)
    std::vector<int> rowlen, cols;   // my rows: lengths, joined columns (ascending in a row)
    // value of entry e (k_cpr_gather_vals, cpr_joined_values): src[e] >= 0: the last level's entry at that place of its image (H.lastPos),
    // else the sum of apg[xidx[t]] over t in [xptr[x], xptr[x + 1]), x = -1 - src[e], in list order = by (owned row, owner-side place)
    std::vector<int> src, xptr, xidx;
};
// My rows, structure only.  rowptr / col: the local pattern (nb owned rows, columns >= nb: ghost cells); per ghost cell (column - nb)
// what its owner says of it: its row of the joined level, and the owner-side global place of the cell; off = offs[me]
void cpr_joined_rows(int nb, const std::vector<int>& rowptr, const std::vector<int>& col, const std::vector<int>& cagg, const std::vector<int>& ghostRow,
                     const std::vector<long long>& ghostPlace, int off, const HCsr& lastA, const std::vector<int>& lastPos, CprJoinedRows& out);
// Their values: k_cpr_gather_vals's statement with the last level's values in entry order (own entries appear in that order)
std::vector<double> cpr_joined_values(const CprJoinedRows& Q, const std::vector<double>& apg, const std::vector<double>& lastval);
// Everybody's rows into one CSR.  bl / bc / bv: per rank maxn row lengths, maxnnz columns and values (padded); nnzs[r]: entries of
// rank r.  unpad / vunpad: the place of row I / entry e of J in the padded buffers.  Every index is bounded before it is used; the
// refusal names the rank (the same data on every rank: all refuse alike)
struct CprJoined {
    HCsr J;
    std::vector<int> unpad, vunpad;
    std::string error;
};
void cpr_join_rows(const std::vector<int>& bl, const std::vector<int>& bc, const std::vector<double>& bv, const std::vector<int>& nnzs, const std::vector<int>& offs,
                   int maxn, int maxnnz, CprJoined& out);

}  // namespace opmhip
