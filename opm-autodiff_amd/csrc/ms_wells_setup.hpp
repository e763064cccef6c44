// Host set-up of the device-resident multisegment wells (opmhip_set_ms_wells): the check of the caller's list, its layout on the device
// (descriptors, the form chosen per well, the tree wells' index lists, per block its segment row, cells in the internal order, shared
// cells) and, for the tree form (opmhip_set_ms_wells_form, OPMHIP_MS_WELLS_TREE / _AUTO), from the scalar CSC arrays of one well's D the
// block graph over its segments, the check that this graph is a forest, the elimination order (parents, levels, children) and, per CSC
// entry, its place in the blocks the kernels keep.  Pure host work on its arguments, no context and no HIP call, so that it is built and
// checked without a device (tests/san/ms_wells_tree_san.cpp, tests/san/ms_wells_list_san.cpp).  capi_ms_wells.cpp allocates, uploads and
// launches.  A refusal is a code other than OPMHIP_SUCCESS with its text in `msg`, for the caller's fail(); `out` is then untouched.
#pragma once
#include <string>
#include <vector>

#include "../../include/opmhip.h"

namespace opmhip {

// The blocks of one segment as k_ms_wells_tree_factor keeps them: MS_TREE_SEG doubles, three 4 x 4 blocks, row-major.
//   MS_TREE_DIAG  D_ii, after the factorisation S_i^-1
//   MS_TREE_UP    D_pi (row in the parent p, column in i), after the factorisation E_i = D_pi S_i^-1
//   MS_TREE_DOWN  D_ip (row in i, column in the parent)
// A root's UP and DOWN blocks stay zero.
constexpr int MS_TREE_DIAG = 0, MS_TREE_UP = 16, MS_TREE_DOWN = 32, MS_TREE_SEG = 48;

// Per well one descriptor; D^-1 dense and COLUMN-major (element (i, j) of well w at inv[inv0 + j * M + i]) - the elimination's lanes and
// the product's threads both run down a column.
struct MsWellDesc {
    int Mb, nblk;      // segments, blocks
    int seg0;          // well's part of Brows (Mb + 1 entries)
    int blk0;          // first block
    int dcol0, dnz0;   // well's part of Dcol_pointers (4 Mb + 1 entries), first entry of D
    int inv0;          // first double of the dense D^-1
    int well;          // its number in the list (the place of its pivot flag): a list may hold wells of both forms
};
// The tree form: D block-sparse over the segment tree, 48 doubles per segment (S_i^-1 | E_i = D_pi S_i^-1 | D_ip).  The well's index
// lists lie one after the other in MsWellsDev::d_tint.
struct MsTreeDesc {
    int Mb, nblk, seg0, blk0, dcol0, dnz0, well;   // as MsWellDesc's
    int depth, width;                              // levels; segments of the widest level
    int par0, cptr0, child0, lptr0, lseg0, dest0;  // in d_tint: parent [Mb], child_ptr [Mb + 1], child, level_ptr [depth + 1], level_seg [Mb], dest [nnz]
    int fac0;                                      // first double of the well's blocks in d_fac
};

struct MsTreeWell {
    int Mb = 0;
    int depth = 0;      // levels
    int width = 0;      // segments of the widest level
    std::vector<int> parent;     // [Mb] -1: a root (the lowest segment number of its component)
    std::vector<int> level;      // [Mb] distance from the root
    std::vector<int> child_ptr;  // [Mb + 1] ...
    std::vector<int> child;      // ... the children of each segment, ascending
    std::vector<int> level_ptr;  // [depth + 1] ...
    std::vector<int> level_seg;  // [Mb] ... the segments of each level, ascending
    std::vector<int> dest;       // [nnz] per CSC entry: segment * MS_TREE_SEG + block + 4 * (row in the block) + column in the block
};

// colptr: the well's 4 Mb + 1 column pointers (from 0, ascending); rows: its entries' rows, each inside [0, 4 Mb) - both checked by the
// caller.  Segments i != j are neighbours if an entry of D lies in block (i, j) or (j, i).  A graph with a cycle is refused
// (INVALID_ARGUMENT) naming `well` and the two segments of an edge that closes it.
int ms_wells_tree_analyse(int well, int Mb, const int* colptr, const int* rows, MsTreeWell& out, std::string& msg);

// The list check, on every call: the pointer arrays' consistency, the size caps of the form in force (OPMHIP_MS_WELLS_DENSE / _TREE /
// _AUTO), D's rows and values, the blocks' cells against Nb - in this order, the first defect met is the one reported.  The arrays of
// `ms` are non-null and num_ms_wells > 0 (the caller has looked).
struct MsWellsList {
    std::vector<MsWellDesc> all;   // every well's descriptor, in list order; inv0 counts the dense wells only
    std::vector<int> wform;        // its form: 0 dense, 1 tree (under AUTO a well above OPMHIP_MS_WELLS_MAX_M is a candidate for the tree form, settled by the layout)
    size_t invDoubles = 0;         // the dense wells' D^-1
    int maxM = 0;
    size_t nseg = 0, nblk = 0, nnz = 0;   // the list's totals
};
int ms_wells_list_check(const opmhip_ms_wells& ms, int form, int Nb, MsWellsList& out, std::string& msg);

// The list layout, for a list whose structure is new: the descriptors by form, the tree wells' analysis with their index lists one after
// the other, per block its segment row and its cell in the internal order (toOrder: Nb entries), and whether two blocks meet in a cell.
struct MsWellsLayout {
    std::vector<MsWellDesc> desc;    // the dense wells
    std::vector<MsTreeDesc> tdesc;   // the tree wells
    std::vector<int> tint;
    size_t facDoubles = 0;           // the tree wells' blocks
    int treeSeg = 0, treeDepth = 0;  // the largest tree well's segments, the deepest one's levels
    std::vector<int> cell, blkrow;
    bool shared = false;
};
int ms_wells_list_layout(const opmhip_ms_wells& ms, int form, int Nb, const int* toOrder, const MsWellsList& list, MsWellsLayout& out, std::string& msg);

}   // namespace opmhip
