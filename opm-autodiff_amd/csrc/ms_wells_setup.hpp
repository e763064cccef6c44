// Host set-up of the tree form of the device-resident multisegment wells (opmhip_set_ms_wells_form, OPMHIP_MS_WELLS_TREE / _AUTO): from
// the scalar CSC arrays of one well's D the block graph over its segments, the check that this graph is a forest, the elimination order
// (parents, levels, children) and, per CSC entry, its place in the blocks the kernels keep.  Pure host work on its arguments, no context
// and no HIP call, so that it is built and checked without a device (tests/san/ms_wells_tree_san.cpp).  capi.cpp allocates, uploads and
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

}   // namespace opmhip
