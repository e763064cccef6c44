// Host set-up of the open boundaries (csrc/boundary_setup.cpp: the checks with their codes and texts, the packed per-face arrays, the
// grouping of the faces by distinct cell, the exterior records' slots) under AddressSanitizer + UBSan + libstdc++'s container
// assertions (test infrastructure; built and run by tests/test_boundary_setup_sanitized.py with g++, no GPU).  boundary_setup.cpp is
// linked with source_lists.cpp (group_by_cell) and no stand-in for any HIP runtime call: that the link succeeds is the check that the
// set-up makes none.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <limits>
#include <numeric>
#include <string>
#include <vector>

#include "../../opm-autodiff_amd/csrc/boundary_setup.hpp"

using namespace opmhip;

static int g_fail = 0;
#define CHECK(cond, ...)                                                 \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); \
            std::printf(__VA_ARGS__);                                    \
            std::printf("\n");                                           \
            ++g_fail;                                                    \
            return false;                                                \
        }                                                                \
    } while (0)
static void report(bool ok, const char* what) {
    if (ok) std::printf("ok  %s\n", what);
}

// a list on heap arrays of exactly its length, so that a read past an end is seen
struct Faces {
    std::vector<int> cell, direction, type;
    std::vector<double> area, trans, depth, rate;
    opmhip_boundary_conditions bc() const {
        return opmhip_boundary_conditions{(int)cell.size(), cell.data(), direction.data(), type.data(), area.data(), trans.data(), depth.data(), rate.data()};
    }
    void add(int c, int d, int t, double a = 2.0, double tr = 1e-12, double z = 2500.0) {
        cell.push_back(c); direction.push_back(d); type.push_back(t); area.push_back(a + (double)cell.size()); trans.push_back(tr); depth.push_back(z);
        for (int e = 0; e < 3; ++e) rate.push_back(t == OPMHIP_BC_RATE ? 1e-4 * (e + 1) + (double)cell.size() : 777.0);
    }
};

// all six sides of an nx x ny x nz box, side by side as the tests list them; every `rate_every`-th face a RATE face
static Faces box_faces(int nx, int ny, int nz, int rate_every) {
    Faces F;
    int n = 0;
    for (int d = 0; d < 6; ++d)
        for (int k = 0; k < nz; ++k)
            for (int j = 0; j < ny; ++j)
                for (int i = 0; i < nx; ++i) {
                    const int at[6] = {i == 0, i == nx - 1, j == 0, j == ny - 1, k == 0, k == nz - 1};
                    if (!at[d]) continue;
                    F.add(i + nx * (j + ny * k), d, (rate_every && ++n % rate_every == 0) ? OPMHIP_BC_RATE : OPMHIP_BC_FREE);
                }
    return F;
}

static bool check_lists(const Faces& F, int Nb, const std::vector<int>& toOrder, int want_nf, int want_nd) {
    BoundaryContext X;
    X.Nb = Nb;
    BoundaryLists L;
    std::string msg;
    const opmhip_boundary_conditions bc = F.bc();
    const int rc = boundary_lists(&bc, X, toOrder.data(), L, msg);
    CHECK(rc == OPMHIP_SUCCESS, "rc %d: %s", rc, msg.c_str());
    const int nf = (int)F.cell.size(), nd = (int)L.cpos.size();
    CHECK(L.nf == nf && nf == want_nf && nd == want_nd, "nf %d nd %d", L.nf, nd);
    CHECK((int)L.type.size() == nf && (int)L.geo.size() == 3 * nf && (int)L.rate.size() == 3 * nf && (int)L.pos.size() == nf && (int)L.cconn.size() == nf &&
              (int)L.cptr.size() == nd + 1 && (int)L.slot.size() == nd, "sizes");
    for (int f = 0; f < nf; ++f) {
        CHECK(L.type[f] == F.type[f] && L.geo[3 * f] == F.area[f] && L.geo[3 * f + 1] == F.trans[f] && L.geo[3 * f + 2] == F.depth[f], "face %d", f);
        CHECK(L.pos[f] == toOrder[F.cell[f]], "pos %d", f);
        for (int e = 0; e < 3; ++e) CHECK(L.rate[3 * f + e] == (F.type[f] == OPMHIP_BC_RATE ? F.rate[3 * f + e] : 0.0), "rate %d", f);
    }
    // the grouping against a quadratic restatement: distinct cells in the order of first mention, their faces ascending
    std::vector<int> first;
    for (int f = 0; f < nf; ++f)
        if (std::find(first.begin(), first.end(), F.cell[f]) == first.end()) first.push_back(F.cell[f]);
    CHECK((int)first.size() == nd && L.cptr[0] == 0 && L.cptr[nd] == nf, "distinct cells");
    int nfree = 0;
    for (int t = 0; t < nd; ++t) {
        CHECK(L.cpos[t] == toOrder[first[t]], "cpos %d", t);
        std::vector<int> mine;
        bool has_free = false;
        for (int f = 0; f < nf; ++f)
            if (F.cell[f] == first[t]) { mine.push_back(f); has_free = has_free || F.type[f] == OPMHIP_BC_FREE; }
        CHECK(L.cptr[t + 1] - L.cptr[t] == (int)mine.size() && mine.size() <= 6, "faces of cell %d", t);
        for (size_t k = 0; k < mine.size(); ++k) CHECK(L.cconn[L.cptr[t] + k] == mine[k], "cconn %d", t);
        if (has_free) {
            CHECK(L.slot[t] == nfree && L.fcell[nfree] == t, "slot %d", t);
            ++nfree;
        } else CHECK(L.slot[t] == -1, "slot %d of a cell without a FREE face", t);
    }
    CHECK((int)L.fcell.size() == nfree, "records");
    return true;
}

static bool lists() {
    std::vector<int> id(162), rev(162), three{2, 0, 1};
    std::iota(id.begin(), id.end(), 0);
    for (int i = 0; i < 162; ++i) rev[i] = 161 - i;
    if (!check_lists(box_faces(9, 9, 2, 0), 162, id, 234, 162)) return false;        // more than two waves, corner cells with three faces
    if (!check_lists(box_faces(9, 9, 2, 3), 162, rev, 234, 162)) return false;       // RATE faces among them, another ordering
    if (!check_lists(box_faces(3, 1, 1, 2), 3, three, 14, 3)) return false;          // five faces per end cell
    if (!check_lists(box_faces(1, 1, 1, 1), 1, std::vector<int>{0}, 6, 1)) return false;   // six RATE faces: no record at all
    Faces one;
    one.add(7, 3, OPMHIP_BC_FREE);
    Faces norate = one;
    norate.rate.clear();                                                                 // rate may be NULL without RATE faces
    opmhip_boundary_conditions bc = norate.bc();
    bc.rate = nullptr;
    BoundaryContext X;
    X.Nb = 162;
    BoundaryLists L;
    std::string msg;
    CHECK(boundary_lists(&bc, X, id.data(), L, msg) == OPMHIP_SUCCESS && L.nf == 1 && L.fcell.size() == 1, "one FREE face, rate NULL: %s", msg.c_str());
    return check_lists(one, 162, id, 1, 1);
}

static bool refused_as(Faces F, BoundaryContext X, const char* word, void (*edit)(opmhip_boundary_conditions&) = nullptr) {
    std::vector<int> id((size_t)X.Nb);
    std::iota(id.begin(), id.end(), 0);
    opmhip_boundary_conditions bc = F.bc();
    if (edit) edit(bc);
    BoundaryLists L;
    L.nf = -5;
    std::string msg;
    const int rc = boundary_lists(&bc, X, id.data(), L, msg);
    CHECK(rc == OPMHIP_INVALID_ARGUMENT, "%s: rc %d", word, rc);
    CHECK(msg.find(word) != std::string::npos && msg.rfind("set_boundary_conditions", 0) == 0 && msg.size() < 512, "%s: text '%s'", word, msg.c_str());
    CHECK(L.nf == -5 && L.type.empty() && L.cpos.empty(), "%s: outputs touched", word);
    return true;
}

static bool refusals() {
    BoundaryContext X;
    X.Nb = 12;
    Faces G;
    G.add(0, 0, OPMHIP_BC_FREE); G.add(0, 2, OPMHIP_BC_RATE); G.add(11, 5, OPMHIP_BC_FREE);
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    bool ok = true;
    ok = ok && refused_as(G, X, "null array", [](opmhip_boundary_conditions& b) { b.cell = nullptr; });
    ok = ok && refused_as(G, X, "null array", [](opmhip_boundary_conditions& b) { b.direction = nullptr; });
    ok = ok && refused_as(G, X, "null array", [](opmhip_boundary_conditions& b) { b.type = nullptr; });
    ok = ok && refused_as(G, X, "null array", [](opmhip_boundary_conditions& b) { b.area = nullptr; });
    ok = ok && refused_as(G, X, "null array", [](opmhip_boundary_conditions& b) { b.trans = nullptr; });
    ok = ok && refused_as(G, X, "null array", [](opmhip_boundary_conditions& b) { b.depth = nullptr; });
    ok = ok && refused_as(G, X, "null array", [](opmhip_boundary_conditions& b) { b.rate = nullptr; });
    ok = ok && refused_as(G, X, "num_faces", [](opmhip_boundary_conditions& b) { b.num_faces = -1; });
    Faces F = G; F.cell[2] = 12;
    ok = ok && refused_as(F, X, "outside [0, 12)");
    F = G; F.cell[0] = -1;
    ok = ok && refused_as(F, X, "outside [0, 12)");
    F = G; F.direction[1] = 6;
    ok = ok && refused_as(F, X, "outside 0..5");
    F = G; F.direction[1] = -1;
    ok = ok && refused_as(F, X, "outside 0..5");
    F = G; F.direction[1] = 0;
    ok = ok && refused_as(F, X, "listed twice");
    F = G; F.area[0] = 0.0;
    ok = ok && refused_as(F, X, "not positive");
    F = G; F.area[2] = -1.0;
    ok = ok && refused_as(F, X, "not positive");
    F = G; F.area[2] = nan;
    ok = ok && refused_as(F, X, "not positive");
    F = G; F.trans[1] = -1e-15;
    ok = ok && refused_as(F, X, "negative or not finite");
    F = G; F.trans[1] = inf;
    ok = ok && refused_as(F, X, "negative or not finite");
    F = G; F.trans[1] = nan;
    ok = ok && refused_as(F, X, "negative or not finite");
    F = G; F.type[2] = 2;
    ok = ok && refused_as(F, X, "unknown type");
    F = G; F.depth[0] = inf;
    ok = ok && refused_as(F, X, "depth");
    F = G; F.rate[4] = nan;
    ok = ok && refused_as(F, X, "rate 1 is not finite");
    BoundaryContext D = X; D.nranks = 2;
    ok = ok && refused_as(G, D, "decomposed");
    BoundaryContext H = X; H.hysteresis = true;
    ok = ok && refused_as(G, H, "hysteresis");
    BoundaryContext W = X; W.water_compaction = true;
    ok = ok && refused_as(G, W, "water-induced compaction");
    if (!ok) return false;
    // accepted: RATE faces alone beside hysteresis; a zero transmissibility; a FREE face's rate entries are never read as numbers
    Faces R;
    R.add(3, 1, OPMHIP_BC_RATE, 2.0, 0.0);
    std::vector<int> id(12);
    std::iota(id.begin(), id.end(), 0);
    BoundaryLists L;
    std::string msg;
    const opmhip_boundary_conditions bc = R.bc();
    CHECK(boundary_lists(&bc, H, id.data(), L, msg) == OPMHIP_SUCCESS && L.fcell.empty() && L.slot[0] == -1, "RATE beside hysteresis: %s", msg.c_str());
    F = G; F.rate[0] = nan;
    const opmhip_boundary_conditions bf = F.bc();
    CHECK(boundary_lists(&bf, X, id.data(), L, msg) == OPMHIP_SUCCESS && L.rate[0] == 0.0, "a FREE face's rate: %s", msg.c_str());
    return true;
}

int main() {
    report(lists(), "lists: 9 x 9 x 2 with six sides (234 faces, 162 cells), with RATE faces and another ordering, 3 x 1 x 1, one cell, one face");
    report(refusals(), "refused: null arrays, count, cell, direction, twice, area, transmissibility, type, depth, rate, ranks, hysteresis, compaction; accepted: RATE beside hysteresis");
    if (g_fail) return 1;
    std::printf("all checks passed\n");
    return 0;
}
