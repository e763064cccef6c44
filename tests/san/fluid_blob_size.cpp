// The sizes of the property-table blobs build_fluid_tables (csrc/fluid_tables.cpp) makes of a fluid, under AddressSanitizer + UBSan +
// libstdc++'s container assertions (test infrastructure; built and run by tests/test_table_states.py with g++, no GPU).
// fluid_tables.cpp is linked alone: that the link succeeds is the check that the unit makes no HIP call.
// usage: fluid_blob_size FILE...   each FILE as tests/table_states.py write_fluid_binary writes it: int32 header (num_pvt, num_sat,
// num_rock, wet, then the element count of each of the 18 arrays), then the arrays in that order.  One line per file:
// "dbl <dbl.size()> idx <idx.size()>", or "error <text>".
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../opm-autodiff_amd/csrc/fluid_tables.hpp"

namespace {
const int N_ARR = 18;
// true: int32 array
const bool IS_INT[N_ARR] = {false, false, true, false, true, false, true, false, true, false, true, false, true, false, true, false, true, false};

bool read_exact(std::FILE* f, void* dst, size_t bytes) { return bytes == 0 || std::fread(dst, 1, bytes, f) == bytes; }
}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) {
        std::printf("usage: %s FILE...\n", argv[0]);
        return 2;
    }
    int bad = 0;
    for (int a = 1; a < argc; ++a) {
        std::FILE* f = std::fopen(argv[a], "rb");
        if (!f) {
            std::printf("error cannot open %s\n", argv[a]);
            ++bad;
            continue;
        }
        int head[4 + N_ARR];
        std::vector<std::vector<int>> iv(N_ARR);
        std::vector<std::vector<double>> dv(N_ARR);
        bool ok = read_exact(f, head, sizeof(head));
        for (int k = 0; ok && k < N_ARR; ++k) {
            const int n = head[4 + k];
            if (n < 0 || n > (1 << 24)) { ok = false; break; }
            if (IS_INT[k]) { iv[k].resize(n); ok = read_exact(f, iv[k].data(), sizeof(int) * (size_t)n); }
            else { dv[k].resize(n); ok = read_exact(f, dv[k].data(), sizeof(double) * (size_t)n); }
        }
        std::fclose(f);
        if (!ok) {
            std::printf("error short or malformed file %s\n", argv[a]);
            ++bad;
            continue;
        }
        auto D = [&](int k) -> const double* { return dv[k].empty() ? nullptr : dv[k].data(); };
        auto I = [&](int k) -> const int* { return iv[k].empty() ? nullptr : iv[k].data(); };
        opmhip_fluid fl;
        std::memset(&fl, 0, sizeof(fl));
        fl.num_pvt = head[0];
        fl.num_sat = head[1];
        fl.num_rock = head[2];
        fl.pvtw = D(0); fl.density = D(1);
        fl.pvdg_ptr = I(2); fl.pvdg = D(3);
        fl.pvto_node_ptr = I(4); fl.pvto_rs = D(5); fl.pvto_row_ptr = I(6); fl.pvto = D(7);
        fl.swof_ptr = I(8); fl.swof = D(9); fl.sgof_ptr = I(10); fl.sgof = D(11);
        fl.pvtg_node_ptr = I(12); fl.pvtg_pg = D(13); fl.pvtg_row_ptr = I(14); fl.pvtg = D(15);
        fl.rocktab_ptr = I(16); fl.rocktab = D(17);
        fl.rock_pref = 1e5;
        opmhip::FluidTables T;
        const std::string err = opmhip::build_fluid_tables(&fl, T);
        if (!err.empty()) {
            std::printf("error %s\n", err.c_str());
            ++bad;
            continue;
        }
        std::printf("dbl %zu idx %zu\n", T.dbl.size(), T.idx.size());
    }
    return bad ? 1 : 0;
}
