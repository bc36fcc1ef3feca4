// position_map_check.cpp -- TEST INFRASTRUCTURE: a stand-alone program over layout::csc_rows_position_map (spmv_layout.cpp), the map the value refresh of
// qps_update_shared_matrices_csc reads.  tests/test_matrix_update_cpu.py compiles it together with spmv_layout.cpp by g++ -fsanitize=address,undefined and runs it on
// the pattern of every sparse case.  Input (argv[1], text): any number of patterns "nrows ncols nnz" + colptr[ncols + 1] + rowval[nnz], canonical, 0-based.
// For every pattern the map is held against a brute-force search and against the by-rows copy of csc_to_csr_pair.  Exit code 0: all patterns agree.
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <vector>

#include "../../quadraticprogramsolver_amd/csrc/spmv_layout.h"

using namespace qps::layout;

static int check(int64_t nrows, int64_t ncols, const std::vector<int64_t>& cp, const std::vector<int64_t>& ri) {
    const int64_t nnz = cp[(size_t)ncols];
    const std::vector<int> map = csc_rows_position_map(nrows, ncols, cp, ri);
    if ((int64_t)map.size() != nnz) return 1;
    // the by-rows copy with the CSC position as the value: the map has to name exactly where each of its entries came from
    std::vector<double> nz((size_t)nnz);
    for (int64_t k = 0; k < nnz; ++k) nz[(size_t)k] = (double)k;
    CsrHost rows, cols;
    csc_to_csr_pair(nrows, ncols, cp, ri, nz, rows, cols);
    for (int64_t k = 0; k < nnz; ++k) if (rows.va[(size_t)k] != (double)map[(size_t)k]) return 2;
    // brute force: entry k of row r holds column j; its CSC position is found by walking column j
    std::vector<char> hit((size_t)nnz, 0);
    for (int r = 0; r < rows.nrows; ++r)
        for (int k = rows.rp[(size_t)r]; k < rows.rp[(size_t)r + 1]; ++k) {
            const int j = rows.ci[(size_t)k];
            int64_t found = -1;
            for (int64_t p = cp[(size_t)j]; p < cp[(size_t)j + 1]; ++p) if (ri[(size_t)p] == r) { found = p; break; }
            if (found < 0 || found != map[(size_t)k]) return 3;
            if (hit[(size_t)found]++) return 4;          // a permutation: no CSC position twice
        }
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: %s patterns.txt\n", argv[0]); return 64; }
    std::ifstream in(argv[1]);
    if (!in) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 65; }
    int64_t nrows, ncols, nnz; int count = 0;
    while (in >> nrows >> ncols >> nnz) {
        std::vector<int64_t> cp((size_t)ncols + 1), ri((size_t)nnz);
        for (auto& v : cp) in >> v;
        for (auto& v : ri) in >> v;
        if (!in || cp[(size_t)ncols] != nnz) { std::fprintf(stderr, "pattern %d: malformed input\n", count); return 66; }
        const int rc = check(nrows, ncols, cp, ri);
        if (rc != 0) { std::fprintf(stderr, "pattern %d (%lld x %lld, %lld entries): check %d failed\n", count, (long long)nrows, (long long)ncols, (long long)nnz, rc); return 1; }
        ++count;
    }
    std::printf("%d patterns: position map == brute force\n", count);
    return count > 0 ? 0 : 67;
}
