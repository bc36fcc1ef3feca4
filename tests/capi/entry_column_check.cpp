// entry_column_check.cpp -- TEST INFRASTRUCTURE: a stand-alone program over layout::csc_column_of_entry (spmv_layout.cpp), the row-of-entry index the value
// gradients of qps_adjoint_shared read on the device.  tests/test_adjoint_cpu.py compiles it together with spmv_layout.cpp by g++ -fsanitize=address,undefined and
// runs it on the patterns of its cases.  Input (argv[1], text): any number of patterns "ncols nnz" + colptr[ncols + 1], canonical, 0-based.  For every pattern
// the array is held against a search of colptr per entry.  Exit code 0: all patterns agree.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <vector>

#include "../../quadraticprogramsolver_amd/csrc/spmv_layout.h"

using namespace qps::layout;

static int check(int64_t ncols, const std::vector<int64_t>& cp) {
    const int64_t nnz = cp[(size_t)ncols];
    const std::vector<int> col = csc_column_of_entry(ncols, cp);
    if ((int64_t)col.size() != nnz) return 1;
    for (int64_t k = 0; k < nnz; ++k) {
        const int64_t j = (std::upper_bound(cp.begin(), cp.end(), k) - cp.begin()) - 1;   // the last column that starts at or before k (empty columns skipped)
        if (col[(size_t)k] != j) return 2;
        if (!(cp[(size_t)j] <= k && k < cp[(size_t)j + 1])) return 3;
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: %s patterns.txt\n", argv[0]); return 64; }
    std::ifstream in(argv[1]);
    if (!in) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 65; }
    int64_t ncols, nnz; int count = 0;
    while (in >> ncols >> nnz) {
        std::vector<int64_t> cp((size_t)ncols + 1);
        for (auto& x : cp) in >> x;
        if (!in || cp[(size_t)ncols] != nnz) { std::fprintf(stderr, "pattern %d: malformed input\n", count); return 66; }
        const int rc = check(ncols, cp);
        if (rc != 0) { std::fprintf(stderr, "pattern %d (%lld columns, %lld entries): check %d failed\n", count, (long long)ncols, (long long)nnz, rc); return 1; }
        ++count;
    }
    std::printf("%d patterns: column of entry == search of colptr\n", count);
    return count > 0 ? 0 : 67;
}
