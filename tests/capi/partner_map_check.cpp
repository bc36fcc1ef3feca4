// partner_map_check.cpp -- TEST INFRASTRUCTURE: a stand-alone program over layout::csc_transpose_partner_map (spmv_layout.cpp), the map the symmetry test of
// qps_update_shared_values reads on the device.  tests/test_value_update_cpu.py compiles it together with spmv_layout.cpp by g++ -fsanitize=address,undefined and
// runs it on the pattern of P of every sparse case.  Input (argv[1], text): any number of square patterns "n nnz" + colptr[n + 1] + rowval[nnz], canonical,
// 0-based.  For every pattern the map is held against a brute-force search, and the decision it leads to against layout::csc_asymmetry on values that are
// symmetric, then on values with one entry changed at a time.  Exit code 0: all patterns agree.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <vector>

#include "../../quadraticprogramsolver_amd/csrc/spmv_layout.h"

using namespace qps::layout;

// what the device decides from the map: the minimum, over offending entries, of min(i, j); -1: symmetric
static int64_t column_by_map(int64_t n, const std::vector<int64_t>& cp, const std::vector<int64_t>& ri, const std::vector<int>& map, const std::vector<double>& v) {
    int64_t best = -1;
    for (int64_t j = 0; j < n; ++j)
        for (int64_t k = cp[(size_t)j]; k < cp[(size_t)j + 1]; ++k) {
            const int p = map[(size_t)k];
            const bool off = p >= 0 ? v[(size_t)k] != v[(size_t)p] : v[(size_t)k] != 0.0;
            if (off) { const int64_t c = std::min(j, ri[(size_t)k]); if (best < 0 || c < best) best = c; }
        }
    return best;
}

static int check(int64_t n, const std::vector<int64_t>& cp, const std::vector<int64_t>& ri) {
    const int64_t nnz = cp[(size_t)n];
    const std::vector<int> map = csc_transpose_partner_map(n, cp, ri);
    if ((int64_t)map.size() != nnz) return 1;
    for (int64_t j = 0; j < n; ++j)
        for (int64_t k = cp[(size_t)j]; k < cp[(size_t)j + 1]; ++k) {
            const int64_t i = ri[(size_t)k];
            int64_t found = -1;                                    // brute force: walk column i for row j
            for (int64_t p = cp[(size_t)i]; p < cp[(size_t)i + 1]; ++p) if (ri[(size_t)p] == j) { found = p; break; }
            if (found != map[(size_t)k]) return 2;
            if (found >= 0 && map[(size_t)found] != k) return 3;   // an involution where it is defined
            if (i == j && map[(size_t)k] != k) return 4;           // a diagonal entry is its own partner
        }
    // values: v(i, j) = 1 + min(i, j) + n max(i, j) is symmetric; an entry without a partner holds 0.0
    std::vector<double> v((size_t)nnz);
    for (int64_t j = 0; j < n; ++j)
        for (int64_t k = cp[(size_t)j]; k < cp[(size_t)j + 1]; ++k)
            v[(size_t)k] = map[(size_t)k] >= 0 ? 1.0 + (double)std::min(j, ri[(size_t)k]) + (double)n * (double)std::max(j, ri[(size_t)k]) : 0.0;
    if (nnz > 0 && (csc_asymmetry(n, cp.data(), ri.data(), v.data(), 0) != -1 || column_by_map(n, cp, ri, map, v) != -1)) return 5;
    const int64_t step = std::max<int64_t>(1, nnz / 97);           // one entry changed at a time, a sample that reaches both ends
    for (int64_t k = 0; k < nnz; k += (k + step < nnz || k == nnz - 1) ? step : nnz - 1 - k) {
        if (map[(size_t)k] == (int)k) continue;                    // a diagonal entry cannot be asymmetric
        const double keep = v[(size_t)k];
        v[(size_t)k] = keep + 0.5;
        const int64_t want = csc_asymmetry(n, cp.data(), ri.data(), v.data(), 0), got = column_by_map(n, cp, ri, map, v);
        v[(size_t)k] = keep;
        if (want < 0 || want != got) return 6;
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: %s patterns.txt\n", argv[0]); return 64; }
    std::ifstream in(argv[1]);
    if (!in) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 65; }
    int64_t n, nnz; int count = 0;
    while (in >> n >> nnz) {
        std::vector<int64_t> cp((size_t)n + 1), ri((size_t)nnz);
        for (auto& x : cp) in >> x;
        for (auto& x : ri) in >> x;
        if (!in || cp[(size_t)n] != nnz) { std::fprintf(stderr, "pattern %d: malformed input\n", count); return 66; }
        const int rc = check(n, cp, ri);
        if (rc != 0) { std::fprintf(stderr, "pattern %d (n = %lld, %lld entries): check %d failed\n", count, (long long)n, (long long)nnz, rc); return 1; }
        ++count;
    }
    std::printf("%d patterns: partner map == brute force, decision == csc_asymmetry\n", count);
    return count > 0 ? 0 : 67;
}
