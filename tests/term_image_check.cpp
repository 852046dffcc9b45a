// The host-side image builder of the nonlinear terms (csrc/pnmol_term_image.hpp) on its own: built with
// -fsanitize=address,undefined and run by tests/test_term_image_host.py.  Every case checks the invariants the linearisation
// kernels rely on and the program exits non-zero on the first violation.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>

#include "pnmol_term_image.hpp"

namespace {

constexpr int MP = 32;

#define REQUIRE(cond)                                                                  \
    do {                                                                               \
        if (!(cond)) {                                                                 \
            std::fprintf(stderr, "%s: line %d: %s\n", g_case, __LINE__, #cond);        \
            std::exit(1);                                                              \
        }                                                                              \
    } while (0)
const char* g_case = "";

struct Base {
    int d = 0, bw = 0;
    std::vector<int> col;
    std::vector<double> val;
    std::vector<std::map<int, double>> rows;  // the same, row by row
};

// C species on N points: a tridiagonal block per species (-L's values, all distinct and non-zero; the diagonal of every row but
// the first of a block is not in slot 0) and two boundary rows of three entries
Base tridiagonal(int N, int C) {
    Base b;
    b.d = C * N;
    b.rows.resize(MP);
    for (int i = 0; i < b.d; ++i)
        for (int k = i - 1; k <= i + 1; ++k)
            if (k >= 0 && k < b.d && k / N == i / N) b.rows[i][k] = 100.0 * (i + 1) + k + 0.5;
    b.rows[b.d] = {{0, 1.5}, {1, -2.0}, {2, 0.5}};
    b.rows[b.d + 1] = {{b.d - 3, 0.5}, {b.d - 2, -2.0}, {b.d - 1, 1.5}};
    for (const auto& r : b.rows) b.bw = std::max(b.bw, (int)r.size());
    b.col.assign((size_t)b.bw * MP, -1);
    b.val.assign((size_t)b.bw * MP, 0.0);
    for (int i = 0; i < MP; ++i) {
        int e = 0;
        for (const auto& cv : b.rows[i]) b.col[(size_t)e * MP + i] = cv.first, b.val[(size_t)e++ * MP + i] = cv.second;
    }
    return b;
}

// `extra`: the columns the term adds to each PDE row; G (d x d) or null
void check(const Base& b, const TermImageHost& im, int C, const std::vector<std::set<int>>& extra, const double* G) {
    const int d = b.d, N = d / C;
    REQUIRE(im.w >= 1 && im.col.size() == (size_t)im.w * MP && im.val.size() == im.col.size());
    REQUIRE(im.slot.size() == (size_t)C * MP && im.g.size() == (G ? im.col.size() : 0));
    int widest = 1;
    for (int i = 0; i < MP; ++i) {
        int n = 0;
        while (n < im.w && im.col[(size_t)n * MP + i] >= 0) ++n;
        widest = std::max(widest, n);
        std::set<int> want;
        for (const auto& cv : b.rows[i]) want.insert(cv.first);
        if (i < d) want.insert(extra[i].begin(), extra[i].end());
        REQUIRE(n == (int)want.size());
        for (int e = 0; e < im.w; ++e) {
            const size_t at = (size_t)e * MP + i;
            if (e >= n) {  // packed to the front, -1 and zeros behind
                REQUIRE(im.col[at] == -1 && im.val[at] == 0.0 && (!G || im.g[at] == 0.0));
                continue;
            }
            const int col = im.col[at];
            REQUIRE(want.count(col) == 1);
            if (e > 0) REQUIRE(im.col[at - MP] < col);  // ascending
            const auto in_base = b.rows[i].find(col);
            REQUIRE(im.val[at] == (in_base == b.rows[i].end() ? 0.0 : in_base->second));
            if (G) REQUIRE(im.g[at] == (i < d ? G[(size_t)i * d + col] : 0.0));
            if (i >= d) REQUIRE(e < b.bw && col == b.col[at] && im.val[at] == b.val[at]);  // untouched, slot for slot
        }
    }
    REQUIRE(im.w == widest);
    for (int i = 0; i < d; ++i)
        for (int k = 0; k < C; ++k) {
            const int e = im.slot[(size_t)k * MP + i];
            REQUIRE(e >= 0 && e < im.w && im.col[(size_t)e * MP + i] == k * N + i % N);
        }
}

void system_case(const char* name, int C) {
    g_case = name;
    const int N = 5;
    const Base b = tridiagonal(N, C);
    std::vector<std::set<int>> extra(b.d);
    for (int i = 0; i < b.d; ++i)
        for (int k = 0; k < C; ++k) extra[i].insert(k * N + i % N);
    const TermImageHost im = system_term_image(b.col, b.val, b.bw, b.d, MP, C);
    check(b, im, C, extra, nullptr);
    REQUIRE(im.w == 3 + C - 1);  // an interior row: its three entries and the other species' same-point columns
}

void convection_case(const char* name, bool zero) {
    g_case = name;
    const int N = 5;
    const Base b = tridiagonal(N, 1);
    std::vector<double> G((size_t)N * N, 0.0);
    std::vector<std::set<int>> extra(N);
    bool beyond_base = false;
    for (int i = 0; i < N && !zero; ++i)
        for (int k = std::max(0, i - 2); k <= std::min(N - 1, i + 2); ++k) {
            if (k == i) continue;  // (a gradient stencil has no centre weight: the diagonal slot carries G = 0)
            G[(size_t)i * N + k] = (k - i) * 0.25 + 0.01 * i;
            extra[i].insert(k);
            beyond_base = beyond_base || b.rows[i].count(k) == 0;
        }
    REQUIRE(zero || beyond_base);  // a G entry in a column the base row lacks
    const TermImageHost im = convection_term_image(b.col, b.val, b.bw, N, MP, G.data());
    check(b, im, 1, extra, G.data());
    if (zero) {
        REQUIRE(im.w == b.bw && im.col == b.col && im.val == b.val);
    } else {
        REQUIRE(im.w == 5);
        REQUIRE(im.slot[2] == 2 && im.slot[0] == 0);  // row 2 holds columns 0..4, row 0 columns 0..2
    }
}

}  // namespace

int main() {
    g_case = "base";
    const Base b = tridiagonal(5, 1);
    REQUIRE(b.bw == 3 && b.col[(size_t)0 * MP + 2] == 1 && b.col[(size_t)1 * MP + 2] == 2);  // row 2: the diagonal sits in slot 1
    system_case("system C=2", 2);
    system_case("system C=3", 3);
    convection_case("convection, 5-point G", false);
    convection_case("convection, G = 0", true);
    std::printf("term image: ok\n");
    return 0;
}
