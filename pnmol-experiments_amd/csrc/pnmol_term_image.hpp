// pnmol_term_image.hpp -- the stencil image a nonlinear term needs (pnmol_reaction.hip), built on the host.  Host only: no HIP
// call, no pnmol_filter; tests/term_image_check.cpp includes nothing else.
//
// An ELL image is column-major: slot e of row i sits at [e * mp + i], columns -1 behind a row's entries.  The image of a term is
// the base image (the operator given at creation) with further columns in every PDE row, so that the linearisation kernel finds a
// slot for each entry of the Jacobian it writes.
#pragma once
#include <algorithm>
#include <utility>
#include <vector>

struct TermImageHost {
    std::vector<int> col;     // w x mp, -1 padded
    std::vector<double> val;  // w x mp: the base value, 0 in an added slot
    std::vector<double> g;    // w x mp: the value that came with the slot's column (0 for a base-only column); empty without a G plane
    std::vector<int> slot;    // C x mp: [k * mp + i] = slot of column k N + i % N in PDE row i (N = d / C)
    int w = 1;                // the widest row, at least 1
};

// bcol / bval: the base image, bw slots wide.  Rows i >= d (boundary rows, padding) are copied as they are.  For a PDE row i < d,
// extra(i, out) appends the (column, G value) pairs the term adds; a column the row holds already keeps its value.  Slots are in
// ascending column order, as build_ell leaves them.  C = 1 gives the table of the diagonal slots.
template <class Extra>
TermImageHost build_term_image(const std::vector<int>& bcol, const std::vector<double>& bval, int bw, int d, int mp, int C,
                               bool with_g, Extra&& extra) {
    struct Entry {
        int col;
        double val, g;
    };
    const int N = d / C;
    std::vector<std::vector<Entry>> rows((size_t)mp);
    std::vector<std::pair<int, double>> add;
    TermImageHost img;
    for (int i = 0; i < mp; ++i) {
        auto& row = rows[i];
        for (int e = 0; e < bw; ++e)
            if (bcol[(size_t)e * mp + i] >= 0) row.push_back({bcol[(size_t)e * mp + i], bval[(size_t)e * mp + i], 0.0});
        if (i < d) {
            add.clear();
            extra(i, add);
            for (const auto& cg : add) {
                auto at = std::find_if(row.begin(), row.end(), [&](const Entry& x) { return x.col == cg.first; });
                if (at == row.end()) row.push_back({cg.first, 0.0, cg.second});
                else at->g = cg.second;
            }
            std::stable_sort(row.begin(), row.end(), [](const Entry& x, const Entry& y) { return x.col < y.col; });
        }
        img.w = std::max(img.w, (int)row.size());
    }
    img.col.assign((size_t)img.w * mp, -1);
    img.val.assign((size_t)img.w * mp, 0.0);
    if (with_g) img.g.assign((size_t)img.w * mp, 0.0);
    img.slot.assign((size_t)C * mp, 0);
    for (int i = 0; i < mp; ++i)
        for (int e = 0; e < (int)rows[i].size(); ++e) {
            const Entry& x = rows[i][e];
            img.col[(size_t)e * mp + i] = x.col;
            img.val[(size_t)e * mp + i] = x.val;
            if (with_g) img.g[(size_t)e * mp + i] = x.g;
            if (i < d && x.col % N == i % N && x.col / N < C) img.slot[(size_t)(x.col / N) * mp + i] = e;
        }
    return img;
}

// A coupled system of C species (row i = c N + j): a slot for each same-point column k N + j, and the (C, mp) table of those slots.
inline TermImageHost system_term_image(const std::vector<int>& bcol, const std::vector<double>& bval, int bw, int d, int mp, int C) {
    const int N = d / C;
    return build_term_image(bcol, bval, bw, d, mp, C, false, [=](int i, std::vector<std::pair<int, double>>& out) {
        for (int k = 0; k < C; ++k) out.emplace_back(k * N + i % N, 0.0);
    });
}

// A convection term with the stencil operator G (d x d, row major): the union of the base image and G, G's value beside every
// slot, and the (1, mp) table of the diagonal slots.
inline TermImageHost convection_term_image(const std::vector<int>& bcol, const std::vector<double>& bval, int bw, int d, int mp,
                                           const double* G) {
    return build_term_image(bcol, bval, bw, d, mp, 1, true, [=](int i, std::vector<std::pair<int, double>>& out) {
        for (int k = 0; k < d; ++k)
            if (G[(size_t)i * d + k] != 0.0) out.emplace_back(k, G[(size_t)i * d + k]);
    });
}
