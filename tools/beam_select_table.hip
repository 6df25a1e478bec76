// The beam search's queue selection (csrc/lrg_beam_select.h, the function lrg_beam_advance_kernel calls) over a fixed table of
// cases, on the host: no kernel, no HIP call.  One line per case,
//     name|ml|beam_width|search_width|updated,...|size,...|score,...|best,...|kept,...
// which tests/test_beam_select.py checks against Python's sorted() (the reference's own selection, test_beam_search.py:282).
// With a file name as its argument the cases come from that file instead, one per line: name|ml|beam_width|search_width|updated,...|size,...|score,...
// (the scores only under ml; "-inf" is read as such) -- tests/test_beam_rooms_host.py hands it the 64-slot patterns of the GPU tests.
// A host sanitizer build of this program (-Xarch_host -fsanitize=address,undefined) is where the function's index arithmetic is checked.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>
#include "../learn_region_grow_amd/csrc/lrg_beam_select.h"

struct Case {
    const char *name;
    int ml, bw, sw;
    std::vector<int> updated, size;
    std::vector<double> score;
};

static void run(const Case &c) {
    const int n = (int)c.updated.size();
    // exactly beam_width entries each, on the heap: a write past the end is the sanitizer's to see
    std::vector<int> best(c.bw, -7), kept(c.bw, -7);
    std::vector<double> score = c.score;
    if (!c.ml) { score.resize(n); for (int i = 0; i < n; ++i) score[i] = (double)c.size[i]; }
    int nb = -1;
    const int nk = lrg_beam_select(n, c.updated.data(), c.size.data(), score.data(), c.ml, c.bw, best.data(), &nb, kept.data());
    std::printf("%s|%d|%d|%d|", c.name, c.ml, c.bw, c.sw);
    for (int i = 0; i < n; ++i) std::printf("%s%d", i ? "," : "", c.updated[i]);
    std::printf("|");
    for (int i = 0; i < n; ++i) std::printf("%s%d", i ? "," : "", c.size[i]);
    std::printf("|");
    for (int i = 0; i < n; ++i) std::printf("%s%.17g", i ? "," : "", score[i]);
    std::printf("|");
    for (int i = 0; i < nb; ++i) std::printf("%s%d", i ? "," : "", best[i]);
    std::printf("|");
    for (int i = 0; i < nk; ++i) std::printf("%s%d", i ? "," : "", kept[i]);
    std::printf("\n");
}

static std::vector<std::string> split(const std::string &s, char sep) {
    std::vector<std::string> out;
    std::string item;
    std::istringstream in(s);
    while (std::getline(in, item, sep)) out.push_back(item);
    if (!s.empty() && s.back() == sep) out.push_back("");
    return out;
}

static int run_file(const char *path) {
    std::ifstream in(path);
    if (!in) { std::fprintf(stderr, "cannot read %s\n", path); return 2; }
    std::string line;
    while (std::getline(in, line)) {
        if (line.empty()) continue;
        const std::vector<std::string> f = split(line, '|');
        if (f.size() != 7) { std::fprintf(stderr, "bad line: %s\n", line.c_str()); return 2; }
        Case c{f[0].c_str(), std::atoi(f[1].c_str()), std::atoi(f[2].c_str()), std::atoi(f[3].c_str()), {}, {}, {}};
        for (const std::string &v : split(f[4], ',')) c.updated.push_back(std::atoi(v.c_str()));
        for (const std::string &v : split(f[5], ',')) c.size.push_back(std::atoi(v.c_str()));
        if (c.ml) for (const std::string &v : split(f[6], ',')) c.score.push_back(std::strtod(v.c_str(), nullptr));
        if (c.bw < 1 || c.bw > LRG_BEAM_MAXQ || c.sw < 1 || c.bw * c.sw > 64 || c.updated.size() > 64 || c.size.size() != c.updated.size() ||
            (c.ml && c.score.size() != c.updated.size())) {
            std::fprintf(stderr, "bad case: %s\n", line.c_str());
            return 2;
        }
        run(c);
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1) return run_file(argv[1]);
    const double inf = INFINITY;
    std::vector<Case> cases = {
        // --scoring np: ties in size keep child order (a stable sort); an unchanged child (0) and a parent without neighbours (-1) never enter
        {"np_size_ties", 0, 3, 3, {1, 1, 0, 1, 1, -1, 1, 1, 1}, {5, 9, 99, 9, 5, 0, 9, 2, 9}, {}},
        {"np_empties_last", 0, 3, 2, {1, 1, 1, 1}, {0, 4, 0, 4}, {}},
        // --scoring ml
        {"ml_exact_tie", 1, 2, 2, {1, 1, 1, 1}, {3, 4, 5, 6}, {-1.5, -0.25, -0.25, -0.25}},
        {"ml_minus_inf", 1, 3, 2, {1, 1, 1, 1}, {3, 4, 5, 6}, {-inf, -2.0, -inf, -inf}},
        {"ml_all_minus_inf", 1, 2, 3, {1, 1, 1, 0, 1, 1}, {3, 4, 5, 6, 7, 8}, {-inf, -inf, -inf, -inf, -inf, -inf}},
        {"ml_more_than_beam", 1, 2, 4, {1, 1, 1, 1, 1, 1, 1, 1}, {1, 2, 3, 4, 5, 6, 7, 8}, {-8, -1, -7, -2, -6, -3, -5, -4}},
        // an emptied mask with the highest score takes a place among the best beam_width and is dropped only then: the queue is shorter
        {"ml_empty_mask_on_top", 1, 2, 2, {1, 1, 1, 1}, {0, 7, 8, 9}, {-0.1, -0.2, -0.3, -0.4}},
        {"ml_only_empties_survive", 1, 2, 2, {1, 1, 1, 1}, {0, 0, 8, 9}, {-0.1, -0.2, -0.3, -0.4}},
        {"no_candidate_np", 0, 3, 3, {0, 0, -1, -1, -1, 0}, {4, 4, 0, 0, 0, 4}, {}},
        {"no_candidate_ml", 1, 3, 3, {0, 0, 0}, {4, 4, 4}, {-1, -2, -3}},
        {"no_children", 1, 3, 3, {}, {}, {}},
        {"beam_1", 1, 1, 3, {1, 1, 1}, {2, 3, 4}, {-3, -1, -1}},
    };
    {   // beam_width = 16, search_width = 4: all 64 children, scores with many ties
        Case c{"bw16_sw4_ml", 1, 16, 4, {}, {}, {}};
        Case d{"bw16_sw4_np", 0, 16, 4, {}, {}, {}};
        for (int i = 0; i < 64; ++i) {
            c.updated.push_back(i % 5 != 0); c.size.push_back(i % 11 == 3 ? 0 : 1 + (i * 37) % 9); c.score.push_back(-(double)((i * 29) % 13) / 8.0);
            d.updated.push_back(i % 7 != 0); d.size.push_back((i * 37) % 9);
        }
        cases.push_back(c);
        cases.push_back(d);
    }
    // a fixed pseudo-random sweep: few distinct keys, so ties and empties are the rule
    static char names[400][24];
    uint32_t x = 12345u;
    auto next = [&x]() { x = x * 1664525u + 1013904223u; return x >> 8; };
    for (int k = 0; k < 400; ++k) {
        std::snprintf(names[k], sizeof names[k], "sweep_%03d", k);
        const int bw = 1 + (int)(next() % 16), sw = 1 + (int)(next() % (64 / bw)), nq = 1 + (int)(next() % bw);
        Case c{names[k], (int)(next() & 1), bw, sw, {}, {}, {}};
        for (int i = 0; i < nq * sw; ++i) {
            c.updated.push_back((int)(next() % 4) - 1 > 0 ? 1 : (int)(next() % 2) - 1);
            c.size.push_back((int)(next() % 5));
            const int s = (int)(next() % 7);
            c.score.push_back(s == 6 ? -inf : -(double)s / 4.0);
        }
        cases.push_back(c);
    }
    for (const Case &c : cases) run(c);
    return 0;
}
