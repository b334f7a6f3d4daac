// Stand-alone host check of csrc/nuts_rhs_plan.hpp (no GPU, no library): every leaf of every doubling up to depth 12 against the
// definition, and a workspace of kNutsRhsMaxSlots slots filled and read through the plan's row indices as the kernels address it.
// Meant for a sanitizer build:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/cpp/test_nuts_rhs_plan.cpp -o test_nuts_rhs_plan
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../mcmc-date_amd/csrc/nuts_rhs_plan.hpp"

int main()
{
    const int depth = mcd::kNutsMaxDepthLevels;
    const int64_t B = 3, dim = 5;
    std::vector<double> X((size_t)mcd::kNutsRhsMaxSlots * B * dim, -1.0);
    int64_t r = 0, products = 0;
    int largest = 0;
    for (int j = 0; j < depth; ++j)
        for (int i = 0; i < (1 << j); ++i, ++r) {
            int jr = -1, ir = -1;
            mcd::nuts_round_position(r, &jr, &ir);
            if (jr != j || ir != i) return std::printf("round %lld: (%d, %d) != (%d, %d)\n", (long long)r, jr, ir, j, i), 1;
            const mcd::NutsRhsPlan p = mcd::nuts_rhs_plan(j, i);
            int closes = 0;
            for (int k = 1; k <= j; ++k)
                if ((i + 1) % (1 << k) == 0) {
                    if (k != closes + 1) return std::printf("(%d, %d): the closed levels are not 1 .. closes\n", j, i), 1;
                    ++closes;
                }
            const int whole = i + 1 == (1 << j);
            if (p.closes != closes || p.whole != whole || p.count != 1 + closes + whole || p.count > mcd::kNutsRhsMaxSlots)
                return std::printf("(%d, %d): plan %d %d %d\n", j, i, p.closes, p.whole, p.count), 1;
            // the rows of the round: slot s of chain b at (s B + b) dim, written once each, all inside count B rows
            for (int s = 0; s < p.count; ++s)
                for (int64_t b = 0; b < B; ++b)
                    for (int64_t k = 0; k < dim; ++k) X.at((size_t)((s * B + b) * dim + k)) = (double)r;
            for (size_t at = 0; at < (size_t)(p.count * B * dim); ++at)
                if (X[at] != (double)r) return std::printf("(%d, %d): row element %zu not written\n", j, i, at), 1;
            largest = p.count > largest ? p.count : largest;
            products += p.count;
        }
    if (r != ((int64_t)1 << depth) - 1 || largest != mcd::kNutsRhsMaxSlots) return std::printf("rounds %lld, largest %d\n", (long long)r, largest), 1;
    std::printf("ok: %lld rounds, %lld right-hand sides, at most %d per round\n", (long long)r, (long long)products, largest);
    return 0;
}
