// Prints, per state family and agent count, what the launchers of the large-cluster and the staged forward pass decide from sizes
// alone at ten candidates (tests/test_linesearch_cases.py): forward_on_pipe, the three LDS sizes, kMaxStage, kMaxLds.  Host only.
#include <cstdio>
#include "launch.hpp"
#include "forward.hpp"
#include "riccati_big.hpp"
using namespace dpilqr;
int main() {
    const int fam[5][2] = {{3, 2}, {4, 2}, {5, 2}, {6, 3}, {12, 4}};
    for (auto& f : fam)
        for (int k = 1; k <= 25; ++k) {
            const int n = k * f[0], m = k * f[1], threads = ((k * 10 + 63) / 64) * 64;
            std::printf("%d %d %d %d %zu %zu %zu %d %d\n", f[0], f[1], k, (int)forward_on_pipe(n, m, k, threads, 10),
                        forward_lds_bytes(n, m, k, 10, false), forward_lds_bytes(n, m, k, 10, true),
                        sizeof(double) * (size_t)BigLds(k, f[0], f[1]).total, kMaxStage, kMaxLds);
        }
    return 0;
}
