// admit_order_check.cpp -- stand-alone check of the host side of csrc/admit_order.hpp (tests/test_admit_order_host.py compiles and
// runs it; no HIP, no GPU).  For every list length, CU count and sweep tier:
//   * SweepDeal::slot enumerates every list position 0..n-1 exactly once over the workgroups (round, cu) and their wavefronts;
//   * order_position is a permutation of 0..n-1 for both orders, the identity for the spread order;
//   * grouped: the positions of each sweep workgroup receive consecutive ranks, and the workgroups take them in launch order;
//   * order_class is monotone and stays below kOrderClasses.
// Prints one line per failure and "ok <cases>" at the end; the exit status is the number of failures (capped).
#include <cstdio>
#include <vector>

#include "admit_order.hpp"

using namespace dpilqr;

int main() {
    const int ns[] = {1, 2, 63, 64, 1024, 1025, 2048, 2049, 3071, 3072, 3073, 6144, 6145, 20480};
    const int cus[] = {1, 8, 256};
    const int tiers[] = {4, 8, 12};
    int failures = 0, cases = 0;
    auto bad = [&](const char* what, int n, int c, int w, int at) {
        if (failures < 20) std::printf("FAIL %s: n=%d n_cus=%d waves=%d at %d\n", what, n, c, w, at);
        ++failures;
    };
    for (int n : ns)
        for (int c : cus)
            for (int w : tiers) {
                ++cases;
                const SweepDeal D(n, c, w);
                // the sweep's dealing covers every position once
                std::vector<int> seen(n, 0);
                for (int r = 0; r < D.rounds; ++r)
                    for (int cu = 0; cu < c; ++cu)
                        for (int wave = 0; wave < w; ++wave) {
                            const int s = D.slot(r, cu, wave);
                            if (s < -1 || s >= n) { bad("slot out of range", n, c, w, s); continue; }
                            if (s >= 0) ++seen[s];
                        }
                for (int i = 0; i < n; ++i)
                    if (seen[i] != 1) { bad("slot coverage", n, c, w, i); break; }
                // both orders are permutations
                std::vector<int> rank_at(n, -1);
                for (int order : {(int)kOrderSpread, (int)kOrderGrouped}) {
                    std::vector<int> hit(n, 0);
                    for (int r = 0; r < n; ++r) {
                        const int p = order_position(r, D, order);
                        if (p < 0 || p >= n) { bad("position out of range", n, c, w, r); continue; }
                        ++hit[p];
                        if (order == kOrderSpread && p != r) bad("spread is the identity", n, c, w, r);
                        if (order == kOrderGrouped) rank_at[p] = r;
                    }
                    for (int i = 0; i < n; ++i)
                        if (hit[i] != 1) { bad(order == kOrderSpread ? "spread permutation" : "grouped permutation", n, c, w, i); break; }
                }
                // grouped: a workgroup's positions hold consecutive ranks, workgroups in launch order
                int next = 0;
                for (int r = 0; r < D.rounds; ++r)
                    for (int cu = 0; cu < c; ++cu)
                        for (int wave = 0; wave < w; ++wave) {
                            const int s = D.slot(r, cu, wave);
                            if (s < 0 || s >= n) continue;
                            if (rank_at[s] != next) bad("grouped ranks are consecutive per workgroup", n, c, w, s);
                            ++next;
                        }
                if (next != n) bad("grouped covers the list", n, c, w, next);
            }
    for (int T : {1, 6, 50, 62, 63, 64, 200, 4096}) {
        int prev = 0;
        for (int key = 0; key <= T + 1; ++key) {
            const int cl = order_class(key, T);
            if (cl < prev || cl < 0 || cl >= kOrderClasses) bad("order_class", T, 0, 0, key);
            prev = cl;
        }
        if (T + 1 < kOrderClasses && order_class(T + 1, T) != T + 1) bad("order_class keeps small counts", T, 0, 0, T + 1);
    }
    if (!failures) std::printf("ok %d\n", cases);
    return failures > 100 ? 100 : failures;
}
