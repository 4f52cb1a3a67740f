// trial_inputs_check.cpp -- the order-defining arithmetic of csrc/trial_inputs.hpp on the host, without HIP: a stand-alone program
// (tests/test_trial_inputs_host.py compiles it, with AddressSanitizer and UBSan where the compiler has them, and runs it).
// It walks a scenario the way k_trial_inputs does -- the twist in its three phases, the 64 lanes of a phase emulated as "all lanes
// read, then all lanes write"; a lane per pair; the centre, the norms and NumPy's pairwise sum from the header's own functions --
// and prints, per output array, the two digest words of scripts/make_golden_wide.py, which pytest compares with the fixture.
//   line:  <case> <energy index> <seed> <array index> <digest 0> <digest 1>      (case -1: the fixture's small case, in full:
//   line:  small <seed index> <array index> <element> <bit pattern>)
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "trial_inputs.hpp"

using namespace dpilqr;

namespace {

struct Trial {
    std::vector<double> x0, xf, Ua, Ub;
};

void twist_in_phases(uint32_t* mt) {
    for (int p = 0; p < 3; ++p) {
        const int lo = mt_phase_lo(p), hi = mt_phase_hi(p);
        uint32_t held[4 * 64];      // four words a lane, as the kernel holds them
        for (int lane = 0; lane < 64; ++lane)
            for (int q = 0; q < 4; ++q) {
                const int i = lo + lane + 64 * q;
                held[q * 64 + lane] = i < hi ? mt_twist_word(mt, i) : 0u;
            }
        for (int lane = 0; lane < 64; ++lane)
            for (int q = 0; q < 4; ++q) {
                const int i = lo + lane + 64 * q;
                if (i < hi) mt[i] = held[q * 64 + lane];
            }
    }
}

Trial draw(uint32_t seed, int k, int n_s, int n_d, double var, double energy, int n_warm, int N, int n_u, double warm_scale) {
    std::vector<uint32_t> mt(kMtWords);
    mt[0] = seed;
    for (int i = 1; i < kMtWords; ++i) mt[i] = mt_seed_next(mt[i - 1], i);
    const int n_pos = k * n_d;
    const int64_t n_setup = trial_setup_doubles(k, n_d), n_row = (int64_t)N * n_u, total = trial_doubles(k, n_d, n_warm, N, n_u);
    std::vector<double> pos((size_t)n_setup), nrm((size_t)2 * k);
    Trial t;
    t.Ua.assign(n_warm >= 1 ? (size_t)n_row : 0, -1.0);
    t.Ub.assign(n_warm >= 2 ? (size_t)n_row : 0, -1.0);
    int64_t twists = 0;
    for (int64_t base = 0; base < total; base += kMtPairs, ++twists) {
        twist_in_phases(mt.data());
        for (int j = 0; j < kMtPairs; ++j) {
            const int64_t d = base + j;
            if (d >= total) break;
            const double u = mt_pair_double(mt.data(), j);
            if (d < n_setup) pos[(size_t)d] = trial_position(u, var);
            else if (d - n_setup < n_row) t.Ua[(size_t)(d - n_setup)] = trial_warm(u, warm_scale);
            else t.Ub[(size_t)(d - n_setup - n_row)] = trial_warm(u, warm_scale);
        }
    }
    if (twists != trial_twists(k, n_d, n_warm, N, n_u)) { std::printf("twist count\n"); std::exit(1); }
    if (energy != 0.0) {
        double ctr[8];
        for (int lane = 0; lane < 2 * n_d; ++lane) {
            const int which = lane / n_d, c = lane - which * n_d;
            ctr[which * 3 + c] = trial_centre(pos.data() + which * n_pos, k, n_d, c);
        }
        for (int e = 0; e < 2 * n_pos; ++e) {
            const int which = e >= n_pos ? 1 : 0, c = (e - which * n_pos) % n_d;
            pos[e] -= ctr[which * 3 + c];
        }
        for (int a = 0; a < 2 * k; ++a) nrm[a] = trial_norm(pos.data() + a * n_d, n_d);
        for (int lane = 0; lane < 2; ++lane) ctr[6 + lane] = energy / numpy_pairwise_sum_wide(nrm.data() + lane * k, k);
        for (int e = 0; e < 2 * n_pos; ++e) pos[e] *= ctr[6 + (e >= n_pos ? 1 : 0)];
    }
    t.x0.assign((size_t)k * n_s, 0.0);
    t.xf.assign((size_t)k * n_s, 0.0);
    for (int q = 0; q < k * n_s; ++q) {
        const int a = q / n_s, c = q - a * n_s;
        if (c < n_d) { t.x0[q] = pos[a * n_d + c]; t.xf[q] = pos[n_pos + a * n_d + c]; }
    }
    return t;
}

uint64_t bits_of(double v) { uint64_t b; std::memcpy(&b, &v, sizeof b); return b; }

void print_digest(int ci, int ei, long long seed, int ai, const std::vector<double>& a) {
    uint64_t d0 = 0, d1 = 0;
    for (size_t i = 0; i < a.size(); ++i) { const uint64_t b = bits_of(a[i]); d0 += b; d1 += b * (2 * (uint64_t)i + 1); }
    std::printf("%d %d %lld %d %" PRIu64 " %" PRIu64 "\n", ci, ei, seed, ai, d0, d1);
}

}  // namespace

int main() {
    // the split of NumPy's pairwise sum and the phase bounds, stated independently of the header
    if (numpy_split(129) != 64 || numpy_split(255) != 120 || numpy_split(135) != 64 || numpy_split(256) != 128) return 2;
    if (mt_phase_hi(0) != 227 || mt_phase_lo(1) != 227 || mt_phase_hi(1) != 454 || mt_phase_lo(2) != 454 || mt_phase_hi(2) != 624) return 3;
    const int cases[4][3] = {{65, 4, 2}, {129, 4, 2}, {255, 6, 3}, {256, 6, 3}};
    const int N = 3;
    for (int ci = 0; ci < 4; ++ci) {
        const int k = cases[ci][0], n_s = cases[ci][1], n_d = cases[ci][2], n_u = k * (n_s == 6 ? 3 : 2);
        for (int ei = 0; ei < 2; ++ei)
            for (int seed = 0; seed < 5; ++seed) {
                const Trial t = draw((uint32_t)seed, k, n_s, n_d, k / 2.0, ei == 0 ? 10.0 * k / 5 : 0.0, 2, N, n_u, 0.01);
                print_digest(ci, ei, seed, 0, t.x0); print_digest(ci, ei, seed, 1, t.xf);
                print_digest(ci, ei, seed, 2, t.Ua); print_digest(ci, ei, seed, 3, t.Ub);
            }
    }
    const uint32_t small_seeds[4] = {7u, 3u, 4294967295u, 100u};
    for (int si = 0; si < 4; ++si) {
        const Trial t = draw(small_seeds[si], 5, 4, 2, 2.5, 10.0, 2, N, 10, 0.01);
        const std::vector<double>* arrays[4] = {&t.x0, &t.xf, &t.Ua, &t.Ub};
        for (int ai = 0; ai < 4; ++ai)
            for (size_t i = 0; i < arrays[ai]->size(); ++i)
                std::printf("small %d %d %zu %" PRIu64 "\n", si, ai, i, bits_of((*arrays[ai])[i]));
    }
    return 0;
}
