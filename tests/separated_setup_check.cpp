// separated_setup_check.cpp -- the order-defining arithmetic of csrc/separated_setup.hpp on the host, without HIP: a stand-alone
// program (tests/test_separated_setup_host.py compiles it, with AddressSanitizer and UBSan where the compiler has them, and runs it).
// It draws a trial's raw positions from the header's own MT19937 pieces, then walks a point set the way k_setup_separate does --
// the 256 threads of a round emulated as "all threads read, then all threads write": the centre, a flag per point, the one word
// they raise, the push of the flagged points; then normalize_energy from the header's functions -- and prints, per record of
// tests/golden/g12_separated_setup.npz (scripts/make_golden_separated.py: the same cases in the same order),
//   line:  <record> <array: 0 x0, 1 xf> <digest 0> <digest 1> <rounds>
//   line:  full <record> <array> <element> <bit pattern>                      (k <= 8)
// and, for the cap, one record again under max_iter = 1:
//   line:  cap <record> <array> <digest 0> <digest 1> <rounds>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "separated_setup.hpp"

using namespace dpilqr;

namespace {

// the first 2 k n_d doubles of np.random.seed(seed)'s stream, as positions (the twist in its three phases: read all, write all)
std::vector<double> raw_draws(uint32_t seed, int k, int n_d, double var) {
    std::vector<uint32_t> mt(kMtWords), held(kMtWords);
    mt[0] = seed;
    for (int i = 1; i < kMtWords; ++i) mt[i] = mt_seed_next(mt[i - 1], i);
    const int64_t total = trial_setup_doubles(k, n_d);
    std::vector<double> pos((size_t)total);
    for (int64_t base = 0; base < total; base += kMtPairs) {
        for (int p = 0; p < 3; ++p) {
            for (int i = mt_phase_lo(p); i < mt_phase_hi(p); ++i) held[i] = mt_twist_word(mt.data(), i);
            for (int i = mt_phase_lo(p); i < mt_phase_hi(p); ++i) mt[i] = held[i];
        }
        for (int j = 0; j < kMtPairs && base + j < total; ++j) pos[(size_t)(base + j)] = trial_position(mt_pair_double(mt.data(), j), var);
    }
    return pos;
}

// one point set through k_setup_separate's loop and normalisation; returns the rounds (-1: the cap)
int separate(double* pos, int k, int n_d, double rel_dist, double energy, int max_iter) {
    const double push = sep_push(k);
    double ctr[4];
    std::vector<char> flag((size_t)kSepThreads);
    std::vector<double> next((size_t)k * n_d), nrm((size_t)k);
    int rounds = -1;
    for (int it = 0; it < max_iter; ++it) {
        int any = 0;
        for (int tid = 0; tid < n_d; ++tid) ctr[tid] = sep_centre(pos, k, n_d, tid);
        for (int tid = 0; tid < kSepThreads; ++tid) {
            flag[tid] = tid < k && sep_flag(pos, k, n_d, tid, rel_dist);
            if (flag[tid]) any = 1;
        }
        if (!any) { rounds = it + 1; break; }
        for (int tid = 0; tid < k; ++tid)
            for (int c = 0; c < n_d; ++c)
                next[tid * n_d + c] = flag[tid] ? sep_pushed(pos[tid * n_d + c], ctr[c], push) : pos[tid * n_d + c];
        for (int e = 0; e < k * n_d; ++e) pos[e] = next[e];
    }
    if (rounds > 0 && energy != 0.0) {      // the centre: the last round's, which moved nothing
        for (int e = 0; e < k * n_d; ++e) pos[e] -= ctr[e % n_d];
        for (int tid = 0; tid < k; ++tid) nrm[tid] = trial_norm(pos + tid * n_d, n_d);
        ctr[3] = energy / numpy_pairwise_sum_wide(nrm.data(), k);
        for (int e = 0; e < k * n_d; ++e) pos[e] *= ctr[3];
    }
    return rounds;
}

uint64_t bits_of(double v) { uint64_t b; std::memcpy(&b, &v, sizeof b); return b; }

// the row [k * n_s] of a set: positions in the first n_d states of an agent, zeros behind
std::vector<double> row_of(const double* pos, int k, int n_s, int n_d) {
    std::vector<double> row((size_t)k * n_s, 0.0);
    for (int a = 0; a < k; ++a)
        for (int c = 0; c < n_d; ++c) row[a * n_s + c] = pos[a * n_d + c];
    return row;
}

void print_digest(const char* head, int rec, int ai, const std::vector<double>& a, int rounds) {
    uint64_t d0 = 0, d1 = 0;
    for (size_t i = 0; i < a.size(); ++i) { const uint64_t b = bits_of(a[i]); d0 += b; d1 += b * (2 * (uint64_t)i + 1); }
    std::printf("%s%d %d %" PRIu64 " %" PRIu64 " %d\n", head, rec, ai, d0, d1, rounds);
}

struct Case { int k, n_d, n_s; double rel_dist, var; };

}  // namespace

int main() {
    if (bits_of(sep_push(3)) != bits_of(0.30000000000000004) || sep_dist_dims(3) != 2 || sep_dist_dims(1) != 1) return 2;
    {      // the one-loop pairwise sum is numpy_pairwise_sum_wide, for every length the kernel can give it
        const std::vector<double> a = raw_draws(12345u, kTrialMaxAgents, 1, 1000.0);
        for (int n = 1; n <= kTrialMaxAgents; ++n)
            if (bits_of(sep_pairwise_sum(a.data(), n)) != bits_of(numpy_pairwise_sum_wide(a.data(), n))) return 3;
    }
    const Case cases[13] = {{2, 2, 4, 2.0, 1.0},       {3, 2, 4, 3.0, 1.5},       {3, 3, 6, 3.0, 1.5},       {5, 2, 4, 5.0, 2.5},
                            {7, 2, 4, 2.0, 3.5},       {24, 2, 4, 24.0, 12.0},    {64, 2, 4, 64.0, 32.0},    {65, 2, 4, 65.0, 32.5},
                            {129, 2, 4, 129.0, 64.5},  {130, 3, 6, 130.0, 65.0},  {256, 2, 4, 256.0, 128.0}, {256, 2, 4, 8.0, 128.0},
                            {130, 1, 4, 24.0, 65.0}};
    int rec = 0;
    for (const Case& c : cases)
        for (int ei = 0; ei < 2; ++ei)
            for (int seed = 0; seed < 3; ++seed, ++rec) {
                const double energy = ei == 0 ? 0.0 : 5.0 * c.k;
                const int n_pos = c.k * c.n_d;
                for (int cap = 0; cap < (rec == 66 ? 2 : 1); ++cap) {      // record 66: k = 256, rel_dist = 8, also under max_iter = 1
                    std::vector<double> pos = raw_draws((uint32_t)seed, c.k, c.n_d, c.var);
                    for (int ai = 0; ai < 2; ++ai) {
                        const int rounds = separate(pos.data() + ai * n_pos, c.k, c.n_d, c.rel_dist, energy, cap ? 1 : 256);
                        const std::vector<double> row = row_of(pos.data() + ai * n_pos, c.k, c.n_s, c.n_d);
                        print_digest(cap ? "cap " : "", rec, ai, row, rounds);
                        if (c.k <= 8 && !cap)
                            for (size_t i = 0; i < row.size(); ++i) std::printf("full %d %d %zu %" PRIu64 "\n", rec, ai, i, bits_of(row[i]));
                    }
                }
            }
    return 0;
}
