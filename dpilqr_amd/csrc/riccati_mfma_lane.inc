// Lane terms of k_riccati_mfma (riccati_mfma.hpp): every per-lane address, record offset and column predicate of the
// sweep, written as a function of `lane` alone, plus the prefetch lambdas that use them.  NOT a stand-alone header: it is
// included inside the kernel body, once for the prologue and once at the top of each phase group of a sweep step, in a
// scope that defines `lane`.
//
// Why a fragment: about sixty of these values are loop invariant, and with two wavefronts per SIMD (up to 256 registers)
// they simply stay in registers.  With three per SIMD (WAVES = 12, 168 registers) the compiler spills them, and a
// scratch reload inside the step waits on vmcnt behind the record prefetch, which serialises the step on HBM latency
// (measured: 2.5x slower).  There `lane` is an opaque copy of the lane id made per phase group (phase_lane<true>), so
// the terms cannot be hoisted: each group recomputes the few it uses (a handful of integer operations against
// thousands of cycles of fp64 work) and nothing is spilled.  For WAVES = 4 / 8 phase_lane is the identity and the
// compiler hoists everything exactly as if the definitions stood before the loop.
    const int g = lane >> 4, c16 = lane & 15;
    // ---- lane terms.  For column tile jt this lane's column is j = 16 jt + c16.
    bool colN[T_NM], colP[T_NM], colNM[T_NM], colLE[T_NM];   // j < n ; j == n ; j < n+m ; j <= n
    int colG[T_NM];                                          // column of [Q_uu | Q_ux | Q_u] (and of UG in the record) holding global column j
#pragma unroll
    for (int jt = 0; jt < T_NM; ++jt) {
        const int j = 16 * jt + c16;
        colN[jt] = j < N; colP[jt] = j == N; colNM[jt] = j < NM; colLE[jt] = j <= N;
        colG[jt] = (j < N) ? M + j : j - N;
    }
    // operand pointers X[g][c16]
    const double* pAB = sAB + g * LAB + c16;
    const double* pP = sP + g * LP + c16;
    const double* pT = sT + g * LT + c16;
    const double* pGuu = sG + g * LG + c16;          // Q_uu columns
    const double* pGux = sG + g * LG + M + c16;      // [Q_ux | Q_u] columns
    const double* pK = sK + g * LK + c16;
    const double* pT3 = sT3 + g * N + c16;
    // D-element pointers: row-major "[i][j]" = buf + g*LD + c16 ; transposed "[j][i]" = buf + c16*LD + g
    double* dTt = sT + c16 * LT + g;                 // T^T[j][i']
    const double* dBt = sAB + c16 * LAB + g;         // B[j][a] sits at [A|B][j][i'] with i' = n + a
    double* dQ = sQ + g * LQ + c16;                  // Q_xx / V [i][j]
    const double* dPt = sP + c16 * LP + g;           // V[j][i]
    const double* dQt = sQ + c16 * LQ + g;           // W[j][i] (the team's tail)
    (void)dQt;
    double* dG = sG + g * LG;                        // + colG[jt]
    double* dT3 = sT3 + g * N + c16;
    double* dMt = sMt + g * LM + c16;                // a2[i][j]
    const double* dMtT = sMt + c16 * LM + g;         // a2[j][i]
    double* dP = sP + g * LP + c16;
    // record offsets of this lane's l-values (row part g*ld + column part), see TileLayout
    const int gLxx = L.oLxx + g * N + c16;           // + 16 jt + (row const) * N
    const int gUG = L.oLuu + g * L.ldUG;             // + colG[jt] + (row const) * ldUG
    const int gLxu = L.oLx + g;                      // [l_x ; l_u][i']
    // [A|B] prefetch -> LDS (16-byte pairs, round-robin over the wavefront; surplus lanes store to sTrash), S3 epilogue patterns
    double* sTrash = lds + C::oEnd;
    double* ab_dst[C::AB_ROUNDS];
    int ab_src[C::AB_ROUNDS];
    int ab_srcp[PAD ? C::AB_ROUNDS : 1][2];   // PAD: record offset of each element of the pair; -1: a padding 0, -2: a padding 1
#pragma unroll
    for (int q = 0; q < C::AB_ROUNDS; ++q) {
        const int e = 2 * (lane + 64 * q);
        const int row = e / NM, col = e - row * NM;
        ab_dst[q] = (e < N * NM) ? sAB + row * LAB + col : sTrash;
        ab_src[q] = (e < N * NM) ? L.oA + e : 0;
        if constexpr (PAD) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int c = col + h;      // NM is even: both elements are in row `row`
                int off = -1;
                if (e < N * NM) {
                    if (c < N) off = (row < n_rec && c < n_rec) ? L.oA + row * L.ldAB + c : (row == c ? -2 : -1);
                    else off = (row < n_rec && c - N < m_rec) ? L.oB + row * L.ldAB + (c - N) : -1;
                }
                ab_srcp[q][h] = off;
            }
        }
    }
    // S3 lane layout.  ROWLU (every size instantiated today): each 16-lane row holds its own copy of the M columns of
    // Q_uu (lanes 0..M-1 of the row) and 16-M of the n+1 right-hand sides, so that a multiplier or a U entry is
    // always in the consuming lane's own row (DPP row broadcast) and all 64 lanes work.  Otherwise: lane = column.
    const int s3_q = ROWLU ? (16 - M) * g + (c16 - M) : lane - M;                 // right-hand side index
    const bool s3_rhs = ROWLU ? (c16 >= M && s3_q < NP) : (lane >= M && lane <= M + N);
    const int s3_col = ROWLU ? (c16 < M ? c16 : min(M + s3_q, M + N)) : (lane < M + N + 1 ? lane : M + N);
    double* s3_k = s3_rhs ? sK + s3_q : sT3;   // sT3 is not live during S3
    const bool s3_lhs = ROWLU ? (c16 < M) : (lane < M);                 // this lane holds a column of Q_uu ...
    const int s3_dg = min(ROWLU ? c16 : lane, M - 1) * (LG + 1);         // ... whose diagonal entry is sG[s3_dg]
    static_assert((M - 1) * LK < MK * N, "S3's masked columns must fit the dead T3 buffer");
    int k_in[K_ROUNDS], k_out[K_ROUNDS];
#pragma unroll
    for (int q = 0; q < K_ROUNDS; ++q) {
        const int e2 = min(lane + 64 * q, K_PAIRS - 1), e = 2 * e2;
        k_out[q] = e;
        k_in[q] = (e / N) * LK + (e % N);
    }
    const int d_idx = min(lane, M - 1);

    // ---- block-diagonal variant (NS > 0): [A|B] of a MultiDynamicalModel is block diagonal (dynamics.py:173-186:
    // uniform_block_diag of the agents' (A_i, B_i)), so column i' of [A|B] has its non-zeros in the NS rows of ONE
    // agent and S1 / S2 need NS terms per output instead of n.  The skipped terms are exact zeros (x + 0*y == x),
    // so the results are those of the dense sum, term for term.  The record is still read in full -- it is the
    // dense plugin format -- only the multiplications by structural zeros are dropped; these two phases run on
    // the vector pipe (NS = 4 rows per block is one MFMA reduction step: a 16-row tile would use 4 of its rows).
    // Lane (ag, sub): agent ag = lane / LPA.  S1: rows i' of agent ag (NS columns of A, NC of B) x CPL columns
    // of [P|p];  S2: RPL rows of T x the NS + NC columns of agent ag.  Idle lanes duplicate a working lane
    // (same addresses, same values), so nothing is predicated.
    const int ag = min(lane / LPA, KA - 1);
    const int sub1 = min(lane - (lane / LPA) * LPA, (NP - 1) / CPL), j0 = CPL * sub1;   // S1 columns j0, j0+1
    const int sub2 = min(lane - (lane / LPA) * LPA, (NM - 1) / RPL);
    const double* bP = sP + NS * ag * LP + j0;                 // P[NS ag + l][j0 ..]
    const double* bABa = sAB + NS * ag * LAB + NS * ag;        // A block row l
    const double* bABb = sAB + NS * ag * LAB + N + NC * ag;    // B block row l
    const double* bBmu[CPL];                                   // B[j][NC ag ..] for the mu B^T term (j < n)
    bool bMuOn[CPL];
#pragma unroll
    for (int c = 0; c < CPL; ++c) { bMuOn[c] = j0 + c < N; bBmu[c] = sAB + min(j0 + c, N - 1) * LAB + N + NC * ag; }
    double* bTa = sT + NS * ag * LTB + j0;                     // T[NS ag + r][j0 ..]   (A^T P rows)
    double* bTb = sT + (N + NC * ag) * LTB + j0;               // T[n + NC ag + r][j0 ..] (B^T P rows)
    const bool bPcol = (j0 == N);                              // this lane holds A^T p, B^T p
    const double* bT2[RPL];                                    // S2: T[i'_r][NS ag ..]
    double* bDa[RPL];                                          // S2 outputs over A's columns: Q_xx row or Q_ux row
    double* bDb[RPL];                                          //            over B's columns: Q_uu row (or dropped)
    int bSa[RPL], bSb[RPL];                                    // record offsets of the matching l-values
#pragma unroll
    for (int r = 0; r < RPL; ++r) {
        const int ip = min(RPL * sub2 + r, NM - 1);
        bT2[r] = sT + ip * LTB + NS * ag;
        if (ip < N) {
            bDa[r] = sQ + ip * LQ + NS * ag; bSa[r] = L.oLxx + ip * N + NS * ag;
            bDb[r] = lds + C::oEnd;          bSb[r] = bSa[r];
        } else {
            bDa[r] = sG + (ip - N) * LG + M + NS * ag; bSa[r] = L.oLux + (ip - N) * L.ldUG + NS * ag;
            bDb[r] = sG + (ip - N) * LG + NC * ag;     bSb[r] = L.oLuu + (ip - N) * L.ldUG + NC * ag;
        }
    }
    const int bSx = L.oLx + NS * ag, bSu = L.oLu + NC * ag;
    // (A/B switch: the records are read once, -DDPILQR_REC_NT loads them with the non-temporal cache policy)
#ifdef DPILQR_REC_NT
#define DPILQR_REC_LD(p) __builtin_nontemporal_load(p)
#else
#define DPILQR_REC_LD(p) (*(p))
#endif
    auto prefetch_bd_l = [&](int t) {
        const double* rec = base + (int64_t)t * L.stride;
#pragma unroll
        for (int r = 0; r < RPL; ++r) {
#pragma unroll
            for (int q = 0; q < NS / 2; ++q) nbL[r][q] = DPILQR_REC_LD(reinterpret_cast<const v2d*>(rec + bSa[r] + 2 * q));
#pragma unroll
            for (int q = 0; q < NC / 2; ++q) nbL[r][NS / 2 + q] = DPILQR_REC_LD(reinterpret_cast<const v2d*>(rec + bSb[r] + 2 * q));
        }
    };
    auto prefetch_bd_x = [&](int t) {
        const double* rec = base + (int64_t)t * L.stride;
#pragma unroll
        for (int q = 0; q < NS / 2; ++q) nbX[q] = DPILQR_REC_LD(reinterpret_cast<const v2d*>(rec + bSx + 2 * q));
#pragma unroll
        for (int q = 0; q < NC / 2; ++q) nbX[NS / 2 + q] = DPILQR_REC_LD(reinterpret_cast<const v2d*>(rec + bSu + 2 * q));
    };

    // ---- prefetch registers (one record ahead), re-filled right after they are consumed.  They mirror the D
    // layout: nL[it][jt][v] is the l-value added to element (it, jt, v) of the S2 product.
    // PAD: a record element by its offset code (>= 0 an offset, -1 a padding zero, -2 a padding one): loaded from a
    // clamped address whatever the code is, then selected
    auto rec_or_pad = [&](const double* rec, int off) {
        const double val = rec[max(off, 0)];
        return off >= 0 ? val : (off == -2 ? 1.0 : 0.0);
    };
    auto prefetch_ab = [&](int t) {
        const double* rec = base + (int64_t)t * L.stride;
        if constexpr (PAD) {
#pragma unroll
            for (int q = 0; q < C::AB_ROUNDS; ++q) nAB[q] = v2d{rec_or_pad(rec, ab_srcp[q][0]), rec_or_pad(rec, ab_srcp[q][1])};
        } else {
#pragma unroll
        for (int q = 0; q < C::AB_ROUNDS; ++q) nAB[q] = DPILQR_REC_LD(reinterpret_cast<const v2d*>(rec + ab_src[q]));
        }
    };
    auto prefetch_lxu = [&](int t) {   // only the lanes of the p column need it
        const double* rec = base + (int64_t)t * L.stride + (PAD ? 0 : gLxu);
#pragma unroll
        for (int it = 0; it < T_NM; ++it) {
#pragma unroll
            for (int v = 0; v < 4; ++v) nLxu[it][v] = 0.0;
            for_rows(16 * it, 0, NM, g, colP[N / 16], [&](int v, int r) {
                if constexpr (PAD) {   // entry i' = g + r of [l_x ; l_u] of the padded problem
                    const int ip = g + r;
                    nLxu[it][v] = rec_or_pad(rec, ip < N ? (ip < n_rec ? L.oLx + ip : -1) : (ip - N < m_rec ? L.oLu + ip - N : -1));
                } else {
                nLxu[it][v] = rec[r];
                }
            });
        }
    };
    auto prefetch_l = [&](int t) {
        const double* rec = base + (int64_t)t * L.stride;
#pragma unroll
        for (int it = 0; it < T_NM; ++it)
#pragma unroll
            for (int jt = 0; jt < T_NM; ++jt) {
#pragma unroll
                for (int v = 0; v < 4; ++v) nL[it][jt][v] = 0.0;
                if constexpr (PAD) {
                    const int j = 16 * jt + c16;
                    for_rows(16 * it, 0, N, g, colN[jt], [&](int v, int r) {       // L_xx[i][j], i = g + r
                        const int i = g + r;
                        nL[it][jt][v] = rec_or_pad(rec, (i < n_rec && j < n_rec) ? L.oLxx + i * n_rec + j : -1);
                    });
                    for_rows(16 * it, N, NM, g, colNM[jt], [&](int v, int r) {     // row a = g + r of [L_ux | L_uu] (global columns)
                        const int a = g + r, cu = j - N;
                        const int off = (j < N) ? ((a < m_rec && j < n_rec) ? L.oLux + a * L.ldUG + j : -1)
                                                : ((a < m_rec && cu < m_rec) ? L.oLuu + a * L.ldUG + cu : ((a == cu && a >= m_rec) ? -2 : -1));
                        nL[it][jt][v] = rec_or_pad(rec, off);
                    });
                } else {
                for_rows(16 * it, 0, N, g, colN[jt], [&](int v, int r) { nL[it][jt][v] = rec[gLxx + 16 * jt + r * N]; });
                for_rows(16 * it, N, NM, g, colNM[jt], [&](int v, int r) { nL[it][jt][v] = rec[gUG + colG[jt] + r * L.ldUG]; });
                }
            }
    };

    // ---- fused variant (FUSED): the step's plugin data live behind [Q_xx | Q_x] in R1 (MfmaCfg::oF*)
    constexpr int FKA = C::F_KA, FNP = C::F_NP;
    // (HELP: the step-dependent arrays exist twice, C::FB apart; step t_cur's are in copy t_cur & 1)
    const int fb = HELP ? (t_cur & 1) * C::FB : 0;
    double* sFG = lds + C::oQ + C::oFG + fb;      // pair gradients  [FNP][2]
    double* sFH = lds + C::oQ + C::oFH + fb;      // pair Hessians   [FNP][4]  (xx, xy, yx, yy)
    double* sFD = lds + C::oQ + C::oFD + fb;      // their sums over the pairs containing agent a [FKA][4]
    double* sFQQ = lds + C::oQ + C::oFQQ;    // Q + Q^T  [4][4]
    double* sFRR = lds + C::oQ + C::oFRR;    // R + R^T  [2][2]
    double* sFXf = lds + C::oQ + C::oFXf;    // x_f      [N]
    double* sFL = lds + C::oQ + C::oFL + fb;      // the step's [l_x | l_u]  [N + M]
    double* sFA = lds + C::oQ + C::oFA + fb;      // FUSED == 2: the step's entries (0,2), (1,2), (0,3), (1,3) of every agent's A block [FKA][4]
    double* sFflag = lds + C::oQ + C::oFflag + fb;   // HELP: "some pair of the step is within the radius" (the helper's f_prox)
    (void)sFflag;
    const double* Xfb = FUSED ? F.X + (int64_t)b * (T + 1) * N : nullptr;
    const double* Ufb = FUSED ? F.U + (int64_t)b * T * M : nullptr;
    // lane roles: lanes 0 .. FNP-1 evaluate one pair (i, j) each (itertools.combinations order); lane 32 + j forms entry j
    // of [l_x | l_u].  Each lane requests, a step ahead, the two 16-byte pieces of (X[t], U[t]) it needs.
    static_assert(!FUSED || (C::F_NP <= 32 && NM <= 32), "lane roles of the fused variant");
    int f_pi = 0, f_pj = 0;
    {
        int rem = min(lane, FNP > 0 ? FNP - 1 : 0);
        while (FKA > 1 && rem >= FKA - 1 - f_pi) { rem -= FKA - 1 - f_pi; ++f_pi; }
        f_pj = f_pi + 1 + rem;
    }
    const bool f_pair = FUSED && lane < FNP;
    const int f_j = min(max(lane - 32, 0), NM - 1);               // entry of [l_x | l_u] this lane forms (lanes >= 32)
    const bool f_lx = FUSED && lane >= 32 && lane - 32 < N, f_lu = FUSED && lane - 32 >= N && lane - 32 < NM;
    const int f_a = f_lx ? (f_j >> 2) : (f_lu ? ((f_j - N) >> 1) : 0);   // its agent (lanes without a role read agent 0's piece)
    // FUSED == 2: this lane's agent's model, DoubleInt4D or Unicycle4D (the host checked the descriptor's hints); read once: the
    // general form runs at one or two wavefronts per SIMD, where these terms are hoisted out of the horizon loop
    const int f_model = FUSED == 2 ? F.D.model[(int64_t)b * F.D.model_bstride + f_a] : 0;
    const int f_o0 = f_pair ? 4 * f_pi : (f_lu ? 2 * f_a : 4 * f_a);
    const int f_o1 = f_pair ? 4 * min(f_pj, FKA - 1) : (f_lu ? 2 * f_a : 4 * f_a + 2);
    auto fused_prefetch = [&](int t) {
        const double* row = (f_lu ? Ufb + (int64_t)min(t, T - 1) * M : Xfb + (int64_t)t * N);
        pf[0] = *reinterpret_cast<const v2d*>(row + f_o0);
        pf[1] = *reinterpret_cast<const v2d*>(row + f_o1);
    };
    // The plugin data of the step whose pieces are in pf.  Pair derivatives: quadraticize_distance (cost.py:269-315, planar),
    // skipped altogether when every pair is safely beyond the radius (then they are exact zeros and f_prox tells the
    // consumers not to look: adding w_prox * 0 changes nothing); per-agent sums of the Hessians and [l_x | l_u] in the
    // tile producer's expressions and orders (tiles_wave.hpp phases A3, B2).  QQt: Q_f for the terminal record.
    auto fused_step_data = [&](int t, const double* Qterm) {
        if (FNP > 0) {
            const double ddx = pf[0].x - pf[1].x, ddy = pf[0].y - pf[1].y;
            const double s2 = ddx * ddx + ddy * ddy;
            const bool near = f_pair && !(s2 > f_radius * f_radius * (1.0 + 1e-12));
            f_prox = __builtin_amdgcn_ballot_w64(near) != 0ull;
            if (f_prox) {
                if (f_pair) {
                    const double pa[2] = {pf[0].x, pf[0].y}, pb[2] = {pf[1].x, pf[1].y};
                    double gg[3], HH[9];
                    pair_quadraticize(pa, pb, 2, f_radius, gg, HH);
                    sFG[2 * lane] = gg[0]; sFG[2 * lane + 1] = gg[1];
                    sFH[4 * lane] = HH[0]; sFH[4 * lane + 1] = HH[1]; sFH[4 * lane + 2] = HH[3]; sFH[4 * lane + 3] = HH[4];
                }
                DPILQR_LDS_FENCE();
                if (lane < 4 * FKA) {
                    const int a = lane >> 2, c = lane & 3;
                    // (all loads first -- the own index reads pair 0 and is not added: a load behind `o != a` is a branch
                    // and an LDS round trip per term)
                    double hv[FKA > 0 ? FKA : 1];
#pragma unroll
                    for (int o = 0; o < FKA; ++o)
                        hv[o] = sFH[(o == a ? 0 : ((o < a) ? pair_index(o, a, FKA) : pair_index(a, o, FKA))) * 4 + c];
                    double acc = 0.0;
#pragma unroll
                    for (int o = 0; o < FKA; ++o) {
                        const double nx = acc + hv[o];
                        acc = (o == a) ? acc : nx;
                    }
                    sFD[lane] = acc;
                }
            }
        }
        if (f_lx) {
            const int lj = f_j & 3;
            const double e0 = pf[0].x - sFXf[4 * f_a], e1 = pf[0].y - sFXf[4 * f_a + 1];
            const double e2 = pf[1].x - sFXf[4 * f_a + 2], e3 = pf[1].y - sFXf[4 * f_a + 3];
            double v = 0.0;
            if (Qterm) {
                const double* Qt = Qterm + (FUSED == 2 ? 16 * f_a : 0);
                v += e0 * (Qt[0 * 4 + lj] + Qt[lj * 4 + 0]); v += e1 * (Qt[1 * 4 + lj] + Qt[lj * 4 + 1]);
                v += e2 * (Qt[2 * 4 + lj] + Qt[lj * 4 + 2]); v += e3 * (Qt[3 * 4 + lj] + Qt[lj * 4 + 3]);
            } else {
                const double* qq = sFQQ + (FUSED == 2 ? 16 * f_a : 0);
                v += e0 * qq[0 * 4 + lj]; v += e1 * qq[1 * 4 + lj]; v += e2 * qq[2 * 4 + lj]; v += e3 * qq[3 * 4 + lj];
            }
            v = F.D.w_ref * v;
            if (FKA > 1 && lj < 2 && f_prox) {
                double gv[FKA > 0 ? FKA : 1];
#pragma unroll
                for (int o = 0; o < FKA; ++o)
                    gv[o] = sFG[(o == f_a ? 0 : ((o < f_a) ? pair_index(o, f_a, FKA) : pair_index(f_a, o, FKA))) * 2 + lj];
                double acc = 0.0;
#pragma unroll
                for (int o = 0; o < FKA; ++o) {
                    const double nx = acc + ((o < f_a) ? -gv[o] : gv[o]);
                    acc = (o == f_a) ? acc : nx;
                }
                v += F.D.w_prox * acc;
            }
            sFL[f_j] = v;
            if constexpr (FUSED == 2) {
                // this step's A block of the agent, by its first l_x lane (it holds the agent's whole state): the model's Jacobian
                // entries as MultiDynamicalModel.linearize forms them (models.hpp: jac, then I + dt A_c -- 0 + dt a is dt a)
                if (lj == 0 && t < T) {
                    const double fdt_ = F.D.dt;
                    double a02 = fdt_ * 1.0, a12 = fdt_ * 0.0, a03 = fdt_ * 0.0, a13 = fdt_ * 1.0;   // DoubleIntDynamics4D
                    if (f_model == kUnicycle4D) {
                        double sn, cs;
                        sincos(pf[1].y, &sn, &cs);            // (one argument reduction; the same values as sin(), cos())
                        const double vv = pf[1].x;            // x = [px, py, v, theta]
                        a02 = fdt_ * cs; a03 = fdt_ * (-vv * sn);
                        a12 = fdt_ * sn; a13 = fdt_ * (vv * cs);
                    }
                    *reinterpret_cast<v2d*>(sFA + 4 * f_a) = v2d{a02, a12};
                    *reinterpret_cast<v2d*>(sFA + 4 * f_a + 2) = v2d{a03, a13};
                }
            }
        }
        if (f_lu && t < T) {
            const int lj = (f_j - N) & 1;
            const double* rr = sFRR + (FUSED == 2 ? 4 * f_a : 0);
            double v = 0.0;
            v += pf[0].x * rr[0 * 2 + lj]; v += pf[0].y * rr[1 * 2 + lj];
            sFL[f_j] = F.D.w_ref * v;
        }
        DPILQR_LDS_FENCE();
    };
