// In-sweep production (riccati_mfma.hpp, PNS > 0): the producer half.  NOT a stand-alone header: included once in the body of
// riccati_mfma_sweep, before the prologue.  For PNS == 0 everything here folds away.
//
// What the reference computes per step inside ilqrSolver._backward_pass (control.py:125-133) -- MultiDynamicalModel.linearize
// (dynamics.py:173-186 -> bbdynamics.cpp linearize_*), GameCost.quadraticize (cost.py:208-239, :85-101, :135-171, :269-315) -- in
// the expressions and summation orders of the sparse tile producer (tiles.hpp, SPARSE), entry for entry, so that what the S1 / S2
// epilogues add is what the record-fed padded sweep reads from its records:
//   lanes a < k         their agent's (x, u): x, x - x_f, u -> LDS; [A_a | B_a] = I + dt A_c, dt B_c into the zeroed [A|B] operand
//   lanes p < pairs     quadraticize_distance of pair p (itertools.combinations order)
//   lanes j < n         l_x[j];   lanes 32 + j, j < m: l_u[j]
//   all lanes           the position entries of the agents' diagonal blocks of L_xx and the coupling blocks (the rest of a
//                       diagonal block is w_ref (Q + Q^T): written once)
// The agent lanes hold their agent's (x[t], u[t]) in registers, requested a step ahead.
    constexpr int PNS1 = PNS > 0 ? PNS : 1, PNC = IC::PNC, PD = PNS1 < 3 ? PNS1 : 3;
    double* sLxx = lds + C::total + IC::oLxx;
    double* sLuu = lds + C::total + IC::oLuu;
    double* sLxu = lds + C::total + IC::oLxu;
    double* sIX = lds + C::total + IC::oX;
    double* sIE = lds + C::total + IC::oE;
    double* sIU = lds + C::total + IC::oU;
    double* sIXf = lds + C::total + IC::oXf;
    double* sIG = lds + C::total + IC::oGp;
    double* sIH = lds + C::total + IC::oHp;
    double* sIQQ = lds + C::total + IC::oQQ;
    double* sIRR = lds + C::total + IC::oRR;
    int* sIPair = reinterpret_cast<int*>(lds + C::total + IC::oPair);   // pair p = (i, j), i < j, itertools.combinations order: i | j << 8
    (void)sIPair;
    (void)sLxx; (void)sLuu; (void)sLxu; (void)sIX; (void)sIE; (void)sIU; (void)sIXf; (void)sIG; (void)sIH; (void)sIQQ; (void)sIRR;
    const int inp_k = INP ? n_rec / PNS1 : 0;                      // agents of the cluster
    const int inp_np = inp_k * (inp_k - 1) / 2;
    double inp_x[PNS1], inp_u[PNC];                                // the agent lanes' share of (X[t], U[t]), one step ahead
    bool inp_prev_near = true;     // L_xx's position / coupling entries and the pair arrays do not hold a far step's values
    int inp_model = 0, inp_nd = 2;
    double inp_radius = 0.0;
    if constexpr (INP) {
        const ItemParams IP = item_params(F.D, b);
        inp_model = IP.model[min(lane0, inp_k - 1)];
        inp_radius = IP.radius;
        // the pair lanes' n_dims (cost.py:145)
        int pi = 0, rem = min(lane0, max(inp_np - 1, 0));
        while (inp_k > 1 && rem >= inp_k - 1 - pi) { rem -= inp_k - 1 - pi; ++pi; }
        const int pj = min(pi + 1 + rem, inp_k - 1);
        inp_nd = min(IP.n_dims[pi], IP.n_dims[pj]);
    }
    auto inp_prefetch = [&](int t) {
        if constexpr (INP) {
            const int a = min(lane0, inp_k - 1);
            const double* xr = F.X + ((int64_t)b * (T + 1) + t) * n_rec + a * PNS1;
            const double* ur = F.U + ((int64_t)b * T + min(t, T - 1)) * m_rec + a * PNC;
#pragma unroll
            for (int i = 0; i < PNS1; ++i) inp_x[i] = xr[i];
#pragma unroll
            for (int i = 0; i < PNC; ++i) inp_u[i] = ur[i];
        }
    };
    // once per item: Q + Q^T, R + R^T, x_f; L_uu = w_ref blockdiag(R + R^T) with 1 on the diagonal of padded controls; the
    // whole LDS has just been zeroed
    auto inp_constants = [&]() {
        if constexpr (INP) {
            const ItemParams IP = item_params(F.D, b);
            const double wr = F.D.w_ref;
            for (int e = lane0; e < inp_k * PNS1 * PNS1; e += 64) {
                const int a = e / (PNS1 * PNS1), r = e - a * PNS1 * PNS1, li = r / PNS1, lj = r - li * PNS1;
                sIQQ[e] = IP.Q[a * PNS1 * PNS1 + li * PNS1 + lj] + IP.Q[a * PNS1 * PNS1 + lj * PNS1 + li];
            }
            for (int e = lane0; e < inp_k * PNC * PNC; e += 64) {
                const int a = e / (PNC * PNC), r = e - a * PNC * PNC, li = r / PNC, lj = r - li * PNC;
                const double rr = IP.R[a * PNC * PNC + li * PNC + lj] + IP.R[a * PNC * PNC + lj * PNC + li];
                sIRR[e] = rr;
                sLuu[(a * PNC + li) * M + a * PNC + lj] = wr * rr;
            }
            for (int e = lane0; e < n_rec; e += 64) sIXf[e] = IP.xf[e];
            if (lane0 < inp_np) {
                int i = 0, rem = lane0;
                while (rem >= inp_k - 1 - i) { rem -= inp_k - 1 - i; ++i; }
                sIPair[lane0] = i | ((i + 1 + rem) << 8);
            }
            if (lane0 >= m_rec && lane0 < M) sLuu[lane0 * M + lane0] = 1.0;
            DPILQR_LDS_FENCE();
        }
    };
    // the agents' diagonal blocks of L_xx (whole: every entry; else the position entries only) and, unless blocks_only, the coupling
    // blocks: L_xx = w_ref blockdiag(Q + Q^T) + w_prox sum_pairs(+-H) (cost.py:228-237, 160-169)
    // (every divisor a compile-time constant: WHOLE selects the walk over whole blocks or over their position entries)
    auto inp_lxx_diag = [&](auto whole_tag, bool terminal, bool with_pairs) {
        if constexpr (INP) {
            constexpr bool WHOLE = decltype(whole_tag)::value;
            constexpr int per = WHOLE ? PNS1 * PNS1 : PD * PD, edge = WHOLE ? PNS1 : PD;
            int ln = lane0;
            asm volatile("" : "+v"(ln));
            const double wr = F.D.w_ref, wp = F.D.w_prox;
            const double* Qf_all = item_params(F.D, b).Qf;
            for (int e = ln; e < inp_k * per; e += 64) {
                const int a = e / per, r = e - a * per, li = r / edge, lj = r - li * edge;
                double v;
                if (terminal) {
                    const double* Mf = Qf_all + a * PNS1 * PNS1;
                    v = wr * (Mf[li * PNS1 + lj] + Mf[lj * PNS1 + li]);
                } else {
                    v = wr * sIQQ[a * PNS1 * PNS1 + li * PNS1 + lj];
                }
                if (inp_k > 1 && li < 3 && lj < 3) {   // (without the pairs: + w_prox 0, what the sum of exact zeros adds)
                    double acc = 0.0;
                    if (with_pairs) {
                        for (int o = 0; o < inp_k; ++o) {
                            if (o == a) continue;
                            const int p = (o < a) ? pair_index(o, a, inp_k) : pair_index(a, o, inp_k);
                            acc += sIH[p * 9 + li * 3 + lj];
                        }
                    }
                    v += wp * acc;
                }
                sLxx[(a * PNS1 + li) * N + a * PNS1 + lj] = v;
            }
        }
    };
    auto inp_lxx_blocks = [&](bool terminal, bool blocks_only) {
        if constexpr (INP) {
            if (terminal || blocks_only) inp_lxx_diag(std::true_type{}, terminal, !blocks_only);
            else inp_lxx_diag(std::false_type{}, false, true);
            if (!blocks_only) {
                int ln = lane0;
                asm volatile("" : "+v"(ln));
                const double wp = F.D.w_prox;
                for (int e = ln; e < inp_np * 2 * PD * PD; e += 64) {
                    const int p = e / (2 * PD * PD), r = e - p * 2 * PD * PD, mirror = r / (PD * PD), q = r - mirror * PD * PD;
                    const int li = q / PD, lj = q - li * PD;
                    const int ij = sIPair[p], i = ij & 255, j = ij >> 8;
                    const int ai = mirror ? j : i, aj = mirror ? i : j;
                    double acc = 0.0;
                    acc += -sIH[p * 9 + li * 3 + lj];
                    sLxx[(ai * PNS1 + li) * N + aj * PNS1 + lj] = 0.0 + wp * acc;
                }
            }
        }
    };
    auto inp_produce = [&](int t, bool terminal) {
        if constexpr (INP) {
            int ln = lane0;
            asm volatile("" : "+v"(ln));     // the lane terms below are recomputed per call, not kept across the step's phases
            const double wr = F.D.w_ref, wp = F.D.w_prox;
            if (!terminal) {
                // the [A|B] operand: zeros (the region held [Q_xx | Q_x] of the previous step), then the agents' blocks
                for (int e = ln; e < N * LAB / 2; e += 64) *reinterpret_cast<v2d*>(sAB + 2 * e) = v2d{0.0, 0.0};
                DPILQR_LDS_FENCE();
            }
            if (ln < inp_k) {
                const int a = ln;
                double u[PNC];
#pragma unroll
                for (int i = 0; i < PNC; ++i) u[i] = terminal ? 0.0 : inp_u[i];
#pragma unroll
                for (int i = 0; i < PNS1; ++i) {
                    sIX[a * PNS1 + i] = inp_x[i];
                    sIE[a * PNS1 + i] = inp_x[i] - sIXf[a * PNS1 + i];
                }
#pragma unroll
                for (int i = 0; i < PNC; ++i) sIU[a * PNC + i] = u[i];
                if (!terminal) {
                    // the agent's [A_a | B_a], stored INSIDE its model's case: merged behind the switch the blocks of all the
                    // family's models would meet in PNS (PNS + PNC) registers; inside, a model's constant entries are immediates
                    double* row = sAB + (a * PNS1) * LAB;
                    auto lin_store = [&](auto model_tag) {
                        constexpr int MDL = decltype(model_tag)::value;
                        if constexpr (ModelDef<MDL>::NS == PNS1) {
                            double A[PNS1 * PNS1], Bm[PNS1 * PNC];
                            linearize<MDL>(inp_x, u, F.D.dt, A, Bm);
#pragma unroll
                            for (int li = 0; li < PNS1; ++li) {
#pragma unroll
                                for (int lj = 0; lj < PNS1; ++lj) row[li * LAB + a * PNS1 + lj] = A[li * PNS1 + lj];
#pragma unroll
                                for (int lj = 0; lj < PNC; ++lj) row[li * LAB + N + a * PNC + lj] = Bm[li * PNC + lj];
                            }
                        }
                    };
#define DPILQR_INP_CASE(MDL) case MDL: lin_store(std::integral_constant<int, MDL>{}); break;
                    switch (inp_model) {
                        DPILQR_INP_CASE(kDoubleInt4D) DPILQR_INP_CASE(kDoubleInt6D) DPILQR_INP_CASE(kCar3D) DPILQR_INP_CASE(kUnicycle4D)
                        DPILQR_INP_CASE(kQuadcopter6D) DPILQR_INP_CASE(kHuman6D) DPILQR_INP_CASE(kHumanLin6D)
                        DPILQR_INP_CASE(kQuadcopter12D) DPILQR_INP_CASE(kHumanPad12D) DPILQR_INP_CASE(kBike5D)
                        default: break;
                    }
#undef DPILQR_INP_CASE
                }
            }
            if (!terminal && ln >= n_rec && ln < N) sAB[ln * LAB + ln] = 1.0;   // padded states: A = 1 on the diagonal, B = 0
            DPILQR_LDS_FENCE();
            // The pair derivatives -- skipped when every pair is safely beyond the radius: they are exact zeros then
            // (quadraticize_distance returns zeros for distance > radius; the margin covers the rounding of r r and of the square
            // root), and so is everything they are summed into.  The first far step after a near one writes the zeros once.
            bool near_any = false;
            if (inp_k > 1) {
                bool near = false;
                const int ij = sIPair[min(ln, inp_np - 1)], pi_ = ij & 255, pj_ = ij >> 8;
                if (ln < inp_np) {
                    double s2 = 0.0;
#pragma unroll
                    for (int c = 0; c < PD; ++c) {
                        const double df = sIX[pi_ * PNS1 + c] - sIX[pj_ * PNS1 + c];
                        s2 += (c < inp_nd) ? df * df : 0.0;
                    }
                    near = !(s2 > inp_radius * inp_radius * (1.0 + 1e-12));
                }
                near_any = __builtin_amdgcn_ballot_w64(near) != 0ull;
                if (near_any) {
                    if (ln < inp_np) {
                        double gg[3], HH[9];
                        pair_quadraticize(sIX + pi_ * PNS1, sIX + pj_ * PNS1, inp_nd, inp_radius, gg, HH);
#pragma unroll
                        for (int c = 0; c < 3; ++c) sIG[ln * 3 + c] = gg[c];
#pragma unroll
                        for (int c = 0; c < 9; ++c) sIH[ln * 9 + c] = HH[c];
                    }
                    DPILQR_LDS_FENCE();
                } else if (inp_prev_near) {
                    if (ln < inp_np) {
#pragma unroll
                        for (int c = 0; c < 3; ++c) sIG[ln * 3 + c] = 0.0;
#pragma unroll
                        for (int c = 0; c < 9; ++c) sIH[ln * 9 + c] = 0.0;
                    }
                    DPILQR_LDS_FENCE();
                }
            }
            // L_x = w_ref e^T (Q + Q^T) + w_prox sum_pairs(+-g) ; L_u = w_ref u^T (R + R^T)
            if (ln < n_rec) {
                const int j = ln, a = j / PNS1, lj = j - a * PNS1;
                double v = 0.0;
                if (terminal) {
                    const double* Mf = item_params(F.D, b).Qf + a * PNS1 * PNS1;
#pragma unroll
                    for (int i = 0; i < PNS1; ++i) v += sIE[a * PNS1 + i] * (Mf[i * PNS1 + lj] + Mf[lj * PNS1 + i]);
                } else {
#pragma unroll
                    for (int i = 0; i < PNS1; ++i) v += sIE[a * PNS1 + i] * sIQQ[a * PNS1 * PNS1 + i * PNS1 + lj];
                }
                v = wr * v;
                if (inp_k > 1 && lj < 3) {
                    double acc = 0.0;
                    if (near_any) {
                        for (int o = 0; o < inp_k; ++o) {
                            if (o == a) continue;
                            if (o < a) acc += -sIG[pair_index(o, a, inp_k) * 3 + lj];
                            else       acc += sIG[pair_index(a, o, inp_k) * 3 + lj];
                        }
                    }
                    v += wp * acc;
                }
                sLxu[j] = v;
            }
            if (!terminal && ln >= 32 && ln - 32 < m_rec) {
                const int j = ln - 32, a = j / PNC, lj = j - a * PNC;
                double v = 0.0;
#pragma unroll
                for (int i = 0; i < PNC; ++i) v += sIU[a * PNC + i] * sIRR[a * PNC * PNC + i * PNC + lj];
                sLxu[N + j] = wr * v;
            }
            // L_xx: the terminal record whole; else the position and coupling entries, unless they hold a far step's values already
            if (terminal || near_any || inp_prev_near) inp_lxx_blocks(terminal, false);
            inp_prev_near = near_any || terminal;
            DPILQR_LDS_FENCE();
        }
    };
