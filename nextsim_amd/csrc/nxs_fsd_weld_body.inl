// nxs_fsd_weld_body.inl -- weldingRoach (FE.cpp:4737-4870) on one element's bins in registers, as STATEMENTS: included inside `if (c->welding_type ==
// NXS_WELDING_ROACH) { ... }` by k_fsd_weld (nxs_fsd_kernels.inl) and by k_coupled_bins (nxs_slab_fsd_kernels.inl: the in-loop call of thermo(), FE.cpp:5790), so
// that the welding has one source and k_fsd_weld compiles to the code it always was (as a device function the same lines cost it registers).  The includer has in
// scope: tmp[NB] (M_conc_fsd[..][cpt], then tmp_conc_fsd, then M_conc_fsd again), c (const FsdDev *), n, ddt, crash (bool), a (FsdArrays), e, and defines
// FSD_WELD_MERGED(), a statement run once where floes are merged.
            double c_fsd_broken = tmp[0];
            double old_conc_tot = 0.;   // std::accumulate(old_conc_fsd.begin(), old_conc_fsd.end(), 0.)
#pragma unroll
            for (int k = 0; k < NB; ++k) if (k < n) old_conc_tot = old_conc_tot + tmp[k];
#pragma unroll
            for (int j = 1; j < NB; ++j) if (j < n - 1) c_fsd_broken += tmp[j];
            if ((c_fsd_broken > 0.01) && (old_conc_tot > 0.1)) {
                FSD_WELD_MERGED();
                double unbroken_area_loss = 0.;
                double asu_top = c->asu[0];
#pragma unroll
                for (int k = 1; k < NB; ++k) if (k == n - 1) asu_top = c->asu[k];
                const double stability = ddt * c->kappa * old_conc_tot * asu_top;
                const int ndt_mrg = (int)round(stability + 0.5);
                const double subdt = ddt / ((float)ndt_mrg);
                double coag_pos[NB];
                for (int t = 0; t < ndt_mrg; t++) {
#pragma unroll
                    for (int kx = 0; kx < NB; ++kx) {
                        coag_pos[kx] = 0.;
                        if (kx >= n) continue;
#pragma unroll
                        for (int ky = 0; ky <= kx; ++ky) {
                            const int al = c->alpha[kx][ky];   // the same for every lane: a scalar load
                            double sum_mergers = 0.;
                            double t_a = tmp[0];               // tmp_conc_fsd[a - 1]: a chain of selects, no dynamic register index
#pragma unroll
                            for (int p = 0; p < NB; ++p) {
                                if (p >= al && p < n) sum_mergers += tmp[p];
                                if (p == al - 1) t_a = tmp[p];
                            }
                            coag_pos[kx] = coag_pos[kx] + c->asc[ky] * tmp[ky] * old_conc_tot *
                                                              (sum_mergers + (t_a / c->asb[al - 1]) * (c->asu[al - 1] - c->asu[kx] + c->asc[ky]));
                        }
                    }
                    const double sk = subdt * c->kappa;
                    // coag_neg[0] = 0., coag_neg[m] = coag_pos[m - 1]
                    tmp[0] = tmp[0] - sk * (coag_pos[0] - 0.);
                    double top = coag_pos[0];
#pragma unroll
                    for (int m = 1; m < NB; ++m)
                        if (m < n) { tmp[m] = tmp[m] - sk * (coag_pos[m] - coag_pos[m - 1]); top = coag_pos[m]; }
                    unbroken_area_loss = unbroken_area_loss + sk * top;
                    if (c->debug) {
#pragma unroll
                        for (int m = 0; m < NB; ++m)
                            if (m < n && ((tmp[m] < -1e-11) || (tmp[m] > 1.) || (sk * coag_pos[m] < -1e-11))) crash = true;
                    }
                }
#pragma unroll
                for (int m = 0; m < NB; ++m) if (m == n - 1) tmp[m] = tmp[m] + unbroken_area_loss;
                double sum_new = 0.;
#pragma unroll
                for (int k = 0; k < NB; ++k) if (k < n) sum_new = sum_new + tmp[k];
                const double conc_loss = sum_new - old_conc_tot;
                if (fabs(conc_loss) > 1.e-6) crash = true;
#pragma unroll
                for (int m = 0; m < NB; ++m)
                    if (m < n) {
                        tmp[m] = tmp[m] * old_conc_tot / sum_new;
                        if (tmp[m] < 0.) {
                            if (tmp[m] < -1e-12) crash = true;
                            else tmp[m] = 0.;
                        }
                        a.fsd[(size_t)m * a.Ne + e] = tmp[m];
                    }
            }
