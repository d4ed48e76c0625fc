// lec_level_row.inc -- the contributions of ONE latitude row to the 33 per-level sums of stage 2, included textually by the two
// level kernels of lec_level_core.h, whichever record source they are instantiated on, and (LEC_ROW_COMMON + LEC_ROW_PART_A) by
// lec_section_rows_kernel (identical source, identical arithmetic).  Expects in scope:
//   r[LEC_NSTAT]               the row's record;  rjm[], rjp[]: the records of the rows j-1 / j+1 (only [T] [u] [v] are read)
//   km2, kp2                   {[T], [u]} of the same row one level up / down
//   cw wphi c tn gra grb grc   the row's latitude coefficients, cm / cp: cos(phi) of the rows j-1 / j+1
//   aT aW aP aQ aTm aTp        area means (own level; T one level up / down),  pa pb pc: d/dp coefficients,  ps: phi_scale
//   jb, nyb, acc[V_COUNT]      and LEC_BAZ3_REPAIR(jb): BAz's bottom-top term of this row repaired along p
// Sections (define before including; the general kernel takes all three at once, the small-box kernel reduces part A's sums before
// it forms part B's, to hold fewer of them in registers):  LEC_ROW_COMMON  the row's means, deviations and covariances;
// LEC_ROW_PART_A  energy, conversion and generation sums (V_AZ .. V_GE);  LEC_ROW_PART_B  boundary sums (V_B1 .. V_B3 + 5).
#ifdef LEC_ROW_COMMON
        const double mT = r[LEC_S_MT], mU = r[LEC_S_MU], mV = r[LEC_S_MV], mW = r[LEC_S_MW];
        const double mP = r[LEC_S_MP] * ps, mQ = r[LEC_S_MQ];
        const double Ts = mT - aT, Ws = mW - aW, Ps = mP - aP, Qs = mQ - aQ;      // X* = [X] - {[X]}
        const double sTT = r[LEC_S_TT], sUU = r[LEC_S_UU], sVV = r[LEC_S_VV], sVT = r[LEC_S_VT], sWT = r[LEC_S_WT];
        const double sUV = r[LEC_S_UV], sWU = r[LEC_S_WU], sWV = r[LEC_S_WV], sWP = r[LEC_S_WP] * ps, sQT = r[LEC_S_QT];
#endif
#ifdef LEC_ROW_PART_A
        const double dphiTc = gra * (rjm[LEC_S_MT] - aT) * cm + grb * Ts * c + grc * (rjp[LEC_S_MT] - aT) * cp;
        const double dphiUc = gra * (rjm[LEC_S_MU] / cm) + grb * (mU / c) + grc * (rjp[LEC_S_MU] / cp);
        const double dphiV = gra * rjm[LEC_S_MV] + grb * mV + grc * rjp[LEC_S_MV];
        const double dpT = pa * (km2.x - aTm) + pb * Ts + pc * (kp2.x - aTp);
        const double dpU = pa * km2.y + pb * mU + pc * kp2.y;

        acc[V_AZ] += cw * (Ts * Ts);
        acc[V_AE] += cw * sTT;
        acc[V_KZ] += cw * (mU * mU + mV * mV);
        acc[V_KE] += cw * (sUU + sVV);
        acc[V_CZ2] += cw * (Ws * Ts);
        acc[V_CE2] += cw * sWT;
        acc[V_CA1] += cw * (sVT * dphiTc);
        acc[V_CA2] += cw * (sWT * dpT);
        acc[V_CK1] += cw * (c * sUV / kRe * dphiUc);
        acc[V_CK2] += cw * (sVV / kRe * dphiV);
        acc[V_CK3] += cw * (tn * sUU * mV / kRe);
        acc[V_CK4] += cw * (sWU * dpU);
        acc[V_CK5] += cw * (sWV * dpU);   // sic: d[u]/dp, conversion_terms.py:225-229
        acc[V_GZ] += cw * (Qs * Ts);
        acc[V_GE] += cw * sQT;
#endif
#ifdef LEC_ROW_PART_B
        // east-west pieces, plain trapezoid over phi (boundary_terms.py:135-147,188-197,237-246,287-296,337-344,377-388)
        const double TW = r[LEC_S_TW], TE = r[LEC_S_TE], uW = r[LEC_S_UW], uE = r[LEC_S_UE], vW = r[LEC_S_VW], vE = r[LEC_S_VE];
        const double TpW = TW - mT, TpE = TE - mT;
        const double upW = uW - mU, upE = uE - mU, vpW = vW - mV, vpE = vE - mV;
        const double EW_ = upW * upW + vpW * vpW, EE_ = upE * upE + vpE * vpE;
        const double KW_ = uW * uW + vW * vW - EW_, KE_ = uE * uE + vE * vE - EE_;
        acc[V_B1 + 0] += wphi * (((2 * Ts * TpE * uE) + (Ts * Ts * uE)) - ((2 * Ts * TpW * uW) + (Ts * Ts * uW)));
        acc[V_B1 + 1] += wphi * (uE * (TpE * TpE) - uW * (TpW * TpW));
        acc[V_B1 + 2] += wphi * (uE * KE_ - uW * KW_);
        acc[V_B1 + 3] += wphi * (uE * EE_ - uW * EW_);
        acc[V_B1 + 4] += wphi * (mV * Ps);
        acc[V_B1 + 5] += wphi * (vpE * Ps - vpW * Ps);

        // north-south pieces (boundary_terms.py:150-163,200-212,249-262,299-310,347-356,390-399)
        const double sgn = (jb == nyb - 1 ? 1.0 : 0.0) - (jb == 0 ? 1.0 : 0.0);
        if (sgn != 0.0) {
            acc[V_B2 + 0] += sgn * (((sVT * 2 * Ts) + (Ts * Ts * mV)) * c);
            acc[V_B2 + 1] += sgn * (r[LEC_S_VTT] * c);
            acc[V_B2 + 2] += sgn * (r[LEC_S_KV] * c);
            acc[V_B2 + 3] += sgn * (r[LEC_S_EV] * c);
            acc[V_B2 + 4] += sgn * (mV * Ps * c);
            acc[V_B2 + 5] += sgn * (mV * Ps * c);   // BPhiE term 2 uses zonal means, boundary_terms.py:390
        }

        // bottom-top pieces, area means (boundary_terms.py:165-176,214-221,264-271,312-318,358-363,401-413)
        double x3 = (2 * sWT) * Ts + mW * (Ts * Ts);
        if (isnan(x3)) x3 = LEC_BAZ3_REPAIR(jb);        // per latitude, before the area mean (the reference's order)
        acc[V_B3 + 0] += cw * x3;
        acc[V_B3 + 1] += cw * r[LEC_S_WTT];
        acc[V_B3 + 2] += cw * r[LEC_S_KW];
        acc[V_B3 + 3] += cw * r[LEC_S_EW];
        acc[V_B3 + 4] += cw * (Ws * Ps);
        acc[V_B3 + 5] += cw * sWP;
#endif
