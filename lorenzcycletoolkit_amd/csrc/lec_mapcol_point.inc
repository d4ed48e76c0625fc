// lec_mapcol_point.inc -- Q and the six eddy integrands at ONE point (t, k, j, i), included textually inside the march of
// lec_mapcol_col_kernel (lec_mapcol.h: down the levels of a row) and of lec_lonsec_kernel (lec_lonsections.hip: up the rows of a level).
// Text, not a function: the compiler sees the tokens each kernel held before (DESIGN.md section 4.2h).  Expects in scope:
//   RING DMODE kCp first last  the kernel's template parameters, cp, and "the box's first / last column"
//   Tc Tl Tr Tjm Tjp Tm Tp     T at the point, at its lambda, row and level neighbours;  Uv Vv Wv: u, v, omega at the point
//   cx  ga gb gc  al be gm     d/dlon -> d/dx, the d/dlat and d/dp triples;  ta tb tc: the d/dt triple (DMODE 1, 2, 3)
//   po                         the point's offset from pD / pM / pP (DMODE 0, 1);  rT i otm otp: T's row and the time offsets (DMODE 2, 3)
//   c                          the record of (t, k, j): C_MT .. C_GE
// Defines yAe yKe yCa yCe yCk yGe (and d adv sP sS dTdt rest fq a b v w q wT vv uu on the way).
        // Q / cp = dT/dt + u dT/dx + v dT/dy - S w: stage_row's expression (lec_rowspecq.hip), fma form kept
        // centred on a ring; one-sided at an open box's first and last column
        const double d = RING ? Tr - Tl : (first ? 2.0 * (Tr - Tc) : (last ? 2.0 * (Tc - Tl) : Tr - Tl));
        const double adv = (Uv * cx) * d;
        const double sP = stencil3(ga, Tjm, gc, Tjp, gb, Tc);
        const double sS = stencil3(al, Tm, gm, Tp, be, Tc);
        double dTdt;
        if (DMODE == 0) dTdt = pD[po];
        else if (DMODE == 1) dTdt = stencil3(ta, (double)pM[po], tc, (double)pP[po], tb, Tc);
        else dTdt = stencil3(ta, (double)rT[otm + i], tc, (double)rT[otp + i], tb, Tc);
        const double rest = dTdt + adv;
        const double fq = fma(-Wv, sS, fma(Vv, sP, rest));

        const double a = Tc - c[C_MT], b = Uv - c[C_MU], v = Vv - c[C_MV], w = Wv - c[C_MW];
        const double q = kCp * fq - c[C_MQ];
        const double wT = w * a, vv = v * v, uu = b * b;
        const double yAe = (a * a) * c[C_AE];
        const double yKe = uu + vv;
        const double yCa = -((v * a) * c[C_CA1] + wT * c[C_CA2]);
        const double yCe = -(c[C_CE] * wT);
        const double yCk = (b * v) * c[C_CK1] + vv * c[C_CK2] + uu * c[C_CK3] + (w * b) * c[C_DPU] + (w * v) * c[C_DPU];
        const double yGe = (q * a) * c[C_GE];
