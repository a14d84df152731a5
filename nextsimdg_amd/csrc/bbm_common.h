// bbm_common.h -- the element arithmetic of the brittle Bingham-Maxwell (BBM) sub-cycle (include/nsdg.h "brittle rheology", DESIGN.md
// section 3.8; Olason et al. 2022, Dansereau et al. 2016), stated ONCE and inlined by the kernel that needs it (bbm.hip).  Built from the
// element operators of mevp_common.h: the strain rate at the 3x3 Gauss points, the evaluation and the L2 projection of an
// 8-coefficient function, and the division-free elementary functions.  The node arithmetic of the BBM momentum step is the mEVP one
// (mevp_common.h: node_update) with other launch constants; nothing of it is restated here.
#pragma once
#include "mevp_common.h"

namespace nsdg_mevp_detail {

// launch constants of the element step, formed once per launch on the host (bbm.hip: nsdg_bbm_consts)
struct BbmConsts {
    double dts; // the sub-step length: the packing's time step
    double heal; // dts / t_heal
    double d_max;
    double young, lambda0;
    double k1, k2; // 1 / (1 + nu), nu / (1 - nu^2)
    double tan_phi, coh, N; // coh = cohesion_lab sqrt(0.1 / h), N = compr_strength
    double rc; // dts / (h sqrt(2 (1 + nu) rho_ice)): the damage rate is min(1, rc sqrt(E))
    int nrelax; // relax_exponent - 1 multiplications
};

// One element, one sub-iteration: elastic predictor, Maxwell relaxation, Mohr-Coulomb test and damage update at the 9 Gauss points, in
// the order of include/nsdg.h "brittle rheology" (steps 1-8).  In: the 9 nodal velocities, the old stress (Pa, not thickness-integrated)
// and damage coefficients, and the three per-step Gauss arrays hg, eg, pm of nsdg_bbm_prepare.  Out: s?? = the new stress coefficients,
// d = the new damage coefficients, m?? = the coefficients of the thickness-integrated stress hg sigma that the momentum equation takes.
// Every reciprocal is a fast_rcp whose operand is finite and non-zero in the branch that uses the result.
__device__ __forceinline__ void bbm_element_step(const BbmConsts& B, const double (&ul)[9], const double (&vl)[9], double ihx, double ihy,
    const double (&hg)[9], const double (&eg)[9], const double (&pm)[9], double (&s11)[8], double (&s12)[8], double (&s22)[8], double (&d)[6],
    double (&m11)[8], double (&m12)[8], double (&m22)[8])
{
    double e11[9], e12[9], e22[9];
    strain_rate_gauss(ul, vl, ihx, ihy, e11, e12, e22);
    double t11[9], t12[9], t22[9], dq[9];
    sf_eval<0>(s11, t11);
    sf_eval<0>(s12, t12);
    sf_eval<0>(s22, t22);
    {
        const double dc[8] = { d[0], d[1], d[2], d[3], d[4], d[5], 0., 0. };
        sf_eval<0>(dc, dq);
    }
    double w11[9], w12[9], w22[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) {
        // 1. clamp and heal
        double dd = fmin(fmax(dq[q], 0.), B.d_max);
        dd = fmax(0., dd - B.heal);
        // 2. stiffness and relaxation time
        const double x = (1. - dd) * eg[q];
        const double E = B.young * x;
        double lam = B.lambda0;
        for (int k = 0; k < B.nrelax; ++k) // wave-uniform trip count
            lam *= x;
        // 3. compressive limit, from the old stress
        const double sn0 = 0.5 * (t11[q] + t22[q]);
        const double Pt = sn0 < 0. ? fmin(1., -pm[q] * fast_rcp(sn0)) : 0.;
        // 4. relaxation multiplier
        const double mlt = fmin(1. - 1e-12, lam * fast_rcp(lam + B.dts * (1. - Pt)));
        // 5. elastic predictor and relaxation
        const double dE = B.dts * E, tr = e11[q] + e22[q];
        double a11 = (t11[q] + dE * (B.k1 * e11[q] + B.k2 * tr)) * mlt;
        double a22 = (t22[q] + dE * (B.k1 * e22[q] + B.k2 * tr)) * mlt;
        double a12 = (t12[q] + dE * (B.k1 * e12[q])) * mlt;
        // 6. Mohr-Coulomb on the new stress
        const double sn = 0.5 * (a11 + a22), hd = 0.5 * (a11 - a22);
        const double ss = fast_sqrt(hd * hd + a12 * a12);
        const double den = ss + B.tan_phi * sn;
        double dcrit = 1.;
        if (sn < -B.N)
            dcrit = -B.N * fast_rcp(sn);
        else if (den > B.coh)
            dcrit = B.coh * fast_rcp(den);
        // 7. damage update
        const double r = fmin(1., B.rc * fast_sqrt(E));
        const double f = (1. - dcrit) * r;
        dq[q] = fmin(B.d_max, dd + (1. - dd) * f);
        const double keep = 1. - f;
        a11 *= keep, a22 *= keep, a12 *= keep;
        t11[q] = a11, t22[q] = a22, t12[q] = a12;
        w11[q] = hg[q] * a11, w22[q] = hg[q] * a22, w12[q] = hg[q] * a12;
    }
    // 8. projection: the stress, the damage (coefficients 0..5 of the orthogonal basis are the DG2 projection), the integrated stress
    sf_project(t11, ProjUnit {}, s11);
    sf_project(t12, ProjUnit {}, s12);
    sf_project(t22, ProjUnit {}, s22);
    {
        double dp[8];
        sf_project(dq, ProjUnit {}, dp);
#pragma unroll
        for (int c = 0; c < 6; ++c)
            d[c] = dp[c];
    }
    sf_project(w11, ProjUnit {}, m11);
    sf_project(w12, ProjUnit {}, m12);
    sf_project(w22, ProjUnit {}, m22);
}

} // namespace nsdg_mevp_detail
