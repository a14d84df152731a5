/* nsdg_ocean.h -- the "slab ocean" section of the C ABI of libnsdg.so (csrc/column_step.hip).  include/nsdg.h
 * includes this file: a caller of the library includes nsdg.h and has these calls with it.  The section is a header of its own with a
 * table of its own: abi.OCEAN_SYMBOLS binds its functions, tests/test_gpu_slab_stream_order.py holds each of them to stream order.
 * Plain C99, like nsdg.h. */
#ifndef NSDG_OCEAN_H
#define NSDG_OCEAN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

struct nsdg_ctx;

/* ---- slab ocean: the mixed layer's heat and salt follow the ice ---------------------------------------------------------------------------
 * No counterpart in the reference snapshot, whose column step reads the mixed-layer temperature sst and salinity sss and never changes
 * them.  nsdg_column_step_ocean is nsdg_column_step (nsdg.h: the same 15 planes in the same order, the same parameters
 * nsdg_column_params_set, no diagnostics) that also advances sst and sss, in place, by the fluxes the column step has computed.  The ice
 * outputs hice, cice, hsnow, tice0, newice are, bit for bit, those of nsdg_column_step.
 *
 * Per element: c, H0, S0, T, S are cice, hice, hsnow, sst, sss before the step, H1, S1n are hice, hsnow after it (cell means), and Qio,
 * Qow, subl, evap the column step's FINAL ice-ocean and open-water heat fluxes [W m^-2, positive = the ocean loses], sublimation and
 * evaporation [kg m^-2 s^-1] (what the diagnostic planes NSDG_D_QIO, NSDG_D_QOW, NSDG_D_SUBL hold; evap = drag_ocean_q rho wind (q_w - q_a)
 * of NSDG_D_RHO, NSDG_D_QW, NSDG_D_QA).  rho_w = 1025, c_p = 4186.84, rho_i = 917, rho_s = 330 are the column step's constants.  Every
 * line is ONE IEEE fp64 operation, in this order, with plain divisions; nothing is fused:
 *
 *   heat   m1 = mld * rho_w        mlbhc = m1 * c_p                                       (the column step's own mixed-layer heat capacity)
 *          oc = 1 - c
 *          a  = c * Qio            b = oc * Qow          qnet = a + b
 *          e  = qnet * dt          q = e / mlbhc         T1 = T - q
 *          d  = T_ext - T          r = g_T * d           T1 = T1 + r                      only if relax_t > 0;  g_T = dt / relax_t
 *   salt   dh = H1 - H0            dMi = rho_i * dh
 *          ds = S1n - S0           dMs = rho_s * ds                                       [kg m^-2]
 *          f  = c * subl           g = oc * evap         v = f + g
 *          p  = snowfall - v       w = p * dt            w = w - dMi          W = w - dMs   water that enters the layer
 *          M  = rho_w * mld
 *          x  = M * S              y = S_i * dMi         z = x - y
 *          D  = M + W              S1 = z / D
 *          d  = S_ext - S          r = g_S * d           S1 = S1 + r                      only if relax_s > 0;  g_S = dt / relax_s
 *
 * W closes the water budget by construction (what the atmosphere delivers to the cell, minus what stays in the pack, goes to the ocean;
 * the slab keeps its volume), ice forms and melts at the salinity S_i, and the weights c, 1 - c are those of the concentration the step
 * started from.  mld, M + W and dt are not checked: a zero or negative denominator gives what IEEE gives.
 *
 * nsdg_slab_default_params: relax_t = relax_s = 0 (no relaxation), ice_salinity = 5 (the column step's ICE_S); host only, no context.
 * nsdg_slab_params_set: a negative or non-finite member (or a null argument): NSDG_ERR_ARG and nothing changes.  A new context holds the
 *   defaults.  Acts on the next nsdg_column_step_ocean.
 * nsdg_column_step_ocean: one launch (two elements per lane, 16-byte accesses) for the even part of planes that are all 16-byte aligned
 *   (skip: 2-byte aligned), and one launch of a one-element-per-lane kernel for the rest; stream-ordered on the context's stream.
 *   sst_ext, sss_ext: the relaxation targets, n doubles each, read only while the matching relaxation time is > 0 (NULL allowed
 *   otherwise).  skip: n bytes or NULL; a non-zero byte leaves that element's sst and sss bits as they were (a land element); the ice
 *   outputs do not depend on it.  NSDG_ERR_ARG, with nothing launched, for: a null context, n < 0, a null state or forcing pointer, a
 *   null target whose relaxation is on, and sst or sss overlapping each other or any other plane passed.  n == 0 does nothing. */
typedef struct nsdg_slab_params {
    double relax_t, relax_s; /* relaxation times of sst and sss towards their targets [s]; 0 = no relaxation (default) */
    double ice_salinity;     /* S_i: the salinity at which ice forms and melts (default 5, the column step's ICE_S) */
    int32_t reserved[2];
} nsdg_slab_params;
void nsdg_slab_default_params(nsdg_slab_params* p);
int nsdg_slab_params_set(struct nsdg_ctx* ctx, const nsdg_slab_params* p);
int nsdg_column_step_ocean(struct nsdg_ctx* ctx, int64_t n, double dt, double* hice, double* cice, double* hsnow, double* tice0,
    double* sst, double* sss, const double* tair, const double* tdew, const double* slp, const double* qsw, const double* qlw,
    const double* mld, const double* snowfall, const double* wind, double* newice, const double* sst_ext, const double* sss_ext,
    const uint8_t* skip);

#ifdef __cplusplus
}
#endif

#endif /* NSDG_OCEAN_H */
