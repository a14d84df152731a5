/* nsdg_budget.h -- the "momentum budget" section of the C ABI of libnsdg.so (csrc/budget.hip).
 * include/nsdg.h includes this file: a caller of the library includes nsdg.h and has these calls with it.  The section is a header of its
 * own with a table of its own: abi.BUDGET_SYMBOLS binds its functions, tests/test_gpu_budget_stream_order.py holds the launch to stream
 * order.  Plain C99, like nsdg.h. */
#ifndef NSDG_BUDGET_H
#define NSDG_BUDGET_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

struct nsdg_ctx;

/* ---- momentum balance diagnostics: nodal forces and their power ----------------------------------------------------------------------
 * No counterpart in the reference snapshot.  The sub-cycle solves, per CG2 node, the implicit step of the momentum equation
 *
 *     m (u - u^n) / dt = a tau_a + drag (u_o - u) + m f_c k x (u_o - u) [or - m g grad(eta)] + div(sigma) / M - C_b u
 *
 * and what leaves it is a velocity.  nsdg_momentum_budget evaluates every term of that balance, in N m^-2, at ONE state: the velocity
 * (u, v) and the stress S the sub-cycle left, with the coefficients of the packing it ran with -- `packed`, and the context's pack_dt and
 * flags of that packing (land mask seen, depth seen) -- and the context's sea-surface height, gravity and parameters as they are now.  It
 * depends neither on alpha, beta nor on the form of the sub-cycle (uniform or adaptive): the balance does not see them.
 *
 * Per node, with c[0..5] its packed coefficients (csrc/mevp_common.h) and tb its seventh:
 *
 *     free  = c[0] > 2^50                 an ice-free node: the packing scaled c[0..3] by 2^100
 *     s     = free ? 2^-100 : 1           (a power of two: every product by s is exact)
 *     h'    = s c[0]      cd = s c[1]     c2 = s c[2]      c3 = s c[3]      u_o = c[4]      v_o = c[5]
 *     m     = rho_ice h'
 *     a     = free ? 1 : min(max(cgA, 0), 1),   cgA = the nodal mean of A, summed as nsdg_dg_to_cg(6) sums it
 *     mdt   = rho_ice h' / dt             dt = the packing's
 *     cor   = K3 h'                       K3 = rho_ice f_c, the launch constant of the node update
 *
 *   term        id   x component                         y component
 *   wind         0   a tau_ax                            a tau_ay               tau_a = f_atm |u_a| u_a, f_atm = c_atm rho_atm, as the packing
 *   water        1   drag (u_o - u)                      drag (v_o - v)         drag = cd fast_sqrt((u_o - u)^2 + (v_o - v)^2), as the node update
 *   coriolis     2   + cor v                             - cor u
 *   tilt         3   - cor v_o                           + cor u_o              no sea-surface height on the context
 *                    - m_g sx                            - m_g sy               with one: m_g = (rho_ice h') g, (sx, sy) of nsdg_tilt.h
 *   internal     4   div_x ilumped                       div_y ilumped          the gather of nsdg_mevp_velocity, in its order; exactly 0 at an
 *                                                                               ice-free node, where the sub-cycle weights it by 2^-100
 *   basal        5   - C_b u                             - C_b v                C_b = tb fast_rcp(fast_sqrt(u^2 + v^2) + u0); 0 without a packed depth
 *   inertia      6   (c2 - wind_x - tilt_x) - mdt u      (c3 - wind_y - tilt_y) - mdt v
 *   residual     7   R_x                                 R_y
 *
 * inertia is -m (u - u^n) / dt, recovered from c2 = mdt u^n + wind_x + tilt_x without keeping u^n.  The residual is formed from the packed
 * coefficients in the shape of the node update, NOT as the sum of the reported terms:
 *
 *     R_x = ((((c2 - mdt u) + water_x) + coriolis_x) + internal_x) + basal_x
 *     R_y = ((((c3 - mdt v) + water_y) + coriolis_y) + internal_y) + basal_y
 *
 * the defect of the implicit step that the converged sub-cycle solves: under uniform alpha = beta one more node update u -> u' gives
 * R = (K2 h' + drag + C_b) (u' - u).  Every product above is a statement of its own (-ffp-contract=on fuses inside one expression only):
 * nothing is contracted, and tests/budget_ref.py restates the arithmetic operation for operation.
 *
 * Every term is EXACTLY 0, and no constraint force is computed,
 *   - at a land node (c[1] < 0), and
 *   - at the Dirichlet nodes of the local lattice edge: the zeros nsdg_mevp_velocity writes (left column, bottom row, and the right column
 *     and top row that no element owns).
 * Forcing at a land node (wind, current, sea-surface height) may be anything, NaN included: the kernel selects, it does not multiply by
 * a mask, and reads nothing of eta at a land node.  H is not read -- the thickness of the balance is the packing's h' --: the argument stands
 * in the signature beside A as in nsdg_mevp_prepare, must not be NULL, and takes no part in the overlap check.
 *
 * struct nsdg_budget_out: sixteen planes of (2nx+1)(2ny+1) doubles on the local CG2 lattice, a NULL plane is not stored; and the totals.
 *
 * Row range and node ownership are those of nsdg_mevp_velocity: element rows [j0, j1) write the four nodes each element owns (vertex,
 * bottom edge, left edge, centre) and the zeros of the right column and top row.  Stream-ordered on the context's stream, one launch, no
 * synchronisation.
 *
 * TOTALS (power != NULL): per element row iy in [j0, j1), over the nodes that row owns, for each term t = 0..7
 *
 *     power[t * power_stride + (iy - row0)] = sum_n M_n (u F_x + v F_y)        [W]
 *     power[8 * power_stride + (iy - row0)] = sum_n (1/2) M_n m (u^2 + v^2)    [J]   (NSDG_BUDGET_KE)
 *
 * M_n = the lumped mass of the node, hx hy / 9 (vertex), hx hy / 4.5 (edge), hx hy / 2.25 (centre): one IEEE division each.  The order
 * of the sums is fixed.  One wave64 works on a row; lane l folds the elements ix = l, l + 64, ... in ascending order from 0, each element
 * adding its vertex, bottom edge, left edge and centre in that order; per node
 *
 *     pa = u F_x;  pb = v F_y;  ps = pa + pb;  p = M_n ps;  acc_t = acc_t + p
 *     qa = u u;    qb = v v;    qs = qa + qb;  e = m qs;    eh = 0.5 e;   k = M_n eh;   acc_8 = acc_8 + k
 *
 * every product a statement of its own; then the lanes are folded by halves, p_l = p_l + p_(l + s) for s = 32 ... 1 (__shfl_down: no LDS,
 * no atomics), and lane 0 stores.  A row's total therefore does not depend on launch geometry or decomposition, and adding the rows in row
 * order gives domain totals that are bit for bit independent of the number of row blocks.  Need 0 <= j0 - row0 and j1 - row0 <=
 * power_stride (so power_stride >= j1 - j0).
 *
 * nsdg_momentum_budget: NSDG_ERR_STATE before nsdg_grid_set or without a packing on the context (pack_dt <= 0); NSDG_ERR_ARG for a row
 *   range outside the local array, a null input or `out`, a tiled stress array that is not 16-byte aligned (so is `packed`), an output plane
 *   or `power` that overlaps an input that is read (not H), `packed`, the context's sea-surface height or another output, and
 *   power_stride or row0 that do not hold the rows.  Every error launches nothing.  An empty range, or an `out` without a plane and without `power`, is NSDG_OK and launches
 *   nothing.
 * nsdg_budget_term_id: the id of a term by name, "wind" 0 ... "residual" 7; -1 for an unknown name or NULL.  Host only. */
#define NSDG_BUDGET_TERMS 8
#define NSDG_BUDGET_KE 8 /* the ninth quantity of the totals */
#define NSDG_BUDGET_QUANTITIES 9

struct nsdg_budget_out {
    double *wind_x, *wind_y, *water_x, *water_y, *coriolis_x, *coriolis_y, *tilt_x, *tilt_y;
    double *internal_x, *internal_y, *basal_x, *basal_y, *inertia_x, *inertia_y, *residual_x, *residual_y; /* (2nx+1)(2ny+1) each; NULL: not stored */
    double* power; /* NSDG_BUDGET_QUANTITIES x power_stride; NULL: no totals */
    int64_t power_stride;
    int32_t row0;
};

int nsdg_momentum_budget(struct nsdg_ctx* ctx, int32_t j0, int32_t j1, const double* H, const double* A, const double* ua, const double* va,
    const double* s11, const double* s12, const double* s22, const double* u, const double* v, const double* packed,
    const struct nsdg_budget_out* out);
int nsdg_budget_term_id(const char* name);

#ifdef __cplusplus
}
#endif

#endif /* NSDG_BUDGET_H */
