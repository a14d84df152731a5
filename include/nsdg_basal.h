/* nsdg_basal.h -- the "landfast ice" section of the C ABI of libnsdg.so (csrc/basal.hip).  include/nsdg.h
 * includes this file: a caller of the library includes nsdg.h and has these calls with it.  The section is a header of its own with a
 * table of its own: abi.BASAL_SYMBOLS binds its functions, tests/test_gpu_basal_stream_order.py holds each of them to stream order.
 * Plain C99, like nsdg.h. */
#ifndef NSDG_BASAL_H
#define NSDG_BASAL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

struct nsdg_ctx;

/* ---- landfast ice: grounding on shoals as a basal stress in the momentum update ---------------------------------------------------------
 * No counterpart in the reference snapshot.  The grounding scheme of Lemieux et al. (2015, JGR 120, "A basal stress parameterization for
 * modeling landfast ice"; 2016, JGR 121): where ridge keels reach the seabed the ice feels one more friction term.  depth[iy * nx + ix] >= 0
 * is the static water depth [m] per element of the LOCAL array, ghost rows included.  Every CG2 node gets, at packing time,
 *     h_wn = the mean of depth over the 1 / 2 / 4 elements adjacent to the node inside the local array (the rule of the nodal means of H, A)
 *     a    = clamp(cgA, 0, 1),  h = cgH (NOT raised to the mass floor h_min),  h_c = a h_wn / k1
 *     T_b  = k2 max(0, h - h_c) exp(-alpha_b (1 - a))                                                              [N m^-3 m = N m^-2]
 *     T_b  = 0 at a land node (nsdg_land_mask_set) and at an ice-free node (the rule of nsdg_mevp_params.min_conc / min_thick / h_min):
 *            land and the ice-free rule keep their precedence
 * and in every sub-iteration the seabed stress tau_b = -C_b u^p, C_b = T_b / (|u^(p-1)| + u0), implicit like the ocean drag, is one more
 * term of the denominator of the velocity update (nsdg.h, nsdg_mevp_velocity):
 *     u^p = [ ... unchanged numerator ... ] / ((m / dt)(1 + beta) + c + C_b)                                                (v^p alike)
 * |u^(p-1)| is the speed of the ice itself, not its speed relative to the ocean.  The term is implicit and non-negative: it adds no
 * stability condition (nsdg_mevp_stable_params and nsdg_substep_count are what they were).  The brittle sub-cycle (nsdg_bbm_iterate) runs
 * the same node update and gets the same term.
 *
 * nsdg_basal_default_params: the published values k1 = 8, k2 = 15 N m^-3, alpha_b = 20, u0 = 5e-5 m/s (host only, no context).
 * nsdg_basal_params_set: k1 > 0, k2 >= 0, alpha_b >= 0, u0 > 0, all finite; otherwise (or a null argument) NSDG_ERR_ARG and nothing
 *   changes.  A new context holds the defaults.  Acts from the next coefficient packing on.
 * nsdg_basal_depth_set: `depth` is a device pointer to nx * ny doubles on the LOCAL array, ghost rows included, owned by the caller and
 *   valid while it is set; stream-ordered like every other array argument.  NULL clears it.  Before nsdg_grid_set: NSDG_ERR_STATE.  An
 *   nsdg_grid_set that changes the shape clears the array, the same shape keeps it.  The depth acts through the coefficient packing:
 *   nsdg_mevp_prepare / nsdg_mevp_pack_nodal (and nsdg_mevp_subcycle, which packs) store T_b as the seventh of the eight packed
 *   coefficients of a node (the eighth is 0), and every pass that reads that packing -- nsdg_mevp_iterate*, nsdg_mevp_velocity,
 *   nsdg_bbm_iterate, nsdg_rb_mevp_run, nsdg_rb_bbm_run -- adds the term.  Where T_b = 0 such a pass gives, bit for bit, what the pass
 *   without a depth array gives; a context without a depth array runs the same kernels as ever and reads no byte it did not read before.
 * nsdg_basal_critical: one launch: tb[n] = T_b at every node n of the local lattice, (2nx+1)(2ny+1) doubles, from the nodal means cgh, cga
 *   (nsdg_dg_to_cg): what the next packing would store, land mask and ice-free rule included.  Without a depth array: NSDG_ERR_STATE; a
 *   null pointer: NSDG_ERR_ARG.
 * All of them are stream-ordered on the context's stream; the setters only record their argument. */
typedef struct nsdg_basal_params {
    double k1;      /* keel depth per mean thickness: the ice grounds where h > a h_w / k1 */
    double k2;      /* maximum basal stress per metre of grounded thickness [N m^-3] */
    double alpha_b; /* concentration dependence, as the ice strength's compaction constant */
    double u0;      /* speed below which the stress passes from static to kinetic friction [m/s] */
} nsdg_basal_params;
void nsdg_basal_default_params(nsdg_basal_params* p);
int nsdg_basal_params_set(struct nsdg_ctx* ctx, const nsdg_basal_params* p);
int nsdg_basal_depth_set(struct nsdg_ctx* ctx, const double* depth);
int nsdg_basal_critical(struct nsdg_ctx* ctx, const double* cgh, const double* cga, double* tb);

#ifdef __cplusplus
}
#endif

#endif /* NSDG_BASAL_H */
