/* nsdg_snow.h -- the "snow load" section of the C ABI of libnsdg.so (csrc/snowload.hip, csrc/mevp.hip: pack_node).
 * include/nsdg.h includes this file: a caller of the library includes nsdg.h and has these calls with it.  The section is a header of its
 * own with a table of its own: abi.SNOW_SYMBOLS binds its functions, tests/test_gpu_snow_stream_order.py holds each of them to stream
 * order.  Plain C99, like nsdg.h. */
#ifndef NSDG_SNOW_H
#define NSDG_SNOW_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

struct nsdg_ctx;

/* ---- snow load: the momentum equation feels the snow's weight ---------------------------------------------------------------------------
 * No counterpart in the reference snapshot.  Without this section every kernel takes the nodal mass as m = rho_ice h', h' = max(cgH, h_min).
 *
 * A context may hold a snow field: a device pointer `snow` to `ncoef` coefficient planes of nx * ny doubles on the LOCAL array (ghost rows
 * included), and a density `rho_snow`.
 *
 * - ncoef = 1 is the column plane hsnow.  ncoef = 3 / 6 is the DG field S of the column-state transport.
 * - The ratio r = rho_snow / rho_ice is one IEEE division on the host.  rho_ice is that of the nsdg_mevp_params the context holds when the
 *   packing is launched.
 *
 * At packing time, per CG2 node:
 *
 *     cgS = the nodal mean of snow, by the rule and in the summation order of nsdg_dg_to_cg(ncoef)   (bit-identical to that call)
 *     s   = fmax(cgS, 0)
 *     p   = r * s
 *     hl  = cgH + p            -- a statement of its own: the product must not be contracted into the sum (-ffp-contract=on fuses inside one expression only)
 *     land node                          : unchanged (h' = h_min, the flag)
 *     ice-free node (rule evaluated on cgH, cgA exactly as today) : unchanged, h' = fmax(cgH, h_min): snow on no ice weighs nothing here (the column step deletes it)
 *     every other node                   : h' = fmax(hl, h_min)
 *
 * Everything after h' in pack_node is the code that stands there now: mdt, cor, the six coefficients, the 2^100 scaling.  The following keep
 * reading the ICE alone:
 *
 * - the seabed stress T_b (basal_critical_stress), which reads cgH itself;
 * - the ice strength;
 * - nsdg_concentration_max and nsdg_substep_count;
 * - nsdg_mevp_stable_params.
 *
 * A heavier node only loosens the stability bound  alpha beta >= c zeta dt / (m h^2).  The feature adds no stability condition.
 *
 * Three properties follow:
 *
 * - No load means no change.  Without a snow field the context launches the instantiations it launched before this section existed and reads
 *   no byte it did not read before.  With rho_snow = 0, or with snow that is <= 0 everywhere, p = 0 and hl = cgH: `packed` is then bit for
 *   bit what it is without a field.
 * - The load is a substitution.  p >= 0, so hl >= cgH: a node that is not ice-free on (cgH, cgA) is not ice-free on (hl, cgA) either.  So the
 *   six coefficients packed WITH a snow field equal, bit for bit, those packed WITHOUT one from the nodal thickness
 *   cgH_ref = where(ice_free(cgH, cgA), cgH, hl).  T_b under a depth array still comes from cgH.
 * - Decomposition.  hsnow on ghost rows equals its owner without a message (the column step runs there redundantly), and S is exchanged by
 *   the transport.  So no new exchange is needed, and 1 block equals N blocks.
 *
 * nsdg_snow_load_set: records its arguments only.  NULL clears the field; ncoef and rho_snow are then ignored.  ncoef must be one of 1, 3, 6;
 *   rho_snow must be finite and >= 0; otherwise NSDG_ERR_ARG and nothing changes.  Before nsdg_grid_set: NSDG_ERR_STATE.  An nsdg_grid_set
 *   that changes the shape clears the field, the same shape keeps it.  The array belongs to the caller; it is read, stream-ordered, by the
 *   next nsdg_mevp_prepare, nsdg_mevp_pack_nodal, nsdg_mevp_subcycle (which packs) or nsdg_snow_load_nodal.  A field that overlaps `packed`
 *   is NSDG_ERR_ARG at the packing call, with nothing launched.  The passes read c[0] = h' as ever: nsdg_mevp_iterate*, nsdg_mevp_velocity,
 *   nsdg_bbm_iterate, nsdg_rb_mevp_run and nsdg_rb_bbm_run get the load with the packing they read.
 * nsdg_snow_load_nodal: one launch: hload[n] = the h' the next packing would store as c[0] before its 2^100 scaling, land mask and ice-free
 *   rule included, at every node n of the local lattice, (2nx+1)(2ny+1) doubles, from the nodal means cgh, cga (nsdg_dg_to_cg).  Without a
 *   field: NSDG_ERR_STATE; a null pointer: NSDG_ERR_ARG.
 * Both are stream-ordered on the context's stream; the setter only records its arguments. */
#define NSDG_SNOW_DENSITY 330.0   /* the column step's rho_s */
int nsdg_snow_load_set(struct nsdg_ctx* ctx, const double* snow, int32_t ncoef, double rho_snow);
int nsdg_snow_load_nodal(struct nsdg_ctx* ctx, const double* cgh, const double* cga, double* hload);

#ifdef __cplusplus
}
#endif

#endif /* NSDG_SNOW_H */
