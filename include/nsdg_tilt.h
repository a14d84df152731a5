/* nsdg_tilt.h -- the "sea-surface tilt" section of the C ABI of libnsdg.so (csrc/tilt.hip, csrc/mevp.hip: pack_node).
 * include/nsdg.h includes this file: a caller of the library includes nsdg.h and has these calls with it.  The section is a header of its
 * own with a table of its own: abi.TILT_SYMBOLS binds its functions, tests/test_gpu_tilt_stream_order.py holds each of them to stream
 * order.  Plain C99, like nsdg.h. */
#ifndef NSDG_TILT_H
#define NSDG_TILT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

struct nsdg_ctx;

/* ---- sea-surface tilt from a sea-surface height --------------------------------------------------------------------------------------
 * No counterpart in the reference snapshot.  Without this section the packing writes the tilt force -m g grad(eta) through the geostrophic
 * current, as -m f_c k x u_o:
 *
 *     c2 = mdt u0 + a tax - cor voc          cor = rho_ice h' f_c
 *     c3 = mdt v0 + a tay + cor uoc
 *
 * so that (uo, vo) serves twice, as the drag velocity and as the tilt.  That is exact only for a geostrophic current and is no tilt at all
 * where f_c = 0.
 *
 * A context may hold a sea-surface height: a device pointer `ssh` to (2nx+1)(2ny+1) doubles on the LOCAL CG2 lattice (ghost rows included,
 * the layout of uo, vo), in metres, and a gravity g [m s^-2].
 *
 * At packing time, per node (gx, gy), nn = 2nx+1, nm = 2ny+1 (the nodes are hx/2 apart):
 *
 *     sx = (eta[gx+1] - eta[gx-1]) / hx              1 <= gx <= nn-2
 *     sx = 2 (eta[1] - eta[0]) / hx                  gx = 0
 *     sx = 2 (eta[nn-1] - eta[nn-2]) / hx            gx = nn-1
 *     sy likewise along gy with hy
 *
 *     m_g = (rho_ice h') g                           h' = the thickness the packing uses for mdt and cor: snow load and floor included
 *     tx  = m_g sx                                   -- a statement of its own: the product is rounded before it meets the sum
 *     ty  = m_g sy                                   -- likewise
 *     c2  = mdt u0 + a tax - tx
 *     c3  = mdt v0 + a tay - ty
 *
 * A difference, then one IEEE division (the factor 2 is exact): nothing there can be contracted.  tx and ty REPLACE the terms -cor voc and
 * +cor uoc: the cor terms of the ocean current are not added.  Everything else in pack_node is the code that stands there: c[0], c[1],
 * c[4] = uoc, c[5] = voc (the drag velocity), T_b, the 2^100 scaling of an ice-free node -- which then feels the tilt with its floor mass --
 * and the constants of a land node.
 *
 * What is read of eta:
 *
 * - A land node reads nothing of eta.
 * - An ocean node reads eta at its four lattice neighbours (itself where it lies on the outermost row or column).  Every node of the
 *   lattice that is not a land node is a node of an ocean element, and so are its neighbours in the ocean element it belongs to.
 * - So eta MUST BE FINITE AT EVERY NODE OF EVERY OCEAN ELEMENT, and may be anything (NaN included) at a node all of whose elements are land.
 * - The outermost row or column of the local array takes the one-sided difference.  Like the one-sided nodal means there, it belongs to
 *   Dirichlet nodes or to ghost rows that never reach an owned value: 1 block equals N blocks.
 * - The centred difference is exact, up to rounding, for a quadratic eta.
 *
 * Without a field the context launches the instantiations it launched before this section existed and reads no byte it did not read.
 *
 * nsdg_tilt_set: records its arguments only.  NULL clears the field; gravity is then ignored.  gravity not finite or <= 0: NSDG_ERR_ARG and
 *   nothing changes.  Before nsdg_grid_set: NSDG_ERR_STATE.  An nsdg_grid_set that changes the shape clears the field, the same shape keeps
 *   it.  The array belongs to the caller; it is read, stream-ordered, by the next nsdg_mevp_prepare, nsdg_mevp_pack_nodal, nsdg_mevp_subcycle
 *   (which packs) or nsdg_tilt_nodal.  A field that overlaps `packed` is NSDG_ERR_ARG at the packing call, with nothing launched.  The passes
 *   read c2, c3 as ever: nsdg_mevp_iterate*, nsdg_mevp_velocity, nsdg_bbm_iterate, nsdg_rb_mevp_run and nsdg_rb_bbm_run get the tilt with the
 *   packing they read.
 * nsdg_tilt_nodal: one launch: sx[n], sy[n] = the gradient the next packing would use, at every node n of the local lattice, land included
 *   (there it is whatever eta gives), (2nx+1)(2ny+1) doubles each.  Without a field: NSDG_ERR_STATE; a null pointer: NSDG_ERR_ARG.
 * nsdg_boxtest_ssh: one launch: the eta whose geostrophic current is the box test's gyre (nsdg_boxtest_forcing: uo, vo),
 *       eta = -(fc / g) (0.01 / L) [x (x - L) + y (y - L)],
 *   x, y those of nsdg_boxtest_forcing on the local array placed by nsdg_block_set, L = domain_size.  g eta_x = fc vo and g eta_y = -fc uo
 *   there.  domain_size <= 0, fc not finite, gravity not finite or <= 0, a null pointer: NSDG_ERR_ARG.
 * All three are stream-ordered on the context's stream; the setter only records its arguments. */
#define NSDG_GRAVITY 9.81
int nsdg_tilt_set(struct nsdg_ctx* ctx, const double* ssh, double gravity);
int nsdg_tilt_nodal(struct nsdg_ctx* ctx, double* sx, double* sy);
int nsdg_boxtest_ssh(struct nsdg_ctx* ctx, double domain_size, double fc, double gravity, double* ssh);

#ifdef __cplusplus
}
#endif

#endif /* NSDG_TILT_H */
