// mevp.hip -- mEVP stress / velocity sub-cycle on a uniform rectangular mesh (CG2 velocity,
// 8-coefficient DG stress, 3x3 Gauss points) and the per-step helper kernels around it.
//
// No counterpart in the reference snapshot (CMakeLists.txt:43-46); the scheme is stated in
// DESIGN.md section 3.2 and restated on the CPU in oracle/dyn_oracle.c (parity unpinned).
//
// Variant 0 ("two-kernel"): per sub-iteration
//   mevp_stress_kernel   one lane per element: gathers its 9 nodal velocities, forms the strain-rate
//                        coefficients (sparse 8x9 constant operators folded into the instruction
//                        stream), evaluates the VP law at the 9 Gauss points, relaxes the 3x8 stress
//                        coefficients in place.
//   mevp_velocity_kernel one lane per element = its 4 bottom-left-owned nodes: gathers the stress
//                        of the (up to) 4 adjacent elements -- a node-centred gather, no atomics,
//                        deterministic and independent of the decomposition -- and applies the
//                        momentum update.
// Variant 1 ("fused march") lives in mevp_fused.hip.
#include <algorithm>
#include <initializer_list>
#include <type_traits>

#include "mevp_pipeline.h"

namespace nsdg_mevp_detail {

__global__ __launch_bounds__(256) void mevp_stress_kernel(int nx, int ny, int k0, int k1, double ihx, double ihy,
    double ialpha, double dmin2, const double* __restrict__ u, const double* __restrict__ v,
    const double* __restrict__ pg, const double* S11i, const double* S12i, const double* S22i, double* S11, double* S12,
    double* S22)
{
    // S??i may alias S?? (in-place update): every lane reads only its own element before writing it
    const int ix = blockIdx.x * 64 + threadIdx.x;
    const int iy = k0 + blockIdx.y * 4 + threadIdx.y;
    if (ix >= nx || iy >= k1)
        return;
    const int ntx = tiles_per_row(nx);
    const long ts = tile_off(ix, iy, ntx, 8), tp = tile_off(ix, iy, ntx, 9);
    const int nn = 2 * nx + 1;
    double ul[9], vl[9], P[9], s11[8], s12[8], s22[8];
#pragma unroll
    for (int a = 0; a < 9; ++a) {
        const long n = (long)(2 * iy + a / 3) * nn + 2 * ix + a % 3;
        ul[a] = u[n];
        vl[a] = v[n];
    }
    tile_load9(pg, tp, ix & 63, P);
    tile_load8(S11i, ts, s11);
    tile_load8(S12i, ts, s12);
    tile_load8(S22i, ts, s22);
    stress_update(ul, vl, P, ihx, ihy, ialpha, dmin2, s11, s12, s22);
    tile_store8(S11, ts, s11);
    tile_store8(S12, ts, s12);
    tile_store8(S22, ts, s22);
}

__device__ __forceinline__ void load_stress(const double* __restrict__ S11, const double* __restrict__ S12,
    const double* __restrict__ S22, long ts, double (&s11)[8], double (&s12)[8], double (&s22)[8])
{
    tile_load8(S11, ts, s11);
    tile_load8(S12, ts, s12);
    tile_load8(S22, ts, s22);
}

// the velocity kernel's body; LAND: the instantiation that holds land nodes at 0 (mevp_common.h: node_update); BASAL: the one that reads
// the fourth coefficient pair and adds the seabed stress
template <bool LAND, bool BASAL>
__device__ __forceinline__ void mevp_velocity_body(NodalConstsOf<BASAL> K, int nx, int ny, int j0, int j1, double hx, double hy,
    const double* __restrict__ S11, const double* __restrict__ S12, const double* __restrict__ S22,
    const double* __restrict__ u_old, const double* __restrict__ v_old, const double* __restrict__ packed,
    double* __restrict__ u_new, double* __restrict__ v_new)
{
    const int ix = blockIdx.x * 64 + threadIdx.x;
    const int iy = j0 + blockIdx.y * 4 + threadIdx.y;
    if (ix >= nx || iy >= j1)
        return;
    const int ntx = tiles_per_row(nx);
    const int nn = 2 * nx + 1;
    const long nplane = nodal_plane((long)nn * (2 * ny + 1));
    const double iarea = 1. / (hx * hy);
    double s11[8], s12[8], s22[8];
    double cx, cy;
    // node sums, accumulated in the order below-left, below, left, own (same as the oracle)
    double vx_ = 0., vy_ = 0., exx = 0., exy = 0., eyx = 0., eyy = 0., ccx, ccy;
    const bool hasL = ix > 0, hasB = iy > 0;
    if (hasL && hasB) {
        load_stress(S11, S12, S22, tile_off(ix - 1, iy - 1, ntx, 8), s11, s12, s22);
        node_contrib<8>(s11, s12, s22, hx, hy, cx, cy);
        vx_ += cx, vy_ += cy;
    }
    if (hasB) {
        load_stress(S11, S12, S22, tile_off(ix, iy - 1, ntx, 8), s11, s12, s22);
        node_contrib<6>(s11, s12, s22, hx, hy, cx, cy);
        vx_ += cx, vy_ += cy;
        node_contrib<7>(s11, s12, s22, hx, hy, cx, cy);
        exx += cx, exy += cy;
    }
    if (hasL) {
        load_stress(S11, S12, S22, tile_off(ix - 1, iy, ntx, 8), s11, s12, s22);
        node_contrib<2>(s11, s12, s22, hx, hy, cx, cy);
        vx_ += cx, vy_ += cy;
        node_contrib<5>(s11, s12, s22, hx, hy, cx, cy);
        eyx += cx, eyy += cy;
    }
    load_stress(S11, S12, S22, tile_off(ix, iy, ntx, 8), s11, s12, s22);
    node_contrib<0>(s11, s12, s22, hx, hy, cx, cy);
    vx_ += cx, vy_ += cy;
    node_contrib<1>(s11, s12, s22, hx, hy, cx, cy);
    exx += cx, exy += cy;
    node_contrib<3>(s11, s12, s22, hx, hy, cx, cy);
    eyx += cx, eyy += cy;
    node_contrib<4>(s11, s12, s22, hx, hy, ccx, ccy);

    const long nV = (long)(2 * iy) * nn + 2 * ix; // vertex; EX = nV+1; EY = nV+nn; C = nV+nn+1
    double un[4], vn[4], c[6];
    // inverse lumped masses: 4, 2, 2, 1 adjacent elements times LUMP = 1/36, 1/9, 1/9, 4/9 of the cell area
    if (hasL && hasB) { // vertex
        load_nodal(packed, nplane, nV, c);
        node_update<false, LAND, BASAL>(K, c, u_old[nV], v_old[nV], vx_, vy_, 9. * iarea, un[0], vn[0], 0., 0., BASAL ? load_nodal_tb(packed, nplane, nV) : 0., nodal_u0<BASAL>(K));
    } else
        un[0] = vn[0] = 0.;
    if (hasB) { // bottom edge-mid
        load_nodal(packed, nplane, nV + 1, c);
        node_update<false, LAND, BASAL>(K, c, u_old[nV + 1], v_old[nV + 1], exx, exy, 4.5 * iarea, un[1], vn[1], 0., 0., BASAL ? load_nodal_tb(packed, nplane, nV + 1) : 0., nodal_u0<BASAL>(K));
    } else
        un[1] = vn[1] = 0.;
    if (hasL) { // left edge-mid
        load_nodal(packed, nplane, nV + nn, c);
        node_update<false, LAND, BASAL>(K, c, u_old[nV + nn], v_old[nV + nn], eyx, eyy, 4.5 * iarea, un[2], vn[2], 0., 0., BASAL ? load_nodal_tb(packed, nplane, nV + nn) : 0., nodal_u0<BASAL>(K));
    } else
        un[2] = vn[2] = 0.;
    load_nodal(packed, nplane, nV + nn + 1, c); // centre
    node_update<false, LAND, BASAL>(K, c, u_old[nV + nn + 1], v_old[nV + nn + 1], ccx, ccy, 2.25 * iarea, un[3], vn[3], 0., 0., BASAL ? load_nodal_tb(packed, nplane, nV + nn + 1) : 0., nodal_u0<BASAL>(K));
    // with the zeros of the right column / top row of the local lattice: boundary nodes (v = 0)
    store_owned_nodes(nV, nn, ix == nx - 1, iy == ny - 1, un, vn, u_new, v_new);
}

__global__ __launch_bounds__(256) void mevp_velocity_kernel(NodalConsts K, int nx, int ny, int j0, int j1, double hx, double hy,
    const double* __restrict__ S11, const double* __restrict__ S12, const double* __restrict__ S22,
    const double* __restrict__ u_old, const double* __restrict__ v_old, const double* __restrict__ packed,
    double* __restrict__ u_new, double* __restrict__ v_new)
{
    mevp_velocity_body<false, false>(K, nx, ny, j0, j1, hx, hy, S11, S12, S22, u_old, v_old, packed, u_new, v_new);
}

// the same after a packing that saw a land mask
__global__ __launch_bounds__(256) void mevp_velocity_land_kernel(NodalConsts K, int nx, int ny, int j0, int j1, double hx, double hy,
    const double* __restrict__ S11, const double* __restrict__ S12, const double* __restrict__ S22,
    const double* __restrict__ u_old, const double* __restrict__ v_old, const double* __restrict__ packed,
    double* __restrict__ u_new, double* __restrict__ v_new)
{
    mevp_velocity_body<true, false>(K, nx, ny, j0, j1, hx, hy, S11, S12, S22, u_old, v_old, packed, u_new, v_new);
}

// the same after a packing that saw a depth array (landfast ice, basal.hip), masked or not
template <bool LAND>
__global__ __launch_bounds__(256) void mevp_velocity_basal_kernel(NodalConstsBasal K, int nx, int ny, int j0, int j1, double hx, double hy,
    const double* __restrict__ S11, const double* __restrict__ S12, const double* __restrict__ S22,
    const double* __restrict__ u_old, const double* __restrict__ v_old, const double* __restrict__ packed,
    double* __restrict__ u_new, double* __restrict__ v_new)
{
    mevp_velocity_body<LAND, true>(K, nx, ny, j0, j1, hx, hy, S11, S12, S22, u_old, v_old, packed, u_new, v_new);
}

// ---------------------------------------------------------------------------------------------
// psi_rt, node_average: mevp_common.h
// per-step momentum coefficients of one node, 6 doubles (layout: mevp_common.h); BASAL: pair 3 = (T_b, 0) from the node's mean water
// depth hwn as well (landfast ice, mevp_common.h: basal_critical_stress); SNOW: the mass of a node that is neither land nor ice-free
// carries the snow's nodal mean cgs, weighted by r = rho_snow / rho_ice (snow load, mevp_common.h: snow_loaded_thickness); TILT: the
// sea-surface tilt is -m g (sx, sy) from the gradient of a sea-surface height (include/nsdg_tilt.h, mevp_common.h: tilt_gradient) in
// place of the Coriolis terms of the ocean current
template <bool BASAL, bool SNOW, bool TILT>
__device__ __forceinline__ void pack_node(const nsdg_mevp_params& P, double dt, double u0, double v0, double tax, double tay,
    double uoc, double voc, double cgh, double cga, double* __restrict__ packed, long plane, long n, bool land, const nsdg_basal_params& B, double hwn,
    double r, double cgs, double g, double sx, double sy)
{
    if constexpr (BASAL)
        store_nodal_tb(packed, plane, n, basal_critical_stress(P, B, cgh, cga, hwn, land));
    // Land node (csrc/landmask.hip; before the ice-free rule): the flag cd = c[1] < 0 -- every real node has cd >= 0, and a signed zero
    // cannot serve under -fno-signed-zeros -- beside fixed finite constants that depend neither on the forcing nor on H and A there
    // (h' = h_min: the adaptive form divides by the centre node's h').  The LAND kernels hold such a node at u = v = 0.
    if (land) {
        const double c[6] = { P.h_min, -1., 0., 0., 0., 0. };
        store_nodal(packed, plane, n, c);
        return;
    }
    double h = fmax(cgh, P.h_min);
    // Ice-free-node rule (round 5; the shape of the column model's cut-off  c_new < minc || hi < minh,
    // physics/src/modules/NextsimPhysics.cpp:210-219): a node whose mean concentration is below min_conc, whose TRUE thickness
    // cgH / cgA is below min_thick or whose mean thickness is at the mass floor h_min (a made-up mass) is in FREE DRIFT -- full exposure (a = 1) to wind stress and ocean drag, Coriolis, its floor mass
    // -- and does not feel the stress divergence of the neighbouring elements.  That costs the sub-cycle NOTHING: the update is
    //   u' = (K1 h' u + c2 + drag u_o + K3 h' v + div_x / M) / (K2 h' + drag),  drag = cd |v_o - v|,
    // homogeneous of degree 0 in (h', cd, c2, c3, div): scaling the four packed coefficients by 2^100 (exact: a power of two)
    // leaves every other term as it is and weights the divergence by 2^-100 -- below the last bit of the sum.  Both 0: rule off.
    // (the expression of mevp_common.h: ice_free_node, which T_b tests; written out here, where it has always stood)
    const bool ice_free = (P.min_conc > 0. || P.min_thick > 0.) && (cga < P.min_conc || cgh < P.min_thick * cga || cgh <= P.h_min);
    if constexpr (SNOW)
        if (!ice_free)
            h = fmax(snow_loaded_thickness(cgh, r, cgs), P.h_min);
    const double a = ice_free ? 1. : fmin(fmax(cga, 0.), 1.);
    const double mdt = P.rho_ice * h / dt;
    const double cor = P.rho_ice * h * P.fc;
    const double w = ice_free ? 0x1p100 : 1.;
    if constexpr (TILT) {
        // the products are statements of their own: rounded before they meet the sum (-ffp-contract=on fuses inside one expression only)
        const double m_g = (P.rho_ice * h) * g;
        const double tx = m_g * sx;
        const double ty = m_g * sy;
        const double c[6] = { w * h, w * (a * (P.c_ocean * P.rho_ocean)), w * (mdt * u0 + a * tax - tx), w * (mdt * v0 + a * tay - ty), uoc, voc };
        store_nodal(packed, plane, n, c);
        return;
    }
    const double c[6] = { w * h, w * (a * (P.c_ocean * P.rho_ocean)), w * (mdt * u0 + a * tax - cor * voc), w * (mdt * v0 + a * tay + cor * uoc), uoc, voc };
    store_nodal(packed, plane, n, c);
}

// wind_tau: mevp_common.h
// LAND: with the element land mask of the local array (nx x ny elements), land nodes are packed with the flag
// BASAL: with the water depth of the same elements, pair 3 of a node is (T_b, 0)
// SNOW: with the ncs coefficient planes of the snow on the same elements, the mass of a node carries its nodal mean
// TILT: with the sea-surface height on the nodes, an ocean node reads it at its four lattice neighbours; a land node reads nothing of it
template <bool LAND, bool BASAL, bool SNOW, bool TILT>
__global__ __launch_bounds__(256) void mevp_pack_nodal_kernel(nsdg_mevp_params P, long nnodes, double dt,
    const double* __restrict__ u0, const double* __restrict__ v0, const double* __restrict__ tax,
    const double* __restrict__ tay, const double* __restrict__ uo, const double* __restrict__ vo,
    const double* __restrict__ cgh, const double* __restrict__ cga, double* __restrict__ packed, int nx, int ny, const uint8_t* __restrict__ land,
    nsdg_basal_params B, const double* __restrict__ depth, const double* __restrict__ snow, int ncs, double r,
    const double* __restrict__ ssh, double g, double hx, double hy)
{
    const long n = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= nnodes)
        return;
    const int nn = 2 * nx + 1;
    bool is_land = false;
    if constexpr (LAND)
        is_land = land_node(land, nx, ny, (int)(n % nn), (int)(n / nn));
    double hwn = 0.;
    if constexpr (BASAL)
        hwn = node_mean_of(nx, ny, (int)(n % nn), (int)(n / nn), [&](int ix, int iy) { return depth[(long)iy * nx + ix]; });
    double cgs = 0.;
    if constexpr (SNOW)
        cgs = node_average(nx, ny, ncs, snow, (int)(n % nn), (int)(n / nn));
    double sx = 0., sy = 0.;
    if constexpr (TILT)
        if (!is_land)
            tilt_gradient(nn, 2 * ny + 1, (int)(n % nn), (int)(n / nn), hx, hy, [&](int gx, int gy) { return ssh[(long)gy * nn + gx]; }, sx, sy);
    pack_node<BASAL, SNOW, TILT>(P, dt, u0[n], v0[n], tax[n], tay[n], uo[n], vo[n], cgh[n], cga[n], packed, nodal_plane(nnodes), n, is_land, B, hwn, r, cgs,
        g, sx, sy);
}

// node_average() on a tile of DG coefficients staged in LDS: tile[c][iy - ey0][ix - ex0]; same loops, same order of
// summation, so the result is bit-identical to the global-memory form
constexpr int PREP_TW = 33, PREP_TH = 3; // element columns / rows under a 64 x 4 block of nodes
__device__ __forceinline__ double node_average_tile(int nx, int ny, const double (*tile)[PREP_TH][PREP_TW], int ex0, int ey0, int gx, int gy, int nc = 6)
{
    const int ix_hi = gx / 2, ix_lo = (gx % 2 == 0) ? gx / 2 - 1 : gx / 2;
    const int iy_hi = gy / 2, iy_lo = (gy % 2 == 0) ? gy / 2 - 1 : gy / 2;
    double s = 0.;
    int cnt = 0;
    for (int iy = iy_lo; iy <= iy_hi; ++iy)
        for (int ix = ix_lo; ix <= ix_hi; ++ix) {
            if (ix < 0 || ix >= nx || iy < 0 || iy >= ny)
                continue;
            const double x = -0.5 + 0.5 * (gx - 2 * ix), y = -0.5 + 0.5 * (gy - 2 * iy);
            double val = 0.;
            for (int c = 0; c < nc; ++c)
                val += tile[c][iy - ey0][ix - ex0] * psi_rt(c, x, y);
            s += val;
            ++cnt;
        }
    return s / cnt;
}

// All per-step nodal preparation of the momentum equation in one pass over the CG2 lattice: nodal means of
// H and A (dg_to_cg), wind stress, coefficient packing -- without materialising cgH, cgA, tau_a.  A workgroup
// handles 64 x 4 nodes; the DG coefficients of the 33 x 3 elements under them are staged in LDS once (9.5 KB)
// instead of being gathered by every node lane from memory (a vertex node reads 4 elements x 6 coefficients x 2
// fields: the gather form issued ~57 loads per lane and was bound by vector-memory issue, 0.67 ms at 2048^2).
// LAND: the mask bytes of the same 33 x 3 elements are staged beside the tile and land nodes are packed with the flag.
// BASAL: so are their water depths, and pair 3 of a node is (T_b, 0).
// SNOW: so are the ncs (1, 3 or 6) coefficient planes of the snow, 4.6 KB more for six planes (14.3 KB in all); the nodal mean is read with
// the loops of node_average_tile over ncs coefficients, the order of nsdg_dg_to_cg(ncs).
// TILT: an ocean node reads the sea-surface height at its four lattice neighbours from global memory: the rows above and below are the
// coalesced loads of ua, va, uo, vo over again; staging the 66 x 6 halo in LDS compiled to ~45 instructions and 3.1 KB of LDS more for
// loads the cache already serves (profiles/tilt.md).
template <bool LAND, bool BASAL, bool SNOW, bool TILT>
__global__ __launch_bounds__(256) void mevp_prepare_kernel(nsdg_mevp_params P, int nx, int ny, double dt,
    const double* __restrict__ H, const double* __restrict__ A, const double* __restrict__ ua, const double* __restrict__ va,
    const double* __restrict__ uo, const double* __restrict__ vo, const double* __restrict__ u0, const double* __restrict__ v0,
    double* __restrict__ packed, const uint8_t* __restrict__ land, nsdg_basal_params B, const double* __restrict__ depth,
    const double* __restrict__ snow, int ncs, double r, const double* __restrict__ ssh, double g, double hx, double hy)
{
    __shared__ double tile[2][6][PREP_TH][PREP_TW];
    __shared__ double stile[SNOW ? 6 : 1][PREP_TH][PREP_TW];
    __shared__ uint8_t ltile[LAND ? PREP_TH : 1][PREP_TW];
    __shared__ double dtile[BASAL ? PREP_TH : 1][PREP_TW];
    const int gx0 = blockIdx.x * 64, gy0 = blockIdx.y * 4;
    const int ex0 = gx0 / 2 - 1, ey0 = gy0 / 2 - 1;
    const long N = (long)nx * ny;
    const int tid = threadIdx.y * 64 + threadIdx.x;
    for (int k = tid; k < 2 * 6 * PREP_TH * PREP_TW; k += 256) {
        const int col = k % PREP_TW, r = (k / PREP_TW) % PREP_TH, c = (k / (PREP_TW * PREP_TH)) % 6, fld = k / (PREP_TW * PREP_TH * 6);
        const int ix = ex0 + col, iy = ey0 + r;
        double val = 0.;
        if (ix >= 0 && ix < nx && iy >= 0 && iy < ny)
            val = (fld == 0 ? H : A)[c * N + (long)iy * nx + ix];
        tile[fld][c][r][col] = val;
    }
    if constexpr (LAND) {
        if (tid < PREP_TH * PREP_TW) {
            const int col = tid % PREP_TW, r = tid / PREP_TW;
            const int ix = ex0 + col, iy = ey0 + r;
            ltile[r][col] = (ix >= 0 && ix < nx && iy >= 0 && iy < ny) ? land[(long)iy * nx + ix] : 0;
        }
    }
    if constexpr (BASAL) {
        if (tid < PREP_TH * PREP_TW) {
            const int col = tid % PREP_TW, r = tid / PREP_TW;
            const int ix = ex0 + col, iy = ey0 + r;
            dtile[r][col] = (ix >= 0 && ix < nx && iy >= 0 && iy < ny) ? depth[(long)iy * nx + ix] : 0.;
        }
    }
    if constexpr (SNOW) {
        for (int k = tid; k < ncs * PREP_TH * PREP_TW; k += 256) {
            const int col = k % PREP_TW, rr = (k / PREP_TW) % PREP_TH, c = k / (PREP_TW * PREP_TH);
            const int ix = ex0 + col, iy = ey0 + rr;
            double val = 0.;
            if (ix >= 0 && ix < nx && iy >= 0 && iy < ny)
                val = snow[c * N + (long)iy * nx + ix];
            stile[c][rr][col] = val;
        }
    }
    __syncthreads();
    const int gx = gx0 + threadIdx.x;
    const int gy = gy0 + threadIdx.y;
    const int nn = 2 * nx + 1, nm = 2 * ny + 1;
    if (gx >= nn || gy >= nm)
        return;
    const long n = (long)gy * nn + gx;
    const double cgh = node_average_tile(nx, ny, tile[0], ex0, ey0, gx, gy), cga = node_average_tile(nx, ny, tile[1], ex0, ey0, gx, gy);
    double tax, tay;
    wind_tau(P.c_atm * P.rho_atm, ua[n], va[n], tax, tay);
    bool is_land = false;
    if constexpr (LAND)
        is_land = land_node_of(nx, ny, gx, gy, [&](int ix, int iy) { return ltile[iy - ey0][ix - ex0]; });
    double hwn = 0.;
    if constexpr (BASAL)
        hwn = node_mean_of(nx, ny, gx, gy, [&](int ix, int iy) { return dtile[iy - ey0][ix - ex0]; });
    double cgs = 0.;
    if constexpr (SNOW)
        cgs = node_average_tile(nx, ny, stile, ex0, ey0, gx, gy, ncs);
    double sx = 0., sy = 0.;
    if constexpr (TILT)
        if (!is_land)
            tilt_gradient(nn, nm, gx, gy, hx, hy, [&](int x, int y) { return ssh[(long)y * nn + x]; }, sx, sy);
    pack_node<BASAL, SNOW, TILT>(P, dt, u0[n], v0[n], tax, tay, uo[n], vo[n], cgh, cga, packed, nodal_plane((long)nn * nm), n, is_land, B, hwn, r, cgs, g,
        sx, sy);
}

// one lane per CG2 node
__global__ __launch_bounds__(256) void dg_to_cg_kernel(int nx, int ny, int nc, const double* __restrict__ f, double* __restrict__ g)
{
    const int gx = blockIdx.x * 64 + threadIdx.x;
    const int gy = blockIdx.y * 4 + threadIdx.y;
    const int nn = 2 * nx + 1, nm = 2 * ny + 1;
    if (gx >= nn || gy >= nm)
        return;
    g[(long)gy * nn + gx] = node_average(nx, ny, nc, f, gx, gy);
}

__global__ __launch_bounds__(256) void ice_strength_kernel(int nx, int ny, int j0, int j1, double pstar, double compaction,
    const double* __restrict__ H, const double* __restrict__ A, double* __restrict__ pg)
{
    const int ix = blockIdx.x * 64 + threadIdx.x;
    const int iy = j0 + blockIdx.y * 4 + threadIdx.y;
    if (ix >= nx || iy >= j1)
        return;
    const long N = (long)nx * ny;
    const long e = (long)iy * nx + ix;
    const long tp = tile_off(ix, iy, tiles_per_row(nx), 9);
    double hc[6], ac[6];
    plane_load6(H, N, e, hc);
    plane_load6(A, N, e, ac);
    double pq[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) {
        double h, a;
        gauss_thickness_conc(q, hc, ac, h, a);
        clamp_thickness_conc(h, a);
        pq[q] = pstar * h * exp(-compaction * (1. - a));
    }
    tile_store9(pg, tp, ix & 63, pq);
}

__global__ __launch_bounds__(256) void wind_stress_kernel(long n, double f_atm, const double* __restrict__ ua,
    const double* __restrict__ va, double* __restrict__ tax, double* __restrict__ tay)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n)
        return;
    wind_tau(f_atm, ua[i], va[i], tax[i], tay[i]);
}

} // namespace nsdg_mevp_detail

using namespace nsdg_mevp_detail;

// the adaptive form of alpha, beta (mevp_common.h) exists in the marching kernels only
#define NSDG_NOT_ADAPTIVE(ctx)                                                                                                  \
    do {                                                                                                                        \
        if (nsdg_adaptive(ctx)) {                                                                                               \
            nsdg_set_error("%s: the two-kernel form has no adaptive alpha / beta (nsdg_mevp_params.aevp_c > 0): use nsdg_mevp_iterate*", __func__); \
            return NSDG_ERR_STATE;                                                                                              \
        }                                                                                                                       \
    } while (0)

extern "C" {

int64_t nsdg_tiled_len(int32_t nx, int32_t ny, int32_t nc) { return (int64_t)ny * tiles_per_row(nx) * nc * 64; }

int nsdg_dg_to_cg(nsdg_ctx* ctx, int32_t ncoef, const double* f_dg, double* f_cg)
{
    NSDG_NEED_GRID(ctx);
    NSDG_CHECK_ARG(ncoef == 1 || ncoef == 3 || ncoef == 6, "ncoef must be 1, 3 or 6");
    NSDG_CHECK_ARG(f_dg && f_cg, "null field pointer");
    NSDG_CHECK_HIP(hipSetDevice(ctx->device));
    const dim3 block(64, 4), grid(nsdg_div_up(2 * ctx->nx + 1, 64), nsdg_div_up(2 * ctx->ny + 1, 4));
    hipLaunchKernelGGL(dg_to_cg_kernel, grid, block, 0, ctx->stream, ctx->nx, ctx->ny, ncoef, f_dg, f_cg);
    NSDG_CHECK_LAUNCH();
    return NSDG_OK;
}

int nsdg_ice_strength(nsdg_ctx* ctx, int32_t j0, int32_t j1, const double* H, const double* A, double* pg)
{
    NSDG_NEED_GRID(ctx);
    NSDG_CHECK_ARG(0 <= j0 && j0 <= j1 && j1 <= ctx->ny, "row range outside the local array");
    NSDG_CHECK_ARG(H && A && pg, "null field pointer");
    NSDG_CHECK_TILED(pg);
    if (j0 == j1)
        return NSDG_OK;
    NSDG_CHECK_HIP(hipSetDevice(ctx->device));
    const dim3 block(64, 4), grid(nsdg_div_up(ctx->nx, 64), nsdg_div_up(j1 - j0, 4));
    hipLaunchKernelGGL(ice_strength_kernel, grid, block, 0, ctx->stream, ctx->nx, ctx->ny, j0, j1, ctx->mevp.pstar,
        ctx->mevp.compaction, H, A, pg);
    NSDG_CHECK_LAUNCH();
    return NSDG_OK;
}

int nsdg_wind_stress(nsdg_ctx* ctx, int64_t nnodes, const double* ua, const double* va, double* tax, double* tay)
{
    NSDG_CHECK_ARG(ctx != nullptr, "null context");
    NSDG_CHECK_ARG(nnodes >= 0, "negative node count");
    NSDG_CHECK_ARG(ua && va && tax && tay, "null field pointer");
    if (nnodes == 0)
        return NSDG_OK;
    NSDG_CHECK_HIP(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(wind_stress_kernel, dim3(nsdg_div_up(nnodes, 256)), dim3(256), 0, ctx->stream, (long)nnodes,
        ctx->mevp.c_atm * ctx->mevp.rho_atm, ua, va, tax, tay);
    NSDG_CHECK_LAUNCH();
    return NSDG_OK;
}

static int launch_stress(nsdg_ctx* ctx, int k0, int k1, const double* u, const double* v, const double* pg, const double* s11i,
    const double* s12i, const double* s22i, double* s11, double* s12, double* s22)
{
    const dim3 block(64, 4), grid(nsdg_div_up(ctx->nx, 64), nsdg_div_up(k1 - k0, 4));
    hipLaunchKernelGGL(mevp_stress_kernel, grid, block, 0, ctx->stream, ctx->nx, ctx->ny, k0, k1, 1. / ctx->hx, 1. / ctx->hy,
        1. / ctx->mevp.alpha, ctx->mevp.delta_min * ctx->mevp.delta_min, u, v, pg, s11i, s12i, s22i, s11, s12, s22);
    NSDG_CHECK_LAUNCH();
    return NSDG_OK;
}

int nsdg_mevp_stress(nsdg_ctx* ctx, int32_t k0, int32_t k1, const double* u, const double* v, const double* pg, double* s11,
    double* s12, double* s22)
{
    NSDG_NEED_GRID(ctx);
    NSDG_CHECK_ARG(0 <= k0 && k0 <= k1 && k1 <= ctx->ny, "row range outside the local array");
    NSDG_CHECK_ARG(u && v && pg && s11 && s12 && s22, "null field pointer");
    NSDG_CHECK_TILED(pg, s11, s12, s22);
    NSDG_NOT_ADAPTIVE(ctx);
    if (k0 == k1)
        return NSDG_OK;
    NSDG_CHECK_HIP(hipSetDevice(ctx->device));
    return launch_stress(ctx, k0, k1, u, v, pg, s11, s12, s22, s11, s12, s22);
}

int nsdg_mevp_pack_nodal(nsdg_ctx* ctx, double dt, const double* u0, const double* v0, const double* tax, const double* tay,
    const double* uo, const double* vo, const double* cgh, const double* cga, double* packed)
{
    NSDG_NEED_GRID(ctx);
    NSDG_CHECK_ARG(u0 && v0 && tax && tay && uo && vo && cgh && cga && packed, "null field pointer");
    NSDG_CHECK_ARG(dt > 0, "dt must be positive");
    NSDG_CHECK_ARG(((uintptr_t)packed & 15) == 0, "packed must be 16-byte aligned");
    NSDG_CHECK_HIP(hipSetDevice(ctx->device));
    const long nnodes = (long)(2 * ctx->nx + 1) * (2 * ctx->ny + 1);
    const int snow_rc = nsdg_snow_check_packed(ctx, __func__, packed);
    if (snow_rc)
        return snow_rc;
    const int tilt_rc = nsdg_tilt_check_packed(ctx, __func__, packed);
    if (tilt_rc)
        return tilt_rc;
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(nsdg_div_up(nnodes, 256)), dim3(256), 0, ctx->stream, ctx->mevp, nnodes, dt, u0, v0, tax, tay, uo, vo, cgh, cga,
            packed, ctx->nx, ctx->ny, ctx->land, ctx->basal, ctx->depth, ctx->snow, ctx->snow_ncoef, nsdg_snow_ratio(ctx), ctx->ssh,
            ctx->gravity, ctx->hx, ctx->hy);
    };
    // snow load (snowload.hip), sea-surface tilt (tilt.hip): a context without the field launches the instantiations it always did
    auto choose = [&](auto snow, auto tilt) {
        constexpr bool SNOW = decltype(snow)::value, TILT = decltype(tilt)::value;
        if (ctx->depth)
            ctx->land ? launch(mevp_pack_nodal_kernel<true, true, SNOW, TILT>) : launch(mevp_pack_nodal_kernel<false, true, SNOW, TILT>);
        else
            ctx->land ? launch(mevp_pack_nodal_kernel<true, false, SNOW, TILT>) : launch(mevp_pack_nodal_kernel<false, false, SNOW, TILT>);
    };
    auto choose_tilt = [&](auto snow) { ctx->ssh ? choose(snow, std::true_type()) : choose(snow, std::false_type()); };
    ctx->snow ? choose_tilt(std::true_type()) : choose_tilt(std::false_type());
    NSDG_CHECK_LAUNCH();
    ctx->pack_dt = dt; // the launch constants K1, K2 of the velocity update belong to this packing
    ctx->pack_land = ctx->land != nullptr; // and so does the choice of the passes' instantiation: this packing flagged land nodes, or not,
    ctx->pack_basal = ctx->depth != nullptr; // and stored T_b as the seventh coefficient, or not
    return NSDG_OK;
}

int nsdg_mevp_prepare(nsdg_ctx* ctx, double dt, const double* H, const double* A, const double* ua, const double* va,
    const double* uo, const double* vo, const double* u0, const double* v0, double* packed)
{
    NSDG_NEED_GRID(ctx);
    NSDG_CHECK_ARG(H && A && ua && va && uo && vo && u0 && v0 && packed, "null field pointer");
    NSDG_CHECK_ARG(dt > 0, "dt must be positive");
    NSDG_CHECK_ARG(((uintptr_t)packed & 15) == 0, "packed must be 16-byte aligned");
    NSDG_CHECK_HIP(hipSetDevice(ctx->device));
    const dim3 block(64, 4), grid(nsdg_div_up(2 * ctx->nx + 1, 64), nsdg_div_up(2 * ctx->ny + 1, 4));
    const int snow_rc = nsdg_snow_check_packed(ctx, __func__, packed);
    if (snow_rc)
        return snow_rc;
    const int tilt_rc = nsdg_tilt_check_packed(ctx, __func__, packed);
    if (tilt_rc)
        return tilt_rc;
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, block, 0, ctx->stream, ctx->mevp, ctx->nx, ctx->ny, dt, H, A, ua, va, uo, vo, u0, v0, packed, ctx->land,
            ctx->basal, ctx->depth, ctx->snow, ctx->snow_ncoef, nsdg_snow_ratio(ctx), ctx->ssh,
            ctx->gravity, ctx->hx, ctx->hy);
    };
    auto choose = [&](auto snow, auto tilt) {
        constexpr bool SNOW = decltype(snow)::value, TILT = decltype(tilt)::value;
        if (ctx->depth)
            ctx->land ? launch(mevp_prepare_kernel<true, true, SNOW, TILT>) : launch(mevp_prepare_kernel<false, true, SNOW, TILT>);
        else
            ctx->land ? launch(mevp_prepare_kernel<true, false, SNOW, TILT>) : launch(mevp_prepare_kernel<false, false, SNOW, TILT>);
    };
    auto choose_tilt = [&](auto snow) { ctx->ssh ? choose(snow, std::true_type()) : choose(snow, std::false_type()); };
    ctx->snow ? choose_tilt(std::true_type()) : choose_tilt(std::false_type());
    NSDG_CHECK_LAUNCH();
    ctx->pack_dt = dt;
    ctx->pack_land = ctx->land != nullptr;
    ctx->pack_basal = ctx->depth != nullptr;
    return NSDG_OK;
}

int nsdg_mevp_velocity(nsdg_ctx* ctx, int32_t j0, int32_t j1, const double* s11, const double* s12, const double* s22,
    const double* u_old, const double* v_old, double* u_new, double* v_new, const double* packed)
{
    NSDG_NEED_GRID(ctx);
    NSDG_CHECK_ARG(0 <= j0 && j0 <= j1 && j1 <= ctx->ny, "row range outside the local array");
    NSDG_CHECK_ARG(s11 && s12 && s22 && u_old && v_old && u_new && v_new && packed, "null field pointer");
    NSDG_CHECK_TILED(s11, s12, s22);
    NSDG_CHECK_ARG(u_new != u_old && v_new != v_old, "u_new/v_new must not alias u_old/v_old");
    NSDG_NOT_ADAPTIVE(ctx);
    if (j0 == j1)
        return NSDG_OK;
    NSDG_CHECK_HIP(hipSetDevice(ctx->device));
    const dim3 block(64, 4), grid(nsdg_div_up(ctx->nx, 64), nsdg_div_up(j1 - j0, 4));
    if (!(ctx->pack_dt > 0)) {
        nsdg_set_error("nsdg_mevp_velocity: nsdg_mevp_pack_nodal was not called on this context");
        return NSDG_ERR_STATE;
    }
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, block, 0, ctx->stream, nsdg_nodal_consts_basal(ctx), ctx->nx, ctx->ny, j0, j1, ctx->hx, ctx->hy, s11, s12, s22, u_old, v_old,
            packed, u_new, v_new);
    };
    if (ctx->pack_basal)
        ctx->pack_land ? launch(mevp_velocity_basal_kernel<true>) : launch(mevp_velocity_basal_kernel<false>);
    else
        ctx->pack_land ? launch(mevp_velocity_land_kernel) : launch(mevp_velocity_kernel);
    NSDG_CHECK_LAUNCH();
    return NSDG_OK;
}

} // extern "C"

int nsdg_pass_check(nsdg_ctx* ctx, const char* fn, int v, int k0, int j0, int j1, bool pair, int j0b, int j1b, const nsdg_mevp_bufs& b,
    std::initializer_list<const void*> gauss, bool* run)
{
    static const char* const count[] = { "", "one", "two", "three", "four" };
    static const char* const variants[] = { "", "", "2, 3 or 4 (nsdg_mevp_variant_set) or call nsdg_mevp_iterate twice",
        "3 or 4 (nsdg_mevp_variant_set)", "4 (nsdg_mevp_variant_set)" };
    *run = false;
    NSDG_CHECK_ARG_IN(fn, ctx != nullptr, "null context");
    if (ctx->nx <= 0) {
        nsdg_set_error("%s: nsdg_grid_set was not called", fn);
        return NSDG_ERR_STATE;
    }
    const int ny = ctx->ny;
    if (v == 1) {
        NSDG_CHECK_ARG_IN(fn, 0 <= k0 && k0 <= j0 && j0 <= j1 && j1 <= ny, "need 0 <= k0 <= j0 <= j1 <= ny");
        NSDG_CHECK_ARG_IN(fn, k0 == j0 - 1 || (k0 == 0 && j0 == 0), "need k0 == j0 - 1 (one ghost row below) or k0 == j0 == 0");
    } else {
        // v ghost rows below, v - 1 above (for v = 2 that always holds); a range of a pair must not be empty
        const char* rows = pair ? "rows of a range" : "owned rows";
        for (int k = 0; k < (pair ? 2 : 1); ++k) {
            const int r0 = k ? j0b : j0, r1 = k ? j1b : j1;
            NSDG_CHECK_ARG_IN(fn, 0 <= r0 && (pair ? r0 < r1 : r0 <= r1) && r1 <= ny, "row range outside the local array%s", pair ? " (or empty)" : "");
            NSDG_CHECK_ARG_IN(fn, r0 == 0 || r0 >= v, "need %s ghost rows below the %s (or j0 == 0 at the physical boundary)", count[v], rows);
            NSDG_CHECK_ARG_IN(fn, r1 == ny || r1 + v - 1 <= ny, "need %s ghost rows above the %s (or j1 == ny at the physical boundary)", count[v - 1], rows);
        }
        NSDG_CHECK_ARG_IN(fn, !pair || j1 <= j0b || j1b <= j0, "the two row ranges must be disjoint");
    }
    NSDG_CHECK_ARG_IN(fn, b.s11i && b.s12i && b.s22i && b.s11 && b.s12 && b.s22 && b.u_old && b.v_old && b.u_new && b.v_new && b.packed
            && std::find(gauss.begin(), gauss.end(), nullptr) == gauss.end(),
        "null field pointer");
    NSDG_CHECK_ARG_IN(fn, nsdg_aligned16({ b.s11i, b.s12i, b.s22i, b.s11, b.s12, b.s22 }) && nsdg_aligned16(gauss), NSDG_TILED_MSG);
    NSDG_CHECK_ARG_IN(fn, b.u_new != b.u_old && b.v_new != b.v_old, "u_new/v_new must not alias u_old/v_old");
    NSDG_CHECK_ARG_IN(fn, b.s11 != b.s11i && b.s12 != b.s12i && b.s22 != b.s22i, "the output stress must not alias the input stress");
    // nothing to do: v = 1 without a stress row, checked before the packing (j0 == j1 > k0 still updates the stress row k0); v >= 2
    // on an empty range, checked after the packing and before the variant
    if (v == 1 && k0 == j1)
        return NSDG_OK;
    if (!(ctx->pack_dt > 0)) {
        nsdg_set_error("%s: nsdg_mevp_pack_nodal was not called on this context", fn);
        return NSDG_ERR_STATE;
    }
    if (v >= 2 && j0 == j1)
        return NSDG_OK;
    if (v >= 2 && ctx->mevp_variant < v) {
        nsdg_set_error("%s: select variant %s", fn, variants[v]);
        return NSDG_ERR_STATE;
    }
    const hipError_t e = hipSetDevice(ctx->device);
    if (e != hipSuccess) {
        nsdg_set_error("%s: hipSetDevice(ctx->device) failed: %s", fn, hipGetErrorString(e));
        return NSDG_ERR_HIP;
    }
    *run = true;
    return NSDG_OK;
}

int nsdg_mevp_pass(nsdg_ctx* ctx, int v, int k0, int j0, int j1, bool pair, int j0b, int j1b, const nsdg_mevp_bufs& b)
{
    static const char* const names[2][5] = { { "", "nsdg_mevp_iterate", "nsdg_mevp_iterate2", "nsdg_mevp_iterate3", "nsdg_mevp_iterate4" },
        { "", "", "", "nsdg_mevp_iterate3_pair", "nsdg_mevp_iterate4_pair" } };
    bool run;
    const int checked = nsdg_pass_check(ctx, names[pair][v], v, k0, j0, j1, pair, j0b, j1b, b, { b.pg }, &run);
    if (!run)
        return checked;
    // masked or not: the instantiation goes with the packing the pass reads (nsdg_mevp_pack_nodal / nsdg_mevp_prepare remembered whether
    // they flagged land nodes, and whether they stored T_b from a depth array); the two-kernel form's velocity kernel (nsdg_mevp_velocity)
    // reads the same flags
    const bool land = ctx->pack_land, basal = ctx->pack_basal;
    if (v >= 2) // a pass of the stage-per-wave pipeline with v stages
        return nsdg_launch_mevp_fused4_ranges(ctx, land, basal, v, j0, j1, j0b, j1b, b);
    if (ctx->mevp_variant >= 1 || nsdg_adaptive(ctx)) // variants 2-4 use the single-iteration fused kernel for one sub-iteration; so does variant 0 in the adaptive form
        return nsdg_launch_mevp_fused(ctx, land, basal, k0, j0, j1, b);
    const int rc = launch_stress(ctx, k0, j1, b.u_old, b.v_old, b.pg, b.s11i, b.s12i, b.s22i, b.s11, b.s12, b.s22);
    return rc ? rc : nsdg_mevp_velocity(ctx, j0, j1, b.s11, b.s12, b.s22, b.u_old, b.v_old, b.u_new, b.v_new, b.packed);
}

extern "C" {

int nsdg_mevp_iterate(nsdg_ctx* ctx, int32_t k0, int32_t j0, int32_t j1, const double* s11i, const double* s12i,
    const double* s22i, double* s11, double* s12, double* s22, const double* u_old, const double* v_old, double* u_new,
    double* v_new, const double* packed, const double* pg)
{
    return nsdg_mevp_pass(ctx, 1, k0, j0, j1, false, 0, 0, { s11i, s12i, s22i, s11, s12, s22, u_old, v_old, u_new, v_new, packed, pg });
}

int nsdg_mevp_iterate2(nsdg_ctx* ctx, int32_t j0, int32_t j1, const double* s11i, const double* s12i, const double* s22i,
    double* s11, double* s12, double* s22, const double* u_old, const double* v_old, double* u_new, double* v_new,
    const double* packed, const double* pg)
{
    return nsdg_mevp_pass(ctx, 2, 0, j0, j1, false, 0, 0, { s11i, s12i, s22i, s11, s12, s22, u_old, v_old, u_new, v_new, packed, pg });
}

int nsdg_mevp_iterate3(nsdg_ctx* ctx, int32_t j0, int32_t j1, const double* s11i, const double* s12i, const double* s22i,
    double* s11, double* s12, double* s22, const double* u_old, const double* v_old, double* u_new, double* v_new,
    const double* packed, const double* pg)
{
    return nsdg_mevp_pass(ctx, 3, 0, j0, j1, false, 0, 0, { s11i, s12i, s22i, s11, s12, s22, u_old, v_old, u_new, v_new, packed, pg });
}

int nsdg_mevp_iterate3_pair(nsdg_ctx* ctx, int32_t j0a, int32_t j1a, int32_t j0b, int32_t j1b, const double* s11i, const double* s12i,
    const double* s22i, double* s11, double* s12, double* s22, const double* u_old, const double* v_old, double* u_new, double* v_new,
    const double* packed, const double* pg)
{
    return nsdg_mevp_pass(ctx, 3, 0, j0a, j1a, true, j0b, j1b, { s11i, s12i, s22i, s11, s12, s22, u_old, v_old, u_new, v_new, packed, pg });
}

int nsdg_mevp_iterate4(nsdg_ctx* ctx, int32_t j0, int32_t j1, const double* s11i, const double* s12i, const double* s22i,
    double* s11, double* s12, double* s22, const double* u_old, const double* v_old, double* u_new, double* v_new,
    const double* packed, const double* pg)
{
    return nsdg_mevp_pass(ctx, 4, 0, j0, j1, false, 0, 0, { s11i, s12i, s22i, s11, s12, s22, u_old, v_old, u_new, v_new, packed, pg });
}

int nsdg_mevp_iterate4_pair(nsdg_ctx* ctx, int32_t j0a, int32_t j1a, int32_t j0b, int32_t j1b, const double* s11i, const double* s12i,
    const double* s22i, double* s11, double* s12, double* s22, const double* u_old, const double* v_old, double* u_new, double* v_new,
    const double* packed, const double* pg)
{
    return nsdg_mevp_pass(ctx, 4, 0, j0a, j1a, true, j0b, j1b, { s11i, s12i, s22i, s11, s12, s22, u_old, v_old, u_new, v_new, packed, pg });
}

int nsdg_mevp_subcycle(nsdg_ctx* ctx, double dt, int32_t nsub, double* s11, double* s12, double* s22, double* u, double* v,
    const double* u0, const double* v0, const double* tax, const double* tay, const double* uo, const double* vo,
    const double* cgh, const double* cga, const double* pg, double* scratch)
{
    NSDG_NEED_GRID(ctx);
    NSDG_CHECK_ARG(nsub >= 0, "negative sub-iteration count");
    NSDG_CHECK_ARG(u && v && s11 && s12 && s22 && scratch, "null field pointer");
    // u0/v0 may alias u/v: they are consumed by the coefficient packing before the first pass writes u, v
    NSDG_CHECK_ARG(u0 && v0, "null field pointer");
    NSDG_CHECK_ARG(((uintptr_t)scratch & 15) == 0, "scratch must be 16-byte aligned");
    const long nnodes = (long)(2 * ctx->nx + 1) * (2 * ctx->ny + 1);
    const long M = nsdg_tiled_len(ctx->nx, ctx->ny, 8);
    // scratch: [packed nodal 8*nnodes (6*nnodes used without a depth array)][u, v ping-pong 2*nnodes][stress ping-pong 3*M]
    double* packed = scratch;
    double *ua = u, *va = v, *ub = scratch + 8 * nnodes, *vb = ub + nnodes;
    double *sa[3] = { s11, s12, s22 };
    double *sb[3] = { vb + nnodes, vb + nnodes + M, vb + nnodes + 2 * M };
    int rc = nsdg_p2p_check(ctx, __func__); // a pipeline wait that gave up in an earlier launch: the fields this call would start from are wrong
    if (rc)
        return rc;
    rc = nsdg_mevp_pack_nodal(ctx, dt, u0, v0, tax, tay, uo, vo, cgh, cga, packed);
    if (rc)
        return rc;
    for (int it = 0; it < nsub;) {
        const int n = std::max(1, std::min(ctx->mevp_variant, nsub - it)); // sub-iterations of this pass: as many as the variant allows
        rc = nsdg_mevp_pass(ctx, n, 0, 0, ctx->ny, false, 0, 0, { sa[0], sa[1], sa[2], sb[0], sb[1], sb[2], ua, va, ub, vb, packed, pg });
        if (rc)
            return rc;
        it += n;
        double* t = ua; ua = ub; ub = t;
        t = va; va = vb; vb = t;
        for (int k = 0; k < 3; ++k) { t = sa[k]; sa[k] = sb[k]; sb[k] = t; }
    }
    if (ua != u) { // odd number of sub-iterations: the results sit in scratch
        NSDG_CHECK_HIP(hipMemcpyAsync(u, ua, nnodes * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
        NSDG_CHECK_HIP(hipMemcpyAsync(v, va, nnodes * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
        NSDG_CHECK_HIP(hipMemcpyAsync(s11, sa[0], M * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
        NSDG_CHECK_HIP(hipMemcpyAsync(s12, sa[1], M * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
        NSDG_CHECK_HIP(hipMemcpyAsync(s22, sa[2], M * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    }
    return NSDG_OK;
}

} // extern "C"
