// mevp_pipeline.h -- the march that the marching kernels share: the single-iteration mEVP kernel (mevp_fused.hip) and its brittle sibling
// (bbm.hip) -- one wave, one sub-iteration -- and the stage-per-wave pipeline (mevp_fused4.hip: one sub-iteration per wave of a
// workgroup).  A wave marches through its strip bottom to top, one element per lane per row.  Who owns what:
//   here             the per-lane constants of a march and the ONE function that fills them (march_frame), the stress pointers of a pass,
//                    the contributions a row carries to the row above it, the packed coefficients and the update of the four nodes an
//                    element owns (vertex, bottom edge-mid, left edge-mid, centre), the gather of an element's nine nodal velocities from
//                    owned nodes, the store of the owned nodes with the boundary zeros -- which the two-kernel form (mevp.hip) shares --
//                    and the row loop of a single-iteration march (march_strip): prologue row, velocity gather, contributions, node
//                    update, store, carry;
//   mevp_fused.hip   the mEVP element step inside march_strip, with its load orders per register budget, and the strip height of a
//                    single-iteration march (nsdg_march_strip_rows);
//   bbm.hip          the brittle element step inside march_strip;
//   mevp_fused4.hip  its own march (p2p_row: inputs from LDS, one stage per wave) on the same frame and the same node functions.
// The same inlined functions in every kernel keep the marching kernels bit-identical to each other.
#pragma once
#include "mevp_common.h"

namespace nsdg_mevp_detail {

struct MarchConst {
    NodalConsts K;
    double u0; // BASAL instantiations only: the speed u0 of the seabed stress (NodalConstsBasal)
    int nx, ny, y0, y1, ix, ntx, nn, lane;
    long nplane; // doubles between two pair planes of the packed nodal coefficients
    bool own, hasL, lastcol;
    double hx, hy, ihx, ihy, iarea, ialpha, dmin2;
    AdaptConsts AC; // adaptive alpha, beta only
};

// the stress of a pass: read from i??, written to o?? (out of place: a recomputing strip must never read what its owner has overwritten)
struct StressPtrs {
    const double *i11, *i12, *i22;
    double *o11, *o12, *o22;
};

// contributions of a row to its top nodes, carried to the next row of the march
struct TopCarry {
    double x6 = 0., y6 = 0., x7 = 0., y7 = 0., xl8 = 0., yl8 = 0.; // 6: top-left, 7: top-mid of my column, 8 of the left column
    double q = 0., ql = 0.; // adaptive form only: the offers q_e = alpha_e h'_c of the element below and of the element below-left
};

// all three pairs of the packed coefficients of the 4 owned nodes of element row `row`
__device__ __forceinline__ void load_owned_nodal(const MarchConst& M, int row, double (&c)[4][6], const double* __restrict__ packed)
{
    const long nV = (long)(2 * row) * M.nn + 2 * M.ix;
    load_nodal(packed, M.nplane, nV, c[0]);
    load_nodal(packed, M.nplane, nV + 1, c[1]);
    load_nodal(packed, M.nplane, nV + M.nn, c[2]);
    load_nodal(packed, M.nplane, nV + M.nn + 1, c[3]);
}

// BASAL: the fourth pair's first member, T_b, of the same four nodes
__device__ __forceinline__ void load_owned_nodal_tb(const MarchConst& M, int row, double (&tb)[4], const double* __restrict__ packed)
{
    const long nV = (long)(2 * row) * M.nn + 2 * M.ix;
    tb[0] = load_nodal_tb(packed, M.nplane, nV);
    tb[1] = load_nodal_tb(packed, M.nplane, nV + 1);
    tb[2] = load_nodal_tb(packed, M.nplane, nV + M.nn);
    tb[3] = load_nodal_tb(packed, M.nplane, nV + M.nn + 1);
}

// the four owned nodes of one element row from the carried contributions of the row below (`carry`), the
// contributions of this row (cx, cy) and the left neighbour's right-column contributions, summed in the oracle's order: below-left,
// below, left, own.  Inverse lumped masses: 4, 2, 2, 1 adjacent elements times 1/36, 1/9, 1/9, 4/9 of the cell area.
// (AD: adaptive form -- `q` is this element's offer q_e = alpha_e h'_c of this sub-iteration, a node takes the largest offer of its adjacent elements)
// (LAND: land nodes stay at 0, node_update; BASAL: tb = T_b of the four nodes, the seabed stress of node_update -- read only then)
template <bool AD, bool LAND, bool BASAL = false>
__device__ __forceinline__ void owned_node_updates(const MarchConst& M, bool hasB, const double (&c)[4][6], const double (&uu)[4],
    const double (&vv)[4], const TopCarry& carry, const double (&cx)[9], const double (&cy)[9], double (&un)[4], double (&vn)[4], double q,
    const double (&tb)[4])
{
    const double l2x = lane_from_left(cx[2]), l2y = lane_from_left(cy[2]);
    const double l5x = lane_from_left(cx[5]), l5y = lane_from_left(cy[5]);
    double qbot = 0., qmid = 0.; // the largest offer at the bottom edge-mid and at the left edge-mid; the vertex takes both and the carried ones
    if constexpr (AD) {
        const double ql = lane_from_left(q); // the left neighbour's (0 without one: it never wins the max)
        qmid = __builtin_fmax(ql, q), qbot = __builtin_fmax(carry.q, q);
    }
    const double amin = M.AC.amin;
    if (M.hasL && hasB)
        node_update<AD, LAND, BASAL>(M.K, c[0], uu[0], vv[0], ((carry.xl8 + carry.x6) + l2x) + cx[0], ((carry.yl8 + carry.y6) + l2y) + cy[0], 9. * M.iarea,
            un[0], vn[0], AD ? __builtin_fmax(__builtin_fmax(carry.ql, carry.q), qmid) : 0., amin, BASAL ? tb[0] : 0., BASAL ? M.u0 : 0.);
    else
        un[0] = vn[0] = 0.;
    if (hasB)
        node_update<AD, LAND, BASAL>(M.K, c[1], uu[1], vv[1], carry.x7 + cx[1], carry.y7 + cy[1], 4.5 * M.iarea, un[1], vn[1], qbot, amin, BASAL ? tb[1] : 0., BASAL ? M.u0 : 0.);
    else
        un[1] = vn[1] = 0.;
    if (M.hasL)
        node_update<AD, LAND, BASAL>(M.K, c[2], uu[2], vv[2], l5x + cx[3], l5y + cy[3], 4.5 * M.iarea, un[2], vn[2], qmid, amin, BASAL ? tb[2] : 0., BASAL ? M.u0 : 0.);
    else
        un[2] = vn[2] = 0.;
    node_update<AD, LAND, BASAL>(M.K, c[3], uu[3], vv[3], cx[4], cy[4], 2.25 * M.iarea, un[3], vn[3], q, amin, BASAL ? tb[3] : 0., BASAL ? M.u0 : 0.);
}

template <bool AD>
__device__ __forceinline__ void carry_top(TopCarry& carry, const double (&cx)[9], const double (&cy)[9], double q = 0.)
{
    carry.x6 = cx[6], carry.y6 = cy[6], carry.x7 = cx[7], carry.y7 = cy[7];
    carry.xl8 = lane_from_left(cx[8]), carry.yl8 = lane_from_left(cy[8]);
    if constexpr (AD)
        carry.q = q, carry.ql = lane_from_left(q);
}

// u at the 9 nodes of an element from the 4 owned nodes of its row (lo), the two bottom nodes of the row
// above (hi0 = V, hi1 = EX) and the right neighbour lane (node column 2*nx is the right boundary)
__device__ __forceinline__ void gather_nodes(const MarchConst& M, const double (&lo)[4], double hi0, double hi1, double (&w)[9])
{
    w[0] = lo[0], w[1] = lo[1], w[3] = lo[2], w[4] = lo[3], w[6] = hi0, w[7] = hi1;
    const double r2 = lane_from_right(lo[0]), r5 = lane_from_right(lo[2]), r8 = lane_from_right(hi0);
    w[2] = M.lastcol ? 0. : r2;
    w[5] = M.lastcol ? 0. : r5;
    w[8] = M.lastcol ? 0. : r8;
}

// u, v of the four owned nodes of an element (vertex node nV, nn nodes per node row) to memory, and the zeros of the boundary nodes nobody
// owns: the right column of the last element column, the top row of the last element row, their corner
__device__ __forceinline__ void store_owned_nodes(long nV, int nn, bool lastcol, bool toprow, const double (&un)[4], const double (&vn)[4],
    double* __restrict__ u_new, double* __restrict__ v_new)
{
    u_new[nV] = un[0], v_new[nV] = vn[0];
    u_new[nV + 1] = un[1], v_new[nV + 1] = vn[1];
    u_new[nV + nn] = un[2], v_new[nV + nn] = vn[2];
    u_new[nV + nn + 1] = un[3], v_new[nV + nn + 1] = vn[3];
    if (lastcol) {
        u_new[nV + 2] = 0., v_new[nV + 2] = 0.;
        u_new[nV + nn + 2] = 0., v_new[nV + nn + 2] = 0.;
    }
    if (toprow) {
        u_new[nV + 2 * nn] = 0., v_new[nV + 2 * nn] = 0.;
        u_new[nV + 2 * nn + 1] = 0., v_new[nV + 2 * nn + 1] = 0.;
        if (lastcol)
            u_new[nV + 2 * nn + 2] = 0., v_new[nV + 2 * nn + 2] = 0.;
    }
}

// Everything of a march's per-lane constants but the strip's rows y0, y1, for column-wave `cw` of waves that own OWNED columns from lane
// LEFT on: lane l works on column cw * OWNED - LEFT + l.  The lanes left and right of the owned ones recompute their neighbours'
// columns; lanes outside the array load a clamped column and store nothing.
template <int OWNED, int LEFT>
__device__ __forceinline__ void march_frame(MarchConst& M, const NodalConsts& K, const AdaptConsts& AC, int nx, int ny, int lane, int cw,
    double hx, double hy, double ialpha, double dmin2, double u0 = 0.)
{
    M.u0 = u0;
    const int ixr = cw * OWNED - LEFT + lane;
    const bool valid = ixr >= 0 && ixr < nx;
    M.K = K, M.AC = AC;
    M.nx = nx, M.ny = ny, M.lane = lane;
    M.own = valid && lane >= LEFT && lane < LEFT + OWNED;
    M.ix = min(max(ixr, 0), nx - 1);
    M.hasL = M.ix > 0, M.lastcol = M.ix == nx - 1;
    M.ntx = tiles_per_row(nx);
    M.nn = 2 * nx + 1;
    M.nplane = nodal_plane((long)M.nn * (2 * ny + 1));
    M.hx = hx, M.hy = hy, M.ihx = 1. / hx, M.ihy = 1. / hy, M.iarea = M.ihx * M.ihy;
    M.ialpha = ialpha, M.dmin2 = dmin2;
}

// The row loop of a single-iteration march over the strip [M.y0, M.y1) of a launch whose stress rows start at k0 and whose velocity rows
// start at j0: a strip above the first recomputes the row below it as a prologue (nothing of it is stored), every row gathers its nine
// nodal velocities from memory, takes the stress that enters the momentum equation from the rheology, updates and stores its four owned
// nodes and carries its top-row contributions to the next row.
// element(iy, store, nV, ul, vl, m11, m12, m22, qe), an inlined callable, is the rheology's element step of row iy: it loads what it
// needs, updates its state and stores it where `store` is true, and returns the coefficients of the stress of the momentum equation in
// m?? and, in the adaptive form, the element's offer in qe.
// FENCE: a compiler fence between the contributions and the nodal-coefficient loads (the 2-waves-per-SIMD build of mevp_fused.hip)
// BASAL: the fourth coefficient pair is loaded beside the three and the node updates add the seabed stress (node_update)
template <bool AD, bool LAND, bool FENCE, bool BASAL, class Element>
__device__ __forceinline__ void march_strip(const MarchConst& M, int k0, int j0, const double* __restrict__ u_old, const double* __restrict__ v_old,
    const double* __restrict__ packed, double* __restrict__ u_new, double* __restrict__ v_new, Element&& element)
{
    const int ix = M.ix, nn = M.nn;
    TopCarry carry; // zero by its member initialisers: the first row of the march adds nothing from a row below

    for (int iy = (M.y0 > k0 ? M.y0 - 1 : M.y0); iy < M.y1; ++iy) {
        const bool prologue = iy < M.y0; // recomputed row owned by the strip below: nothing is stored
        const long nV = (long)(2 * iy) * nn + 2 * ix;
        double ul[9], vl[9], m11[8], m12[8], m22[8];
#pragma unroll
        for (int a = 0; a < 9; ++a) {
            const long n = nV + (a / 3) * nn + a % 3;
            ul[a] = u_old[n];
            vl[a] = v_old[n];
        }
        double qe = 0.; // adaptive form: this element's offer q_e = alpha_e h'_c of this sub-iteration (mevp_common.h)
        element(iy, !prologue && M.own, nV, ul, vl, m11, m12, m22, qe);
        double cx[9], cy[9];
        node_contrib_all(m11, m12, m22, M.hx, M.hy, cx, cy);
        if constexpr (FENCE)
            asm volatile("" ::: "memory"); // keep the nodal-coefficient loads below this point

        if (!prologue && iy >= j0) { // wave-uniform
            double c[4][6], un[4], vn[4], tb[4] = { 0., 0., 0., 0. };
            load_owned_nodal(M, iy, c, packed);
            if constexpr (BASAL)
                load_owned_nodal_tb(M, iy, tb, packed);
            const double uu[4] = { ul[0], ul[1], ul[3], ul[4] }, vv[4] = { vl[0], vl[1], vl[3], vl[4] };
            owned_node_updates<AD, LAND, BASAL>(M, iy > 0, c, uu, vv, carry, cx, cy, un, vn, qe, tb);
            if (M.own)
                store_owned_nodes(nV, nn, M.lastcol, iy == M.ny - 1, un, vn, u_new, v_new);
        }
        carry_top<AD>(carry, cx, cy, qe); // the top-row contributions go to the next row of the march
    }
}

} // namespace nsdg_mevp_detail
