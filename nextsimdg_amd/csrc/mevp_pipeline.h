// mevp_pipeline.h -- the march that the marching mEVP kernels share: the single-iteration kernel (mevp_fused.hip: one wave, one
// sub-iteration) and the stage-per-wave pipeline (mevp_fused4.hip: one sub-iteration per wave of a workgroup).  A wave marches through
// its strip bottom to top, one element per lane per row.  Here are the per-lane constants of a march, the stress pointers of a pass,
// the contributions a row carries to the row above it, the packed coefficients and the update of the four nodes an element owns
// (vertex, bottom edge-mid, left edge-mid, centre), the gather of an element's nine nodal velocities from owned nodes, and the store of
// the owned nodes with the boundary zeros -- which the two-kernel form (mevp.hip) shares.  The same inlined functions in every kernel
// keep the marching kernels bit-identical to each other.
#pragma once
#include "mevp_common.h"

namespace nsdg_mevp_detail {

struct MarchConst {
    NodalConsts K;
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

// the four owned nodes of one element row from the carried contributions of the row below (`carry`), the
// contributions of this row (cx, cy) and the left neighbour's right-column contributions, summed in the oracle's order: below-left,
// below, left, own.  Inverse lumped masses: 4, 2, 2, 1 adjacent elements times 1/36, 1/9, 1/9, 4/9 of the cell area.
// (AD: adaptive form -- `q` is this element's offer q_e = alpha_e h'_c of this sub-iteration, a node takes the largest offer of its adjacent elements)
// (LAND: land nodes stay at 0, node_update)
template <bool AD, bool LAND>
__device__ __forceinline__ void owned_node_updates(const MarchConst& M, bool hasB, const double (&c)[4][6], const double (&uu)[4],
    const double (&vv)[4], const TopCarry& carry, const double (&cx)[9], const double (&cy)[9], double (&un)[4], double (&vn)[4], double q = 0.)
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
        node_update<AD, LAND>(M.K, c[0], uu[0], vv[0], ((carry.xl8 + carry.x6) + l2x) + cx[0], ((carry.yl8 + carry.y6) + l2y) + cy[0], 9. * M.iarea,
            un[0], vn[0], AD ? __builtin_fmax(__builtin_fmax(carry.ql, carry.q), qmid) : 0., amin);
    else
        un[0] = vn[0] = 0.;
    if (hasB)
        node_update<AD, LAND>(M.K, c[1], uu[1], vv[1], carry.x7 + cx[1], carry.y7 + cy[1], 4.5 * M.iarea, un[1], vn[1], qbot, amin);
    else
        un[1] = vn[1] = 0.;
    if (M.hasL)
        node_update<AD, LAND>(M.K, c[2], uu[2], vv[2], l5x + cx[3], l5y + cy[3], 4.5 * M.iarea, un[2], vn[2], qmid, amin);
    else
        un[2] = vn[2] = 0.;
    node_update<AD, LAND>(M.K, c[3], uu[3], vv[3], cx[4], cy[4], 2.25 * M.iarea, un[3], vn[3], q, amin);
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

} // namespace nsdg_mevp_detail
