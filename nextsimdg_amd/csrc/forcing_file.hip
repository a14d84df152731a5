// forcing_file.hip -- forcing records read from a file, sampled ON THE DEVICE at the model time of each step:
// bilinear interpolation in space from a coarse cell-centred lattice over the model's square domain onto the CG2
// nodes or the element centres of a rank's local array, then linear interpolation in time between two records.
//
// The sampling rule (include/nsdg.h, "forcing from a file") is stated in integers so that a numpy restatement
// (tests/forcing_file_ref.py) and every row block reproduce it: the index-space coordinate of a target point is
// num / den with num, den exact integers, divided once; a coincident lattice gives a fraction of exactly 0.
//
// One thread per target point for all fields of its lattice, one launch per lattice per step.  The kernel is
// write-bound (8 B stored per point and field); the coarse records are small and are read through L1/L2.
#include "nsdg_internal.h"

namespace {

struct SamplePtrs {
    const double* r0[NSDG_FORCING_MAX_FIELDS];
    const double* r1[NSDG_FORCING_MAX_FIELDS];
    double* out[NSDG_FORCING_MAX_FIELDS];
};

// index and fraction of one axis: num / den clamped to [0, n - 1]; i1 == i0 where the weight is 0
__device__ inline void axis(long num, long den, int n, int& i0, int& i1, double& f)
{
    if (num <= 0) {
        i0 = i1 = 0, f = 0.;
    } else if (num >= (long)(n - 1) * den) {
        i0 = i1 = n - 1, f = 0.;
    } else {
        const long q = num / den;
        i0 = (int)q, i1 = (int)q + 1;
        f = (double)(num - q * den) / (double)den;
    }
}

__device__ inline double lerp(double a, double b, double f) { return a + f * (b - a); }

__device__ inline double bilinear(const double* __restrict__ r, long o00, long o01, long o10, long o11, double fx, double fy)
{
    return lerp(lerp(r[o00], r[o01], fx), lerp(r[o10], r[o11], fx), fy);
}

// at_nodes: target = CG2 node (gx, gy) of the local array, nn x nm = (2 nx + 1) x (2 ny + 1); else element (ix, iy), nx x ny.
// row0 / ny_glob: placement of local element row 0 in the global domain (nsdg_block_set).
__global__ __launch_bounds__(256) void forcing_sample_kernel(int at_nodes, int nx, int ny, int row0, int ny_glob, int nxr, int nyr,
    int nfields, SamplePtrs p, double w)
{
    const int tx = blockIdx.x * 64 + threadIdx.x;
    const int ty = blockIdx.y * 4 + threadIdx.y;
    const int wx = at_nodes ? 2 * nx + 1 : nx, wy = at_nodes ? 2 * ny + 1 : ny;
    if (tx >= wx || ty >= wy)
        return;
    // index-space coordinates (num / den) on the lattice: nodes x = gx L / (2 nx), elements x = (ix + 1/2) L / nx; point i of the
    // lattice at (i + 1/2) L / nxr
    const long denx = 2L * nx, deny = 2L * ny_glob;
    const long numx = at_nodes ? (long)tx * nxr - nx : (2L * tx + 1) * nxr - nx;
    const long numy = at_nodes ? (long)(ty + 2 * row0) * nyr - ny_glob : (2L * (ty + row0) + 1) * nyr - ny_glob;
    int i0, i1, j0, j1;
    double fx, fy;
    axis(numx, denx, nxr, i0, i1, fx);
    axis(numy, deny, nyr, j0, j1, fy);
    const long o00 = (long)j0 * nxr + i0, o01 = (long)j0 * nxr + i1, o10 = (long)j1 * nxr + i0, o11 = (long)j1 * nxr + i1;
    const long t = (long)ty * wx + tx;
    for (int k = 0; k < nfields; ++k) {
        const double v0 = bilinear(p.r0[k], o00, o01, o10, o11, fx, fy);
        const double v1 = bilinear(p.r1[k], o00, o01, o10, o11, fx, fy);
        p.out[k][t] = lerp(v0, v1, w);
    }
}

} // namespace

extern "C" {

int nsdg_forcing_sample(nsdg_ctx* ctx, int32_t where, int32_t nxr, int32_t nyr, int32_t nfields, const double* const* rec0,
    const double* const* rec1, double w, double* const* out)
{
    NSDG_NEED_GRID(ctx);
    NSDG_CHECK_ARG(where == NSDG_AT_NODES || where == NSDG_AT_ELEMENTS, "where must be NSDG_AT_NODES or NSDG_AT_ELEMENTS");
    NSDG_CHECK_ARG(nxr >= 1 && nyr >= 1, "the forcing lattice needs nxr >= 1 and nyr >= 1");
    NSDG_CHECK_ARG(nxr <= NSDG_FORCING_MAX_LATTICE && nyr <= NSDG_FORCING_MAX_LATTICE, "the forcing lattice is larger than NSDG_FORCING_MAX_LATTICE");
    NSDG_CHECK_ARG(nfields >= 1 && nfields <= NSDG_FORCING_MAX_FIELDS, "nfields must be in [1, NSDG_FORCING_MAX_FIELDS]");
    NSDG_CHECK_ARG(w >= 0. && w <= 1., "the time weight w must be finite and in [0, 1]");
    NSDG_CHECK_ARG(rec0 && rec1 && out, "null pointer array");
    SamplePtrs p;
    for (int k = 0; k < NSDG_FORCING_MAX_FIELDS; ++k) {
        p.r0[k] = p.r1[k] = nullptr, p.out[k] = nullptr;
        if (k < nfields) {
            NSDG_CHECK_ARG(rec0[k] && rec1[k] && out[k], "null field pointer");
            p.r0[k] = rec0[k], p.r1[k] = rec1[k], p.out[k] = out[k];
        }
    }
    const int row0 = ctx->row0, ny_glob = ctx->ny_global > 0 ? ctx->ny_global : ctx->ny;
    NSDG_CHECK_ARG(row0 + ctx->ny <= ny_glob, "nsdg_block_set: the local array does not fit into the global row count");
    NSDG_CHECK_HIP(hipSetDevice(ctx->device));
    const int nodes = where == NSDG_AT_NODES;
    const int wx = nodes ? 2 * ctx->nx + 1 : ctx->nx, wy = nodes ? 2 * ctx->ny + 1 : ctx->ny;
    const dim3 block(64, 4), grid(nsdg_div_up(wx, 64), nsdg_div_up(wy, 4));
    hipLaunchKernelGGL(forcing_sample_kernel, grid, block, 0, ctx->stream, nodes, ctx->nx, ctx->ny, row0, ny_glob, (int)nxr, (int)nyr,
        (int)nfields, p, w);
    NSDG_CHECK_LAUNCH();
    return NSDG_OK;
}

} // extern "C"
