#include "DynamicsBlock.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>

#include "BathymetryFile.hpp"
#include "LandMaskFile.hpp"

namespace Nextsim {

namespace {
bool g_multiProcess = false; // one row block per process, ghost rows over RCCL

// The stress lives on the device in the tiled layout of include/nsdg.h (tiles of 64 elements of a row, the 8 coefficients of a tile
// together, in pairs interleaved by element); a restart file holds coefficient planes [8][rows][nx].
inline std::size_t tiledIndex(int nx, int ix, int iy, int c)
{
    const std::size_t ntx = (std::size_t)(nx + 63) / 64;
    return (((std::size_t)iy * ntx + (std::size_t)(ix >> 6)) * 8) * 64 + (std::size_t)(c / 2) * 128 + 2 * (std::size_t)(ix & 63) + (std::size_t)(c % 2);
}
// rows [row0, row0 + rows) of the tiled array `t` (local array of nx columns) -> planes[c * planeStride + (dstRow0 + r) * nx + ix]
void untileRows(const std::vector<double>& t, int nx, int row0, int rows, double* planes, std::size_t planeStride, std::size_t dstRow0)
{
    for (int c = 0; c < 8; ++c)
        for (int r = 0; r < rows; ++r)
            for (int ix = 0; ix < nx; ++ix)
                planes[c * planeStride + (dstRow0 + r) * nx + ix] = t[tiledIndex(nx, ix, row0 + r, c)];
}
void tileRows(const double* planes, std::size_t planeStride, std::size_t srcRow0, int nx, int rows, std::vector<double>& t)
{
    for (int c = 0; c < 8; ++c)
        for (int r = 0; r < rows; ++r)
            for (int ix = 0; ix < nx; ++ix)
                t[tiledIndex(nx, ix, r, c)] = planes[c * planeStride + (srcRow0 + r) * nx + ix];
}
// the stress components, in the order of S11a.. / S11b.. of Arr
std::vector<double> DynamicsState::*const STRESS[3] = { &DynamicsState::s11, &DynamicsState::s12, &DynamicsState::s22 };

// the eight members every plan descriptor starts with
template <class Desc> void fillGeometry(Desc& m, const DynamicsBlock& b)
{
    m.nx = b.nx, m.ny = b.ny, m.j0 = b.j0, m.j1 = b.j1, m.depth_below = b.depthBelow, m.depth_above = b.depthAbove;
    m.rank_below = b.peerBelow, m.rank_above = b.peerAbove;
}
// the ping-pong of stress and velocity and the packed nodal array of the mEVP and the brittle descriptor
template <class Desc> void fillPingPong(Desc& m, const DynamicsBlock& b)
{
    m.s11[0] = b.d[S11a], m.s12[0] = b.d[S12a], m.s22[0] = b.d[S22a], m.u[0] = b.d[Ua], m.v[0] = b.d[Va];
    m.s11[1] = b.d[S11b], m.s12[1] = b.d[S12b], m.s22[1] = b.d[S22b], m.u[1] = b.d[Ub], m.v[1] = b.d[Vb];
    m.packed = b.d[PACKED];
}
void toHost(void* host, const void* device, std::size_t bytes, const char* what) { checkHip(hipMemcpy(host, device, bytes, hipMemcpyDeviceToHost), what); }
void toDevice(void* device, const void* host, std::size_t bytes, const char* what) { checkHip(hipMemcpy(device, host, bytes, hipMemcpyHostToDevice), what); }
} // namespace

void setMultiProcess(bool on) { g_multiProcess = on; }

void check(int rc, const char* what)
{
    if (rc == NSDG_ERR_COMM && g_multiProcess) {
        // a neighbour rank has died (the bounded wait of nsdg_ctx_synchronize ran out): the device streams of this rank may
        // never drain, so no destructor may run (hipFree synchronises the device) -- leave at once with a non-zero
        // status; the launcher ends the remaining ranks
        std::fprintf(stderr, "nextsim_amd rank: %s: %s\n", what, nsdg_last_error());
        std::fflush(stderr);
        std::_Exit(3);
    }
    if (rc != NSDG_OK)
        throw std::runtime_error(std::string(what) + ": " + nsdg_last_error());
}
void checkHip(hipError_t e, const char* what)
{
    if (e != hipSuccess)
        throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}

DynamicsBlock::DynamicsBlock(int index_, int rank_, int world_, int device_, int nx_, int nyGlobal_, int below, int above, bool loop)
    : index(index_), rank(rank_), world(world_), device(device_), nx(nx_), nyGlobal(nyGlobal_), depthBelow(below), depthAbove(above)
{
    r0 = (int)(((long)rank * nyGlobal) / world); // DynamicsStep::splitRows
    r1 = (int)(((long)(rank + 1) * nyGlobal) / world);
    const bool hasBelow = rank > 0, hasAbove = rank < world - 1;
    lo = r0 - (hasBelow ? depthBelow : 0), hi = r1 + (hasAbove ? depthAbove : 0);
    ny = hi - lo;
    j0 = r0 - lo, j1 = r1 - lo;
    peerBelow = hasBelow ? (loop ? 0 : rank - 1) : -1;
    peerAbove = hasAbove ? (loop ? 0 : rank + 1) : -1;
    N = (long)nx * ny;
    NN = (long)(2 * nx + 1) * (2 * ny + 1);
    std::fill(slot, slot + NFIELD, -1);
}

DynamicsBlock::~DynamicsBlock()
{
    if (ctx)
        (void)hipSetDevice(device);
}

void DynamicsBlock::createContext(bool phaseTiming)
{
    nsdg_ctx* c = nullptr;
    check(nsdg_ctx_create(device, nullptr, &c), "nsdg_ctx_create");
    ctx.reset(c);
    if (phaseTiming)
        check(nsdg_phase_timing_set(c, 1), "nsdg_phase_timing_set");
}

void DynamicsBlock::allocate(bool brittle, bool advectColumn, int ntracers_, bool tiltSsh)
{
    ntracers = ntracers_;
    const long TS = nsdg_tiled_len(nx, ny, 8), TP = nsdg_tiled_len(nx, ny, 9);
    nfields = 0;
    for (int k = 0; k < NFIELD; ++k) {
        const AdvectedField::When w = ADVECTED[k].when;
        const bool in = w == AdvectedField::ALWAYS || (w == AdvectedField::BRITTLE && brittle) || (w == AdvectedField::COLUMN_STATE && advectColumn);
        slot[k] = in ? nfields++ : -1;
    }
    // [6][ny][nx] unless set below: VXDG, VYDG and, after the arrays of Arr, the three buffers of every advected field (adv)
    std::vector<long> sizes(NARR + 3 * nfields, 6 * N);
    if (ntracers > 0) { // the planes of the tracers, three buffers [6][ny][nx] per product, the plane of the thickness before the column step
        sizes.insert(sizes.end(), (std::size_t)ntracers, N);
        sizes.insert(sizes.end(), 3 * (std::size_t)ntracers, 6 * N);
        sizes.push_back(N);
    }
    for (int a : { S11a, S12a, S22a, S11b, S12b, S22b })
        sizes[a] = TS;
    sizes[PG] = TP;
    sizes[UNX] = 3L * (nx + 1) * ny, sizes[UNY] = 3L * nx * (ny + 1);
    for (int a : { Ua, Va, Ub, Vb, UA, VA, UO, VO })
        sizes[a] = NN;
    sizes[PACKED] = 8 * NN;
    sizes[COL] = (long)NCOL * N;
    for (int a : { HG, EG, PM })
        sizes[a] = brittle ? TP : 0;
    sizes[ZERO] = brittle ? NN : 0;
    sizes[SSH] = tiltSsh ? NN : 0;
    long total = 0;
    for (long s : sizes)
        total += (s + 1) & ~1L; // keep every sub-array 16-byte aligned
    arrays = deviceAlloc<double>((std::size_t)total, "DynamicsStep: hipMalloc");
    checkHip(hipMemset(arrays.get(), 0, total * sizeof(double)), "DynamicsStep: hipMemset");
    d.clear();
    long off = 0;
    for (long s : sizes) {
        d.push_back(arrays.get() + off);
        off += (s + 1) & ~1L;
    }
    par = tpar = qpar = 0;
}

void DynamicsBlock::setLandMask(const LandMaskFile& mask)
{
    land = deviceAlloc<std::uint8_t>((std::size_t)N, "DynamicsStep: hipMalloc (land mask)");
    toDevice(land.get(), mask.data() + (std::size_t)lo * nx, (std::size_t)N, "upload land mask");
    check(nsdg_land_mask_set(ctx.get(), land.get()), "nsdg_land_mask_set");
}

void DynamicsBlock::setBathymetry(const BathymetryFile& bathymetry, const nsdg_basal_params& params)
{
    depth = deviceAlloc<double>((std::size_t)N, "DynamicsStep: hipMalloc (bathymetry)");
    toDevice(depth.get(), bathymetry.data() + (std::size_t)lo * nx, (std::size_t)N * sizeof(double), "upload bathymetry");
    check(nsdg_basal_params_set(ctx.get(), &params), "nsdg_basal_params_set");
    check(nsdg_basal_depth_set(ctx.get(), depth.get()), "nsdg_basal_depth_set");
}

void DynamicsBlock::upload(const FieldStore& f, bool thermodynamics, bool announce)
{
    // cell means -> DG coefficient 0 (the local rows, ghost rows included, are one contiguous slice)
    const std::size_t first = (std::size_t)lo * nx, NG = (std::size_t)nx * nyGlobal, plane = N * sizeof(double);
    // a restart: the state a dynamics run left (FieldStore::dyn) -- higher DG2 coefficients, velocity, stress -- for the local
    // rows, ghost rows included (they hold what an exchange would deliver: the neighbours' own values)
    const DynamicsState& dy = f.dyn;
    for (int k = 0; k < NFIELD; ++k) {
        const AdvectedField& a = ADVECTED[k];
        if (slot[k] < 0 || !a.stored())
            continue;
        if (a.full) { // six planes of one host array; a file without it: the field starts at zero
            if (dy.present && (dy.*a.full).size() == 6 * NG)
                for (int c = 0; c < 6; ++c)
                    toDevice(adv(k, 0) + (long)c * N, (dy.*a.full).data() + (std::size_t)c * NG + first, plane, "upload DG coefficients");
            else if (dy.present && announce)
                std::printf("dynamics rheology bbm: the initial state holds no damage, the run starts undamaged (D = 0)\n");
            continue;
        }
        toDevice(adv(k, 0), (f.*a.mean).data() + first, plane, "upload cell means");
        if (!dy.present || (dy.*a.higher).size() != 5 * NG) // (a file without hsnow_dg: the higher coefficients of the snow start at zero)
            continue;
        for (int c = 1; c < 6; ++c)
            toDevice(adv(k, 0) + (long)c * N, (dy.*a.higher).data() + (std::size_t)(c - 1) * NG + first, plane, "upload DG coefficients");
    }
    if (dy.present) {
        const std::size_t nn = 2 * (std::size_t)nx + 1, nfirst = 2 * (std::size_t)lo * nn;
        toDevice(d[Ua], dy.u.data() + nfirst, NN * sizeof(double), "upload u");
        toDevice(d[Va], dy.v.data() + nfirst, NN * sizeof(double), "upload v");
        std::vector<double> t((std::size_t)nsdg_tiled_len(nx, ny, 8), 0.);
        for (int k = 0; k < 3; ++k) {
            tileRows((dy.*STRESS[k]).data(), NG, (std::size_t)lo, nx, ny, t);
            toDevice(d[S11a + k], t.data(), t.size() * sizeof(double), "upload stress");
        }
    }
    if (thermodynamics) {
        const std::vector<double>* planes[NCOL] = { &f.hsnow, &f.tice, &f.sst, &f.sss, &f.tair, &f.tdew, &f.slp, &f.qsw, &f.qlw, &f.mld,
            &f.snowfall, &f.wind, &f.newice };
        for (int c = 0; c < NCOL; ++c)
            toDevice(col(c), planes[c]->data() + first, plane, "upload column fields");
    }
}

void DynamicsBlock::uploadTracers(const FieldStore& f, const std::vector<std::string>& names, const std::vector<std::vector<double>>& init, bool announce)
{
    const std::size_t first = (std::size_t)lo * nx, NG = (std::size_t)nx * nyGlobal;
    for (int k = 0; k < ntracers; ++k) {
        const std::vector<double>* from = init[k].size() == NG ? &init[k] : nullptr; // (none: the plane stays at the zeros of allocate())
        if (f.dyn.present) { // a restart file takes precedence over dynamics.tracer_init; a file without the dataset: zeros
            from = nullptr;
            for (const DynamicsState::NamedPlane& t : f.dyn.tracers)
                if (t.name == names[k] && t.values.size() == NG)
                    from = &t.values;
            if (!from && announce)
                std::printf("dynamics tracers: the initial state holds no tracer_%s, the tracer starts at zero\n", names[k].c_str());
        }
        if (from)
            toDevice(tracer(k), from->data() + first, (std::size_t)N * sizeof(double), "upload tracer");
    }
}

void DynamicsBlock::setSlabOcean(const nsdg_slab_params& params)
{
    check(nsdg_slab_params_set(ctx.get(), &params), "nsdg_slab_params_set");
    const int planes = (params.relax_t > 0) + (params.relax_s > 0);
    sstExt = sssExt = nullptr;
    if (planes == 0)
        return;
    const std::size_t stride = ((std::size_t)N + 1) & ~(std::size_t)1; // both planes 16-byte aligned
    slabTargets = deviceAlloc<double>(planes * stride, "DynamicsStep: hipMalloc (slab ocean targets)");
    double* at = slabTargets.get();
    if (params.relax_t > 0)
        sstExt = at, at += stride;
    if (params.relax_s > 0)
        sssExt = at;
    for (const auto& pr : { std::make_pair(sstExt, col(C_SST)), std::make_pair(sssExt, col(C_SSS)) })
        if (pr.first)
            checkHip(hipMemcpy(pr.first, pr.second, (std::size_t)N * sizeof(double), hipMemcpyDeviceToDevice), "slab ocean targets");
}

void DynamicsBlock::allocateRecords(std::size_t count)
{
    records = deviceAlloc<double>(count, "DynamicsStep: hipMalloc (forcing records)");
    recordOf[0] = recordOf[1] = -1;
}

void DynamicsBlock::clearLand(bool thermodynamics)
{
    for (int k = 0; k < NFIELD; ++k)
        if (slot[k] >= 0 && ADVECTED[k].stored())
            check(nsdg_land_clear(ctx.get(), 0, ny, 6, adv(k, 0)), "nsdg_land_clear");
    if (thermodynamics) {
        check(nsdg_land_clear(ctx.get(), 0, ny, 1, col(C_HSNOW)), "nsdg_land_clear");
        check(nsdg_land_clear(ctx.get(), 0, ny, 1, col(C_NEWICE)), "nsdg_land_clear");
    }
    check(nsdg_land_clear_nodes(ctx.get(), d[Ua], d[Va]), "nsdg_land_clear_nodes");
    for (int k = 0; k < ntracers; ++k)
        check(nsdg_land_clear(ctx.get(), 0, ny, 1, tracer(k)), "nsdg_land_clear");
}

double* DynamicsBlock::outputBuffer(std::size_t count, const char* what)
{
    outputBuffers.push_back(deviceAlloc<double>(count, what));
    return outputBuffers.back().get();
}

void DynamicsBlock::makeMevpPlan(int nsub, bool overlap, bool graph)
{
    nsdg_rb_mevp_desc m;
    std::memset(&m, 0, sizeof m);
    fillGeometry(m, *this);
    fillPingPong(m, *this);
    m.nsub = nsub, m.overlap = overlap, m.use_graph = graph;
    m.pg = d[PG];
    nsdg_rb_mevp* plan = nullptr;
    check(nsdg_rb_mevp_create(ctx.get(), &m, &plan), "nsdg_rb_mevp_create");
    mevp.reset(plan);
}

void DynamicsBlock::makeBbmPlan(int nsub, bool overlap, bool completeNodes)
{
    check(nsdg_ctx_synchronize(ctx.get()), "DynamicsStep: brittle plan");
    bbm.reset();
    nsdg_rb_bbm_desc m;
    std::memset(&m, 0, sizeof m);
    fillGeometry(m, *this);
    fillPingPong(m, *this);
    m.nsub = nsub, m.overlap = overlap;
    m.complete_nodes = completeNodes;
    m.hg = d[HG], m.eg = d[EG], m.pm = d[PM];
    // the transport's two buffers of D, and its stage buffer of D -- free between two transport steps -- as the partner
    m.D[0] = adv(FD, 0), m.D[1] = adv(FD, 1), m.D_work = adv(FD, 2);
    nsdg_rb_bbm* plan = nullptr;
    check(nsdg_rb_bbm_create(ctx.get(), &m, &plan), "nsdg_rb_bbm_create");
    bbm.reset(plan);
    bbmNsub = nsub;
}

void DynamicsBlock::makeTransportPlan(bool closure)
{
    nsdg_rb_transport_desc t;
    std::memset(&t, 0, sizeof t);
    fillGeometry(t, *this);
    t.order = 2, t.nfields = nfields;
    t.vx_dg = d[VXDG], t.vy_dg = d[VYDG], t.un_x = d[UNX], t.un_y = d[UNY];
    t.own_bounds = 1, t.nbounds = closure ? t.nfields : 0; // the closure travels with the plan (its own bounds, not the context's)
    for (int k = 0; k < NFIELD; ++k)
        if (const int at = slot[k]; at >= 0)
            t.phi[at] = adv(k, 0), t.t1[at] = adv(k, 1), t.t2[at] = adv(k, 2), t.bounds[at] = ADVECTED[k].bounds;
    nsdg_rb_transport* plan = nullptr;
    check(nsdg_rb_transport_create(ctx.get(), &t, &plan), "nsdg_rb_transport_create");
    transport.reset(plan);
}

void DynamicsBlock::makeTracerPlan()
{
    nsdg_rb_transport_desc t;
    std::memset(&t, 0, sizeof t);
    fillGeometry(t, *this);
    t.order = 2, t.nfields = ntracers;
    t.vx_dg = d[VXDG], t.vy_dg = d[VYDG], t.un_x = d[UNX], t.un_y = d[UNY];
    t.own_bounds = 1, t.nbounds = 0; // every product is unbounded: no limiter, no cap, whatever the context says
    for (int k = 0; k < ntracers; ++k)
        t.phi[k] = tracerQ(k, 0), t.t1[k] = tracerQ(k, 1), t.t2[k] = tracerQ(k, 2);
    nsdg_rb_transport* plan = nullptr;
    check(nsdg_rb_transport_create(ctx.get(), &t, &plan), "nsdg_rb_transport_create (tracers)");
    tracerTransport.reset(plan);
}

nsdg_history_sources DynamicsBlock::sources(bool thermodynamics, bool advectColumn) const
{ // (D: the current damage of a brittle run)
    nsdg_history_sources src;
    std::memset(&src, 0, sizeof src);
    src.H = cur(FH), src.A = cur(FA), src.u = curU(), src.v = curV();
    const int s = par == 0 ? S11a : S11b;
    src.s11 = d[s], src.s12 = d[s + 1], src.s22 = d[s + 2];
    if (thermodynamics) // the snow plane the column step actually uses: plane 0 of S under dynamics.advect_column_state
        src.hsnow = advectColumn ? cur(FS) : col(C_HSNOW), src.tice = col(C_TICE);
    if (slot[FD] >= 0)
        src.D = cur(FD);
    return src;
}

void DynamicsBlock::ownedRowsToHost(double* hostPlane, int row0, const double* devicePlane, bool ghosted, const char* what) const
{
    toHost(hostPlane + (std::size_t)(r0 - row0) * nx, devicePlane + (ghosted ? (std::size_t)j0 * nx : 0), (std::size_t)ownedRows() * nx * sizeof(double), what);
}

void DynamicsBlock::download(FieldStore& f, bool thermodynamics, bool advectColumn, bool slabOcean) const
{
    if (slabOcean) { // the evolved mixed layer
        ownedRowsToHost(f.sst.data(), 0, col(C_SST), true, "download sst");
        ownedRowsToHost(f.sss.data(), 0, col(C_SSS), true, "download sss");
    }
    if (thermodynamics) {
        if (!advectColumn) // (otherwise f.hsnow receives the mean of S below: S is advected only under thermodynamics)
            ownedRowsToHost(f.hsnow.data(), 0, col(C_HSNOW), true, "download hsnow");
        ownedRowsToHost(f.tice.data(), 0, col(C_TICE), true, "download tice");
        ownedRowsToHost(f.newice.data(), 0, col(C_NEWICE), true, "download newice");
    }
    // the rest of the state a restart needs (FieldStore::dyn): higher DG2 coefficients, velocity, stress of the owned rows
    DynamicsState& dy = f.dyn;
    const std::size_t NG = (std::size_t)nx * nyGlobal;
    if (dy.hdg.size() != 5 * NG)
        dy.resize((std::size_t)nyGlobal, (std::size_t)nx);
    for (int k = 0; k < NFIELD; ++k) {
        const AdvectedField& a = ADVECTED[k];
        if (!a.stored())
            continue;
        if (a.full) { // all six planes in one host array, which exists only while the field is advected
            (dy.*a.full).resize(slot[k] >= 0 ? 6 * NG : 0, 0.);
            for (int c = 0; c < 6 && slot[k] >= 0; ++c)
                ownedRowsToHost((dy.*a.full).data() + (std::size_t)c * NG, 0, cur(k) + (long)c * N, true, "download DG coefficients");
            continue;
        }
        // the higher coefficients of a field exist only while it is advected: otherwise nothing of them is written
        (dy.*a.higher).resize(slot[k] >= 0 ? 5 * NG : 0, 0.);
        if (slot[k] < 0)
            continue;
        ownedRowsToHost((f.*a.mean).data(), 0, cur(k), true, "download cell means");
        for (int c = 1; c < 6; ++c)
            ownedRowsToHost((dy.*a.higher).data() + (std::size_t)(c - 1) * NG, 0, cur(k) + (long)c * N, true, "download DG coefficients");
    }
    // owned node rows: [2 j0, 2 j1) plus the top boundary row on the last block
    const long nn = 2L * nx + 1, rows = 2L * (j1 - j0) + (peerAbove < 0 ? 1 : 0);
    toHost(dy.u.data() + 2L * r0 * nn, curU() + 2L * j0 * nn, rows * nn * sizeof(double), "download u");
    toHost(dy.v.data() + 2L * r0 * nn, curV() + 2L * j0 * nn, rows * nn * sizeof(double), "download v");
    std::vector<double> t((std::size_t)nsdg_tiled_len(nx, ny, 8));
    for (int k = 0; k < 3; ++k) {
        toHost(t.data(), d[(par == 0 ? S11a : S11b) + k], t.size() * sizeof(double), "download stress");
        untileRows(t, nx, j0, j1 - j0, (dy.*STRESS[k]).data(), NG, (std::size_t)r0);
    }
}

void DynamicsBlock::downloadTracers(FieldStore& f, const std::vector<std::string>& names) const
{
    std::vector<DynamicsState::NamedPlane>& held = f.dyn.tracers;
    bool same = held.size() == names.size();
    for (std::size_t k = 0; same && k < names.size(); ++k)
        same = held[k].name == names[k] && held[k].values.size() == (std::size_t)nx * nyGlobal;
    if (!same) { // (the blocks of a process write disjoint rows of the same planes: made once)
        held.clear();
        for (const std::string& name : names)
            held.push_back({ name, std::vector<double>((std::size_t)nx * nyGlobal, 0.) });
    }
    for (int k = 0; k < ntracers; ++k)
        ownedRowsToHost(held[k].values.data(), 0, tracer(k), true, "download tracer");
}

RowRange::RowRange(const DynamicsBlocks& blocks)
    : row0(blocks[0]->r0)
    , row1(blocks[0]->r1)
{
    for (auto& b : blocks)
        row0 = std::min(row0, b->r0), row1 = std::max(row1, b->r1);
}

} // namespace Nextsim
