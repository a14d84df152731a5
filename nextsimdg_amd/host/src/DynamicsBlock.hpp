// DynamicsBlock.hpp -- one row block of DynamicsStep: its geometry, its context, its device arrays and its driver plans.  A private header
// of the host sources (DynamicsStep.cpp, DynamicsOutputs.cpp).
//
// Who owns what.  Everything that lives on a block's device is owned by the block and goes with it: the context, the one allocation of
// the arrays of Arr and of the advected fields, the forcing records, the land mask, the three driver plans and the buffers the outputs ask
// for (outputBuffer(): an output keeps the pointer and says what it holds, DynamicsOutputs.hpp).  DynamicsStep owns the blocks and the
// step across them.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <exception>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "../../../include/nsdg.h"
#include "IStructure.hpp"

namespace Nextsim {

class LandMaskFile;
class BathymetryFile;

//! one row block per process, ghost rows over RCCL: a dead neighbour then ends the process in check()
void setMultiProcess(bool on);
//! throws std::runtime_error "<what>: <nsdg_last_error>" unless rc is NSDG_OK
void check(int rc, const char* what);
void checkHip(hipError_t e, const char* what);

// The fields the DG2 transport advects, stated ONCE: the device buffers, the uploads and land clears of start(), the transport plan with
// its bounds and the downloads of stop() walk this table.  What one field alone needs is said where it happens, by the row's index.
struct AdvectedField {
    const char* name;
    nsdg_field_bounds bounds; // the closure of the transport step (include/nsdg.h "INPUT DOMAIN AND CLOSURE")
    std::vector<double> FieldStore::*mean; // the host's plane of coefficient 0 ...
    std::vector<double> DynamicsState::*higher; // ... and of coefficients 1..5
    std::vector<double> DynamicsState::*full; // or all six coefficients in one host array (no FieldStore plane holds the mean)
    // (all three nullptr: no host storage -- never uploaded, cleared or downloaded)
    enum When { ALWAYS, BRITTLE, COLUMN_STATE } when; // present in every run | with dynamics.rheology = bbm | with dynamics.advect_column_state
    bool stored() const { return mean || full; }
};
enum Field { FH, FA, FD, FS, FQ, NFIELD };
inline constexpr AdvectedField ADVECTED[NFIELD] = {
    { "H", { 0., HUGE_VAL, 0, 0 }, &FieldStore::hice, &DynamicsState::hdg, nullptr, AdvectedField::ALWAYS }, // mean thickness: H >= 0
    { "A", { 0., 1., 1, 0 }, &FieldStore::cice, &DynamicsState::adg, nullptr, AdvectedField::ALWAYS }, // concentration in [0, 1], the cell mean capped at 1
    { "D", { 0., 1., 0, 0 }, nullptr, nullptr, &DynamicsState::damage, AdvectedField::BRITTLE }, // damage in [0, 1], no cap of the mean
    { "S", { 0., HUGE_VAL, 0, 0 }, &FieldStore::hsnow, &DynamicsState::sdg, nullptr, AdvectedField::COLUMN_STATE }, // snow volume: S >= 0; plane 0 IS the column's hsnow
    { "Q", { -HUGE_VAL, HUGE_VAL, 0, 0 }, nullptr, nullptr, nullptr, AdvectedField::COLUMN_STATE }, // = H tice0, unbounded: rebuilt at every step (nsdg_tracer_weight)
};
// the table has five rows; a run advects H and A and EITHER the damage OR the column state (configure() refuses both together)
constexpr int fieldsOfARun(AdvectedField::When w)
{
    int n = 0;
    for (const AdvectedField& a : ADVECTED)
        n += a.when == AdvectedField::ALWAYS || a.when == w;
    return n;
}
static_assert(fieldsOfARun(AdvectedField::BRITTLE) <= NSDG_RB_MAX_FIELDS && fieldsOfARun(AdvectedField::COLUMN_STATE) <= NSDG_RB_MAX_FIELDS,
    "the transport plan holds every advected field of a run");

// further device arrays of a block; the stress (its components in the order of DynamicsBlock.cpp's STRESS) and the velocity exist twice
// (ping-pong)
// (HG, EG, PM, ZERO: the Gauss arrays of nsdg_bbm_prepare and the zero nodal array its packing takes as u0, v0 -- empty under mEVP;
// SSH: the sea-surface height at the nodes of dynamics.tilt = ssh -- empty without it)
enum Arr { S11a, S12a, S22a, S11b, S12b, S22b, PG, VXDG, VYDG, UNX, UNY, Ua, Va, Ub, Vb, UA, VA, UO, VO, PACKED, COL, HG, EG, PM, ZERO, SSH, NARR };
// column planes inside COL
enum Col { C_HSNOW, C_TICE, C_SST, C_SSS, C_TAIR, C_TDEW, C_SLP, C_QSW, C_QLW, C_MLD, C_SNOWFALL, C_WIND, C_NEWICE, NCOL };

// owning handles: device memory, the context, the driver plans
struct HipFree {
    void operator()(void* p) const { (void)hipFree(p); }
};
template <class T> using DeviceBuffer = std::unique_ptr<T[], HipFree>;
template <class T> DeviceBuffer<T> deviceAlloc(std::size_t count, const char* what)
{
    void* p = nullptr;
    checkHip(hipMalloc(&p, count * sizeof(T)), what);
    return DeviceBuffer<T>(static_cast<T*>(p));
}
template <class T, int (*destroy)(T*)> struct NsdgDestroy {
    void operator()(T* p) const { (void)destroy(p); }
};
template <class T, int (*destroy)(T*)> using NsdgHandle = std::unique_ptr<T, NsdgDestroy<T, destroy>>;

class DynamicsBlock {
public:
    //! block `rank` of `world` on `device`, the `index`-th of this process: nx columns of nyGlobal rows, nominal ghost depths (below,
    //! above); loop: dynamics.loopback_world (both neighbours are rank 0 of the communicator)
    DynamicsBlock(int index, int rank, int world, int device, int nx, int nyGlobal, int depthBelow, int depthAbove, bool loop);
    ~DynamicsBlock(); //!< sets the device; then the handles go, last member first

    // geometry: global rows [r0, r1) owned, [lo, hi) held locally; j0/j1 = owned local rows
    const int index, rank, world, device;
    const int nx, nyGlobal;
    int r0 = 0, r1 = 0, lo = 0, hi = 0, ny = 0, j0 = 0, j1 = 0;
    int depthBelow = 0, depthAbove = 0, peerBelow = -1, peerAbove = -1;
    long N = 0, NN = 0;
    int ownedRows() const { return r1 - r0; }

    // ---- the handles, in the reverse of the order in which they go: the plans, the arrays, the forcing records, the outputs' buffers
    // (first asked for, first freed), the context (which finalises the communicator too) and last the land mask the context held
    DeviceBuffer<std::uint8_t> land; // dynamics.land_mask_file: the mask of the local rows, ghost rows included (set on the context)
    DeviceBuffer<double> depth; // dynamics.bathymetry_file: the water depth of the same rows (set on the context, freed after it like the mask)
    NsdgHandle<nsdg_ctx, nsdg_ctx_destroy> ctx;
    std::vector<DeviceBuffer<double>> outputBuffers; // what outputBuffer() handed out
    // dynamics.forcing = file: two records of every variable of the file on the device (slot s: variables one after the other, in the
    // order of ForcingFile::variables()), and which record each slot holds (-1: none)
    DeviceBuffer<double> records;
    long recordOf[2] = { -1, -1 };
    // dynamics.slab_ocean: the relaxation targets of sst and sss, N doubles each, for the relaxation times that are set (null: not read)
    DeviceBuffer<double> slabTargets;
    double *sstExt = nullptr, *sssExt = nullptr;
    DeviceBuffer<double> arrays; // the arrays of Arr and the buffers of the advected fields: one allocation
    NsdgHandle<nsdg_rb_transport, nsdg_rb_transport_destroy> transport;
    NsdgHandle<nsdg_rb_transport, nsdg_rb_transport_destroy> tracerTransport; // dynamics.tracers: the second transport group, without bounds
    NsdgHandle<nsdg_rb_bbm, nsdg_rb_bbm_destroy> bbm; // dynamics.rheology = bbm: the plan of the current sub-iteration count (made when that is known)
    int bbmNsub = -1;
    NsdgHandle<nsdg_rb_mevp, nsdg_rb_mevp_destroy> mevp;

    // the arrays of Arr, then three buffers per advected field (adv), then -- dynamics.tracers -- one plane per tracer, three buffers per
    // tracer's product Q = H T and the plane of the mean thickness before the column step
    std::vector<double*> d;
    int ntracers = 0; // dynamics.tracers: how many
    int qpar = 0; // which buffers hold the tracers' products (the parity of the second transport plan)
    int nfields = 0; // rows of ADVECTED this run advects ...
    int slot[NFIELD]; // ... and where each sits among the device buffers and in the transport plan (-1: not in this run)
    int par = 0, tpar = 0; // which buffers hold the velocity/stress iterate and the advected state
    double amax = 0.; // largest concentration of the owned rows at the start of the model step (dynamics.substeps = auto)

    // ---- the steps of DynamicsStep::start(), in its order
    //! the context on the block's device (made current), with phase timing if asked for
    void createContext(bool phaseTiming);
    //! which rows of ADVECTED this run advects; the arrays of Arr and the advected fields: one allocation, zeroed, every array 16-byte aligned
    //! ntracers: the planes and buffers of dynamics.tracers as well
    void allocate(bool brittle, bool advectColumn, int ntracers = 0, bool tiltSsh = false);
    //! the block's rows of the mask, ghost rows included, on the device and on the context: the mask is static, nothing is ever exchanged
    void setLandMask(const LandMaskFile& mask);
    //! the block's rows of the water depth, ghost rows included, and the grounding scheme's parameters, on the device and on the context
    //! (landfast ice, include/nsdg_basal.h): static like the mask, nothing is ever exchanged
    void setBathymetry(const BathymetryFile& bathymetry, const nsdg_basal_params& params);
    //! the local rows, ghost rows included, of the structure's cell means and, if a dynamics run left it (FieldStore::dyn), of its state;
    //! with thermodynamics the column planes.  announce: this block prints the line about a restart file without damage
    void upload(const FieldStore& f, bool thermodynamics, bool announce);
    //! dynamics.tracers: the local rows of every named tracer -- from the state a restart file left (FieldStore::dyn.tracers, by name), else
    //! from the plane of dynamics.tracer_init (empty: zeros).  announce: this block prints the line about a restart file without a tracer
    void uploadTracers(const FieldStore& f, const std::vector<std::string>& names, const std::vector<std::vector<double>>& init, bool announce);
    //! dynamics.slab_ocean, after upload(): the parameters on the context, and a target plane per relaxation time that is set, filled with
    //! the initial sst / sss of the local rows (what a forcing file's pair sst, sss replaces at every step)
    void setSlabOcean(const nsdg_slab_params& params);
    //! dynamics.forcing = file: room for `count` doubles of records, none resident yet
    void allocateRecords(std::size_t count);
    //! no ice on land, no motion at land nodes, whatever the initial state or the restart file held there
    void clearLand(bool thermodynamics);
    //! device memory of `count` doubles that lives as long as the block, not initialised: what an output keeps on this block's device
    double* outputBuffer(std::size_t count, const char* what);
    void makeMevpPlan(int nsub, bool overlap, bool graph);
    //! replaces the brittle plan, after the work queued on the context, which may still run the old one
    void makeBbmPlan(int nsub, bool overlap, bool completeNodes);
    void makeTransportPlan(bool closure);
    void makeTracerPlan(); //!< dynamics.tracers: a second transport plan over the tracers' products, created without bounds

    // ---- reading the state
    // per advected field, after the arrays of Arr: the two halves of the ping-pong (h = 0, 1; tpar says which is current), the stage buffer (2)
    double* adv(int k, int h) const { return d[NARR + 3 * slot[k] + h]; } // k: a row of ADVECTED that is in this run
    double* cur(int k) const { return adv(k, tpar); }
    double* curU() const { return d[par == 0 ? Ua : Ub]; }
    double* curV() const { return d[par == 0 ? Va : Vb]; }
    double* col(int k) const { return d[COL] + (long)k * N; }
    // dynamics.tracers, after the advected fields: the plane of tracer k, the buffers of its product (h as for adv; qpar says which is
    // current), the plane of the mean thickness before the column step
    double* tracer(int k) const { return d[NARR + 3 * nfields + k]; }
    double* tracerQ(int k, int h) const { return d[NARR + 3 * nfields + ntracers + 3 * k + h]; }
    double* thicknessBefore() const { return d[NARR + 3 * nfields + 4 * ntracers]; }
    //! what a history sample, the row totals and the point samples read: the current side of every ping-pong
    nsdg_history_sources sources(bool thermodynamics, bool advectColumn) const;
    //! the owned rows of a device plane of nx columns -- of the owned rows alone, or (ghosted) of every local row -- into a host plane
    //! that starts at global row `row0`
    void ownedRowsToHost(double* hostPlane, int row0, const double* devicePlane, bool ghosted, const char* what) const;
    //! stop(): the owned rows of the state a restart needs into the structure (the caller has drained the context)
    //! slabOcean: sst and sss with them
    void download(FieldStore& f, bool thermodynamics, bool advectColumn, bool slabOcean = false) const;
    //! stop(): the owned rows of the tracers into FieldStore::dyn.tracers, under their names
    void downloadTracers(FieldStore& f, const std::vector<std::string>& names) const;
};

using DynamicsBlocks = std::vector<std::unique_ptr<DynamicsBlock>>;

//! the rows [row0, row1) the blocks of this process own together
struct RowRange {
    int row0, row1;
    explicit RowRange(const DynamicsBlocks& blocks);
    std::size_t rows() const { return (std::size_t)(row1 - row0); }
};

//! f(block) for every block, one after the other, each on its device
template <class F> void forEachBlockInTurn(const DynamicsBlocks& blocks, F&& f)
{
    for (auto& b : blocks) {
        checkHip(hipSetDevice(b->device), "hipSetDevice");
        f(*b);
    }
}
//! f(block) for every block, each on its device; one thread per block when there are several: the in-process transport hands ghost rows
//! over between host threads
template <class F> void forEachBlock(const DynamicsBlocks& blocks, F&& f)
{
    if (blocks.size() == 1)
        return forEachBlockInTurn(blocks, f);
    std::vector<std::thread> threads;
    std::vector<std::exception_ptr> errors(blocks.size());
    for (std::size_t k = 0; k < blocks.size(); ++k)
        threads.emplace_back([&, k] {
            try {
                checkHip(hipSetDevice(blocks[k]->device), "hipSetDevice");
                f(*blocks[k]);
            } catch (...) {
                errors[k] = std::current_exception();
            }
        });
    for (auto& t : threads)
        t.join();
    for (auto& e : errors)
        if (e)
            std::rethrow_exception(e);
}

} // namespace Nextsim
