#include "DynamicsStep.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <limits>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <sstream>
#include <stdexcept>
#include <thread>

#include "../../../include/nsdg.h"
#include "Drifters.hpp"
#include "Stations.hpp"
#include "ForcingFile.hpp"
#include "HistoryOutput.hpp"
#include "LandMaskFile.hpp"
#include "ModuleLoader.hpp"
#include "PhaseTiming.hpp"
#include "PhysicsModules.hpp"
#include "Rendezvous.hpp"
#include "Timer.hpp"

namespace Nextsim {

namespace {
bool g_multiProcess = false; // one row block per process, ghost rows over RCCL
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
std::atomic<long> g_localGroup { 1 }; // ids of the in-process communicator groups of this process

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
constexpr AdvectedField ADVECTED[NFIELD] = {
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

// further device arrays of a block; the stress (its components in the order of STRESS) and the velocity exist twice (ping-pong)
std::vector<double> DynamicsState::*const STRESS[3] = { &DynamicsState::s11, &DynamicsState::s12, &DynamicsState::s22 };
// (HG, EG, PM, ZERO: the Gauss arrays of nsdg_bbm_prepare and the zero nodal array its packing takes as u0, v0 -- empty under mEVP)
enum Arr { S11a, S12a, S22a, S11b, S12b, S22b, PG, VXDG, VYDG, UNX, UNY, Ua, Va, Ub, Vb, UA, VA, UO, VO, PACKED, COL, HG, EG, PM, ZERO, NARR };
// column planes inside COL
enum Col { C_HSNOW, C_TICE, C_SST, C_SSS, C_TAIR, C_TDEW, C_SLP, C_QSW, C_QLW, C_MLD, C_SNOWFALL, C_WIND, C_NEWICE, NCOL };
} // namespace

// ------------------------------------------------------------------------------------------------ one row block
class DynamicsBlock {
public:
    // geometry: global rows [r0, r1) owned, [lo, hi) held locally; j0/j1 = owned local rows
    int rank = 0, world = 1, device = 0;
    int nx = 0, nyGlobal = 0, r0 = 0, r1 = 0, lo = 0, hi = 0, ny = 0, j0 = 0, j1 = 0;
    int depthBelow = 0, depthAbove = 0, peerBelow = -1, peerAbove = -1;
    long N = 0, NN = 0;
    nsdg_ctx* ctx = nullptr;
    double* block = nullptr;
    std::vector<double*> d;
    int nfields = 0; // rows of ADVECTED this run advects ...
    int slot[NFIELD]; // ... and where each sits among the device buffers and in the transport plan (-1: not in this run)
    nsdg_rb_mevp* mevp = nullptr;
    nsdg_rb_bbm* bbm = nullptr; // dynamics.rheology = bbm: the plan of the current sub-iteration count (made when that is known)
    int bbmNsub = -1;
    nsdg_rb_transport* transport = nullptr;
    int par = 0, tpar = 0; // which buffers hold the velocity/stress iterate and the advected state
    double amax = 0.; // largest concentration of the owned rows at the start of the model step (dynamics.substeps = auto)
    // dynamics.forcing = file: two records of every variable of the file on the device (slot s: variables one after the other, in the
    // order of ForcingFile::variables()), and which record each slot holds (-1: none)
    double* records = nullptr;
    long recordOf[2] = { -1, -1 };
    std::uint8_t* land = nullptr; // dynamics.land_mask_file: the mask of the local rows, ghost rows included (set on the context)
    double* hist = nullptr; // model.output_period: the history accumulator, one plane of the OWNED rows per output field (null: off)
    double* histWeight = nullptr; // ... and the summed weights of its ice-weighted means, one plane (null: none is asked for)
    double* series = nullptr; // model.series_file: [model.series_buffer][quantities][owned rows] row totals (null: off)
    // model.drifters_file: the whole list [3][n] on every block, twice -- a step is out of place; dpar says which half is current (null: off)
    double* drift[2] = { nullptr, nullptr };
    int dpar = 0;
    double* driftSamples = nullptr; // model.drifters_fields: [fields][n], the samples at the current positions (null: off)
    // model.stations_file: the positions [2][n] and [model.stations_buffer][fields][n] samples (null: off)
    double* stationXY = nullptr;
    double* stations = nullptr;

    ~DynamicsBlock() { release(); }
    void release()
    {
        if (ctx)
            (void)hipSetDevice(device);
        nsdg_rb_mevp_destroy(mevp);
        nsdg_rb_bbm_destroy(bbm);
        nsdg_rb_transport_destroy(transport);
        mevp = nullptr, bbm = nullptr, transport = nullptr;
        if (block)
            (void)hipFree(block);
        block = nullptr;
        if (records)
            (void)hipFree(records);
        records = nullptr;
        if (hist)
            (void)hipFree(hist);
        hist = nullptr;
        if (histWeight)
            (void)hipFree(histWeight);
        histWeight = nullptr;
        if (series)
            (void)hipFree(series);
        series = nullptr;
        for (double*& p : drift) {
            if (p)
                (void)hipFree(p);
            p = nullptr;
        }
        for (double** p : { &driftSamples, &stationXY, &stations }) {
            if (*p)
                (void)hipFree(*p);
            *p = nullptr;
        }
        if (ctx)
            nsdg_ctx_destroy(ctx); // finalises the communicator too
        if (land) // after the context, which held the pointer
            (void)hipFree(land);
        land = nullptr;
        ctx = nullptr;
    }
    // per advected field, after the arrays of Arr: the two halves of the ping-pong (h = 0, 1; tpar says which is current), the stage buffer (2)
    double* adv(int k, int h) const { return d[NARR + 3 * slot[k] + h]; } // k: a row of ADVECTED that is in this run
    double* cur(int k) const { return adv(k, tpar); }
    double* curU() const { return d[par == 0 ? Ua : Ub]; }
    double* curV() const { return d[par == 0 ? Va : Vb]; }
    double* col(int k) const { return d[COL] + (long)k * N; }
};

template <>
const std::map<int, std::string> Configured<DynamicsStep>::keyMap = { { 0, "dynamics.domain_size" }, { 1, "dynamics.nsub" },
    { 2, "dynamics.alpha" }, { 3, "dynamics.beta" }, { 4, "dynamics.thermodynamics" }, { 5, "dynamics.row_blocks" },
    { 6, "dynamics.passes_per_exchange" }, { 7, "dynamics.overlap" }, { 8, "dynamics.graph" }, { 9, "dynamics.forcing" },
    { 10, "dynamics.devices" }, { 11, "dynamics.loopback_world" }, { 12, "dynamics.closure" }, { 13, "dynamics.min_conc" },
    { 14, "dynamics.min_thick" }, { 15, "dynamics.delta_min" }, { 16, "dynamics.subcycle" }, { 17, "dynamics.substeps" },
    { 18, "dynamics.substep_courant" }, { 19, "dynamics.max_substeps" }, { 20, "dynamics.forcing_file" },
    { 21, "dynamics.advect_column_state" }, { 22, "dynamics.land_mask_file" }, { 23, "dynamics.rheology" },
    { 24, "dynamics.bbm_courant" } };

// dynamics.rheology = bbm
struct DynamicsStep::Brittle {
    nsdg_bbm_params params;
    double courant = NSDG_BBM_COURANT;
    bool warned = false; // the line about an explicit dynamics.nsub below the rule's value has been printed
};
namespace {
struct BbmKey {
    const char* key;
    double nsdg_bbm_params::*member;
};
const BbmKey BBM_KEYS[] = { { "bbm.young", &nsdg_bbm_params::young }, { "bbm.nu", &nsdg_bbm_params::nu }, { "bbm.p0", &nsdg_bbm_params::p0 },
    { "bbm.lambda0", &nsdg_bbm_params::lambda0 }, { "bbm.tan_phi", &nsdg_bbm_params::tan_phi }, { "bbm.cohesion_lab", &nsdg_bbm_params::cohesion_lab },
    { "bbm.compr_strength", &nsdg_bbm_params::compr_strength }, { "bbm.t_heal", &nsdg_bbm_params::t_heal }, { "bbm.d_max", &nsdg_bbm_params::d_max } };
const char* const BBM_EXPONENT_KEY = "bbm.relax_exponent";
} // namespace

const std::vector<std::string>& DynamicsStep::brittleKeys()
{
    static const std::vector<std::string> keys = [] {
        std::vector<std::string> k = { keyMap.at(23), keyMap.at(24), BBM_EXPONENT_KEY };
        for (const BbmKey& b : BBM_KEYS)
            k.push_back(b.key);
        return k;
    }();
    return keys;
}

DynamicsStep::DynamicsStep() = default;
DynamicsStep::~DynamicsStep() { release(); }

void DynamicsStep::release() { m_blocks.clear(); }

DynamicsStep::SubcycleChoice DynamicsStep::subcycleChoice(double h, double dt) const
{ // the stability rule lives in the library (nsdg_mevp_stable_params): the host only says which of its forms it wants
    nsdg_mevp_params p;
    nsdg_mevp_default_params(&p);
    if (deltaMin > 0)
        p.delta_min = deltaMin;
    const std::string mode = subcycle;
    if (mode == "keep_alpha") {
        p.alpha = alpha > 0 ? alpha : 1500.;
        check(nsdg_mevp_stable_params(&p, NSDG_SUBCYCLE_KEEP_ALPHA, h, dt), "nsdg_mevp_stable_params");
        if (beta > 0)
            p.beta = beta;
    } else if (mode == "keep_delta_min")
        check(nsdg_mevp_stable_params(&p, NSDG_SUBCYCLE_KEEP_DELTA_MIN, h, dt), "nsdg_mevp_stable_params");
    else
        check(nsdg_mevp_stable_params(&p, mode == "adaptive_converged" ? NSDG_SUBCYCLE_ADAPTIVE_CONVERGED : NSDG_SUBCYCLE_ADAPTIVE, h, dt), "nsdg_mevp_stable_params");
    return SubcycleChoice { mode, p.alpha, p.beta, p.delta_min, p.aevp_c, p.aevp_alpha_min, nsdg_mevp_creep_percent_per_day(&p) };
}

void DynamicsStep::splitRows(int ny, int world, int rank, int& r0, int& r1)
{
    r0 = (int)(((long)rank * ny) / world);
    r1 = (int)(((long)(rank + 1) * ny) / world);
}

void DynamicsStep::configure()
{
    L = getConfiguration(keyMap.at(0), 512e3);
    nsub = getConfiguration(keyMap.at(1), 120);
    {
        std::string raw;
        nsubGiven = Configurator::lookup(keyMap.at(1), raw);
    }
    alpha = getConfiguration(keyMap.at(2), 0.);
    beta = getConfiguration(keyMap.at(3), 0.);
    thermo = getConfiguration(keyMap.at(4), false);
    rowBlocks = getConfiguration(keyMap.at(5), 1);
    passesPerExchange = getConfiguration(keyMap.at(6), 2); // the best of the rehearsed 8-block runs at both modelled link rates
    overlap = getConfiguration(keyMap.at(7), true);
    graph = getConfiguration(keyMap.at(8), false);
    forcing = getConfiguration(keyMap.at(9), std::string("host"));
    devices = getConfiguration(keyMap.at(10), std::string(""));
    loopbackWorld = getConfiguration(keyMap.at(11), 0);
    // the closure that keeps the dynamics inside the physical range (include/nsdg.h "INPUT DOMAIN AND CLOSURE"): ridging cap and
    // scaling limiter at the end of a transport step, free drift at ice-free nodes with the column model's cut-off values
    // (nextsim_thermo.min_conc / min_thick, physics/src/modules/NextsimPhysics.cpp:81-82); closure = false: the bare scheme
    closure = getConfiguration(keyMap.at(12), true);
    minConc = getConfiguration(keyMap.at(13), 1e-12);
    minThick = getConfiguration(keyMap.at(14), 0.01);
    // sub-cycle parameters (include/nsdg.h: nsdg_mevp_stable_params): adaptive alpha / beta unless the configuration names a uniform
    // alpha (then keep_alpha: round 5) or says otherwise
    deltaMin = getConfiguration(keyMap.at(15), 0.);
    subcycle = getConfiguration(keyMap.at(16), std::string(alpha > 0 ? "keep_alpha" : "adaptive"));
    if (subcycle != "adaptive" && subcycle != "adaptive_converged" && subcycle != "keep_alpha" && subcycle != "keep_delta_min")
        throw std::invalid_argument("dynamics.subcycle must be adaptive, adaptive_converged, keep_alpha or keep_delta_min");
    // sub-stepping of the model step (include/nsdg.h "sub-stepping"); off by default
    {
        const std::string v = getConfiguration(keyMap.at(17), std::string("1"));
        std::size_t used = 0;
        long k = 0;
        try {
            k = v == "auto" ? 0 : std::stol(v, &used);
        } catch (const std::exception&) {
            used = 0;
        }
        if (v != "auto" && (used != v.size() || k < 1 || k > 1000000))
            throw std::invalid_argument("dynamics.substeps must be an integer >= 1 or auto");
        substeps = (int)k;
    }
    substepCourant = getConfiguration(keyMap.at(18), (double)NSDG_SUBSTEP_COURANT);
    maxSubsteps = getConfiguration(keyMap.at(19), 16);
    if (!(std::isfinite(substepCourant) && substepCourant > 0))
        throw std::invalid_argument("dynamics.substep_courant must be positive");
    if (maxSubsteps < 1)
        throw std::invalid_argument("dynamics.max_substeps must be >= 1");
    timing = getConfiguration(std::string("model.timing"), false);
    phaseTiming = PhaseTiming::enabled();
    if (rowBlocks < 1 || passesPerExchange < 1 || nsub < 0)
        throw std::invalid_argument("dynamics.row_blocks and dynamics.passes_per_exchange must be >= 1, dynamics.nsub >= 0");
    if (forcing != "host" && forcing != "dummy" && forcing != "winter" && forcing != "file")
        throw std::invalid_argument("dynamics.forcing must be host, dummy, winter or file");
    // forcing records from a file: read and checked here, before any device is touched
    m_forcingFile.reset();
    if (forcing == "file") {
        const std::string path = getConfiguration(keyMap.at(20), std::string(""));
        if (path.empty())
            throw std::invalid_argument("dynamics.forcing = file needs dynamics.forcing_file");
        m_forcingFile = std::make_shared<const ForcingFile>(path, thermo);
        if (!thermo && !m_forcingFile->hasWind() && !m_forcingFile->hasOcean())
            throw std::invalid_argument("dynamics.forcing_file " + path + ": without dynamics.thermodynamics the run uses only wind_u / wind_v "
                                        "and ocean_u / ocean_v, and the file holds neither pair");
    }
    // the land mask: read and checked here, before any device is touched (the shape against the structure, once there is one)
    m_landMask.reset();
    {
        const std::string path = getConfiguration(keyMap.at(22), std::string(""));
        if (!path.empty()) {
            m_landMask = std::make_shared<const LandMaskFile>(path);
            if (pStructure)
                m_landMask->checkShape((std::size_t)pStructure->nx(), (std::size_t)pStructure->ny());
        }
    }
    if (loopbackWorld != 0 && loopbackWorld < 3)
        throw std::invalid_argument("dynamics.loopback_world needs an interior block: at least 3");
    // the snow and the surface temperature ride on the moving ice (include/nsdg.h "column state transport"); off by default
    advectColumn = getConfiguration(keyMap.at(21), false);
    if (advectColumn && !thermo)
        throw std::invalid_argument("dynamics.advect_column_state needs dynamics.thermodynamics = true: without the column model there is no "
                                    "snow or surface temperature to carry");
    // the rheology (include/nsdg.h "brittle rheology"): its keys are read and checked here, before any device is touched
    m_brittle.reset();
    {
        const std::string rheology = getConfiguration(keyMap.at(23), std::string("mevp"));
        if (rheology != "mevp" && rheology != "bbm")
            throw std::invalid_argument("dynamics.rheology must be mevp or bbm, got \"" + rheology + "\"");
        if (rheology == "bbm") {
            if (advectColumn)
                throw std::invalid_argument("dynamics.rheology = bbm with dynamics.advect_column_state = true would advect five fields (H, A, D, S, Q); "
                                            "a transport step carries at most " + std::to_string(NSDG_RB_MAX_FIELDS));
            if (substeps == 0)
                throw std::invalid_argument("dynamics.rheology = bbm with dynamics.substeps = auto: that rule is the strength wave of the mEVP "
                                            "rheology; give an integer");
            if (graph)
                throw std::invalid_argument("dynamics.rheology = bbm with dynamics.graph = true: the brittle sub-cycle exchanges after every "
                                            "sub-iteration and replays no graph");
            m_brittle = std::make_unique<Brittle>();
            nsdg_bbm_default_params(&m_brittle->params);
            for (const BbmKey& k : BBM_KEYS)
                m_brittle->params.*k.member = getConfiguration(std::string(k.key), m_brittle->params.*k.member);
            m_brittle->params.relax_exponent = getConfiguration(std::string(BBM_EXPONENT_KEY), (int)m_brittle->params.relax_exponent);
            if (nsdg_bbm_params_check(&m_brittle->params) != NSDG_OK)
                throw std::invalid_argument(std::string("[bbm]: ") + nsdg_last_error());
            m_brittle->courant = getConfiguration(keyMap.at(24), (double)NSDG_BBM_COURANT);
            if (!(std::isfinite(m_brittle->courant) && m_brittle->courant > 0))
                throw std::invalid_argument("dynamics.bbm_courant must be positive");
        }
    }
    // history output (include/HistoryOutput.hpp): the keys are read and checked here, before any device is touched; period 0 = off
    m_history.reset();
    const HistoryOutput::Config hc = HistoryOutput::fromConfiguration(thermo, m_brittle != nullptr);
    if (hc.on())
        m_history = std::make_unique<HistoryOutput>(hc);
    // the time series of the domain totals (SeriesOutput): the same; a multi-process run is refused here, nothing gathers its rows
    m_series.reset();
    const SeriesOutput::Config sc = SeriesOutput::fromConfiguration(thermo, RankEnvironment::fromEnv().world);
    if (sc.on())
        m_series = std::make_unique<SeriesOutput>(sc);
    // drifters (include/Drifters.hpp): the keys and the input file are read and checked here, before any device is touched; a
    // multi-process run is refused here
    m_drifters.reset();
    m_drifterStart.clear();
    const DriftersOutput::Config dc = DriftersOutput::fromConfiguration(RankEnvironment::fromEnv().world, loopbackWorld != 0, thermo, m_brittle != nullptr);
    if (dc.on()) {
        m_drifterStart = DriftersOutput::read(dc.file, L, L);
        m_drifters = std::make_unique<DriftersOutput>(dc);
    }
    // stations (include/Stations.hpp): the same
    m_stations.reset();
    m_stationXY.clear();
    const StationsOutput::Config stc = StationsOutput::fromConfiguration(RankEnvironment::fromEnv().world, loopbackWorld != 0, thermo, m_brittle != nullptr);
    if (stc.on()) {
        m_stationXY = StationsOutput::read(stc.file, L, L);
        m_stations = std::make_unique<StationsOutput>(stc);
    }
}

void DynamicsStep::init()
{
    configure();
    const RankEnvironment env = RankEnvironment::fromEnv();
    m_world = env.world, m_rank = env.rank;
    g_multiProcess = m_world > 1;
    if (m_world > 1 && (rowBlocks > 1 || loopbackWorld))
        throw std::invalid_argument("a multi-process run (WORLD_SIZE > 1) owns one row block per process: leave dynamics.row_blocks / loopback_world unset");
    if (rowBlocks > 1 && loopbackWorld)
        throw std::invalid_argument("dynamics.row_blocks and dynamics.loopback_world exclude each other");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        throw std::runtime_error(std::string("DynamicsStep::init: no HIP device available"));
    if (thermo) { // the column-physics plugins read their keys once (shared static instances, as in the reference)
        tryConfigure(ModuleLoader::getLoader().getImplementation<IPhysics1d>());
        tryConfigure(ModuleLoader::getLoader().getImplementation<IFreezingPoint>());
    }
    m_inited = true;
}

template <class F> void DynamicsStep::forEachBlock(F&& f)
{
    if (m_blocks.size() == 1) {
        f(*m_blocks[0]);
        return;
    }
    // the in-process transport hands ghost rows over between host threads: one thread per block
    std::vector<std::thread> threads;
    std::vector<std::exception_ptr> errors(m_blocks.size());
    for (std::size_t k = 0; k < m_blocks.size(); ++k)
        threads.emplace_back([&, k] {
            try {
                f(*m_blocks[k]);
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

void DynamicsStep::start(const Iterator::TimePoint& startTime)
{
    ScopedTimer timer("start (upload)");
    if (!pStructure)
        throw std::logic_error("DynamicsStep: setInitialData() was not called");
    if (!m_inited)
        init();
    FieldStore& f = pStructure->fields();
    nxf = pStructure->ny(); // fast dimension of the x-major index i*ny + j
    nyf = pStructure->nx();
    m_time = (double)startTime;
    if (m_history)
        m_history->start((long)startTime); // the integer clock the output windows are aligned to (m_time is a double under sub-stepping)
    if (m_series)
        m_series->start((long)startTime);
    if (m_drifters)
        m_drifters->start((long)startTime);
    if (m_stations)
        m_stations->start((long)startTime);
    if (m_landMask) {
        m_landMask->checkShape((std::size_t)nyf, (std::size_t)nxf);
        if (m_rank == 0)
            std::printf("dynamics land mask: %zu of %zu elements are land (%s)\n", m_landMask->landElements(), (std::size_t)nxf * nyf,
                m_landMask->path().c_str());
    }

    // ---- the blocks of this process
    const bool loop = loopbackWorld > 0;
    const int world = m_world > 1 ? m_world : (loop ? loopbackWorld : rowBlocks);
    int ndev = 1;
    (void)hipGetDeviceCount(&ndev);
    std::vector<int> devs;
    {
        std::stringstream ss(devices);
        std::string item;
        while (std::getline(ss, item, ','))
            if (!item.empty())
                devs.push_back(std::stoi(item));
        if (devs.empty())
            devs.push_back(m_world > 1 ? RankEnvironment::fromEnv().localRank % std::max(ndev, 1) : 0);
        for (int dv : devs)
            if (dv < 0 || dv >= ndev)
                throw std::invalid_argument("dynamics.devices names a device that does not exist");
    }
    // ghost depth: (v k, v k - 1) for k passes of the v-iterations-per-pass kernel between two exchanges
    const int v = NSDG_MEVP_DEFAULT_VARIANT; // the library's default kernel: sub-iterations per pass
    int k = world > 1 ? std::max(1, std::min(passesPerExchange, (nyf / world) / 16)) : 1;
    // (the brittle sub-cycle runs one sub-iteration per pass and exchanges after each: (1, 1))
    const int depthBelow = world > 1 ? (m_brittle ? 1 : v * k) : 0, depthAbove = world > 1 ? (m_brittle ? 1 : v * k - 1) : 0;
    if (world > 1 && nyf < world * 2 * std::max(depthBelow, 1))
        throw std::invalid_argument("too few element rows per block for the ghost depth");
    m_blocks.clear();
    const long group = g_localGroup++;
    std::vector<int> ranks;
    if (m_world > 1)
        ranks.push_back(m_rank);
    else if (loop)
        ranks.push_back(loopbackWorld / 2);
    else
        for (int r = 0; r < world; ++r)
            ranks.push_back(r);
    for (std::size_t i = 0; i < ranks.size(); ++i) {
        auto b = std::make_unique<DynamicsBlock>();
        b->rank = ranks[i], b->world = world, b->device = devs[i % devs.size()];
        b->nx = nxf, b->nyGlobal = nyf;
        splitRows(nyf, world, b->rank, b->r0, b->r1);
        b->depthBelow = depthBelow, b->depthAbove = depthAbove;
        const bool below = b->rank > 0, above = b->rank < world - 1;
        b->lo = b->r0 - (below ? depthBelow : 0), b->hi = b->r1 + (above ? depthAbove : 0);
        b->ny = b->hi - b->lo;
        b->j0 = b->r0 - b->lo, b->j1 = b->r1 - b->lo;
        b->peerBelow = below ? (loop ? 0 : b->rank - 1) : -1;
        b->peerAbove = above ? (loop ? 0 : b->rank + 1) : -1;
        m_blocks.push_back(std::move(b));
    }
    // the RCCL communicator id travels before anything else (multi-process run)
    unsigned char commId[NSDG_COMM_ID_BYTES];
    std::memset(commId, 0, sizeof commId);
    if (m_world > 1 || loop) {
        if (m_rank == 0)
            check(nsdg_comm_unique_id(commId), "nsdg_comm_unique_id");
        if (m_world > 1)
            broadcastFromRankZero(RankEnvironment::fromEnv(), commId, sizeof commId);
    }

    const double hx = L / nxf, hy = L / nyf;
    forEachBlock([&](DynamicsBlock& b) {
        checkHip(hipSetDevice(b.device), "hipSetDevice");
        check(nsdg_ctx_create(b.device, nullptr, &b.ctx), "nsdg_ctx_create");
        if (phaseTiming)
            check(nsdg_phase_timing_set(b.ctx, 1), "nsdg_phase_timing_set");
        if (world > 1) {
            if (m_world > 1)
                check(nsdg_comm_init(b.ctx, m_rank, m_world, commId), "nsdg_comm_init");
            else if (loop)
                check(nsdg_comm_init(b.ctx, 0, 1, commId), "nsdg_comm_init (loopback)");
            else
                check(nsdg_comm_init_local(b.ctx, group, b.rank, b.world), "nsdg_comm_init_local");
        }
        if (thermo) {
            nsdg_column_params p;
            IPhysics1d& phys = ModuleLoader::getLoader().getImplementation<IPhysics1d>();
            phys.describe(p);
            check(nsdg_column_params_set(b.ctx, &p), "nsdg_column_params_set");
        }
        b.N = (long)b.nx * b.ny;
        b.NN = (long)(2 * b.nx + 1) * (2 * b.ny + 1);
        const long N = b.N, NN = b.NN;
        const long TS = nsdg_tiled_len(b.nx, b.ny, 8), TP = nsdg_tiled_len(b.nx, b.ny, 9);
        b.nfields = 0;
        for (int k = 0; k < NFIELD; ++k) {
            const AdvectedField::When w = ADVECTED[k].when;
            const bool in = w == AdvectedField::ALWAYS || (w == AdvectedField::BRITTLE && m_brittle) || (w == AdvectedField::COLUMN_STATE && advectColumn);
            b.slot[k] = in ? b.nfields++ : -1;
        }
        // [6][ny][nx] unless set below: VXDG, VYDG and, after the arrays of Arr, the three buffers of every advected field (DynamicsBlock::adv)
        std::vector<long> sizes(NARR + 3 * b.nfields, 6 * N);
        for (int a : { S11a, S12a, S22a, S11b, S12b, S22b })
            sizes[a] = TS;
        sizes[PG] = TP;
        sizes[UNX] = 3L * (b.nx + 1) * b.ny, sizes[UNY] = 3L * b.nx * (b.ny + 1);
        for (int a : { Ua, Va, Ub, Vb, UA, VA, UO, VO })
            sizes[a] = NN;
        sizes[PACKED] = 8 * NN;
        sizes[COL] = (long)NCOL * N;
        for (int a : { HG, EG, PM })
            sizes[a] = m_brittle ? TP : 0;
        sizes[ZERO] = m_brittle ? NN : 0;
        long total = 0;
        for (long s : sizes)
            total += (s + 1) & ~1L; // keep every sub-array 16-byte aligned
        checkHip(hipMalloc(reinterpret_cast<void**>(&b.block), total * sizeof(double)), "DynamicsStep: hipMalloc");
        checkHip(hipMemset(b.block, 0, total * sizeof(double)), "DynamicsStep: hipMemset");
        b.d.clear();
        long off = 0;
        for (long s : sizes) {
            b.d.push_back(b.block + off);
            off += (s + 1) & ~1L;
        }
        check(nsdg_grid_set(b.ctx, b.nx, b.ny, hx, hy), "nsdg_grid_set");
        check(nsdg_block_set(b.ctx, b.lo, b.nyGlobal), "nsdg_block_set");
        if (m_landMask) { // the block's rows of the mask, ghost rows included: the mask is static, nothing is ever exchanged
            checkHip(hipMalloc(reinterpret_cast<void**>(&b.land), (std::size_t)N), "DynamicsStep: hipMalloc (land mask)");
            checkHip(hipMemcpy(b.land, m_landMask->data() + (std::size_t)b.lo * b.nx, (std::size_t)N, hipMemcpyHostToDevice), "upload land mask");
            check(nsdg_land_mask_set(b.ctx, b.land), "nsdg_land_mask_set");
        }
        // cell means -> DG coefficient 0 (the local rows, ghost rows included, are one contiguous slice)
        const std::size_t first = (std::size_t)b.lo * b.nx, NG = (std::size_t)nxf * nyf;
        // a restart: the state a dynamics run left (FieldStore::dyn) -- higher DG2 coefficients, velocity, stress -- for the local
        // rows, ghost rows included (they hold what an exchange would deliver: the neighbours' own values)
        const DynamicsState& dy = f.dyn;
        for (int k = 0; k < NFIELD; ++k) {
            const AdvectedField& a = ADVECTED[k];
            if (b.slot[k] < 0 || !a.stored())
                continue;
            if (a.full) { // six planes of one host array; a file without it: the field starts at zero
                if (dy.present && (dy.*a.full).size() == 6 * NG)
                    for (int c = 0; c < 6; ++c)
                        checkHip(hipMemcpy(b.adv(k, 0) + (long)c * N, (dy.*a.full).data() + (std::size_t)c * NG + first, N * sizeof(double), hipMemcpyHostToDevice), "upload DG coefficients");
                else if (dy.present && &b == m_blocks[0].get() && m_rank == 0)
                    std::printf("dynamics rheology bbm: the initial state holds no damage, the run starts undamaged (D = 0)\n");
                continue;
            }
            checkHip(hipMemcpy(b.adv(k, 0), (f.*a.mean).data() + first, N * sizeof(double), hipMemcpyHostToDevice), "upload cell means");
            if (!dy.present || (dy.*a.higher).size() != 5 * NG) // (a file without hsnow_dg: the higher coefficients of the snow start at zero)
                continue;
            for (int c = 1; c < 6; ++c)
                checkHip(hipMemcpy(b.adv(k, 0) + (long)c * N, (dy.*a.higher).data() + (std::size_t)(c - 1) * NG + first, N * sizeof(double), hipMemcpyHostToDevice), "upload DG coefficients");
        }
        if (dy.present) {
            const std::size_t nn = 2 * (std::size_t)b.nx + 1, nfirst = 2 * (std::size_t)b.lo * nn;
            checkHip(hipMemcpy(b.d[Ua], dy.u.data() + nfirst, NN * sizeof(double), hipMemcpyHostToDevice), "upload u");
            checkHip(hipMemcpy(b.d[Va], dy.v.data() + nfirst, NN * sizeof(double), hipMemcpyHostToDevice), "upload v");
            std::vector<double> t((std::size_t)TS, 0.);
            for (int k = 0; k < 3; ++k) {
                tileRows((dy.*STRESS[k]).data(), NG, (std::size_t)b.lo, b.nx, b.ny, t);
                checkHip(hipMemcpy(b.d[S11a + k], t.data(), (std::size_t)TS * sizeof(double), hipMemcpyHostToDevice), "upload stress");
            }
        }
        // analytic box-test forcing, evaluated on the device (ocean once, wind at the current model time every step); a forcing file's
        // wind and ocean pairs replace it at every step
        check(nsdg_boxtest_forcing(b.ctx, L, m_time, b.d[UA], b.d[VA], b.d[UO], b.d[VO]), "nsdg_boxtest_forcing");
        if (m_forcingFile) {
            const std::size_t n = 2 * m_forcingFile->variables().size() * (std::size_t)m_forcingFile->nxr() * m_forcingFile->nyr();
            checkHip(hipMalloc(reinterpret_cast<void**>(&b.records), n * sizeof(double)), "DynamicsStep: hipMalloc (forcing records)");
            b.recordOf[0] = b.recordOf[1] = -1;
        }
        if (thermo) {
            const std::vector<double>* planes[NCOL] = { &f.hsnow, &f.tice, &f.sst, &f.sss, &f.tair, &f.tdew, &f.slp, &f.qsw, &f.qlw, &f.mld,
                &f.snowfall, &f.wind, &f.newice };
            for (int c = 0; c < NCOL; ++c)
                checkHip(hipMemcpy(b.col(c), planes[c]->data() + first, N * sizeof(double), hipMemcpyHostToDevice), "upload column fields");
        }
        if (m_landMask) { // no ice on land, no motion at land nodes, whatever the initial state or the restart file held there
            for (int k = 0; k < NFIELD; ++k)
                if (b.slot[k] >= 0 && ADVECTED[k].stored())
                    check(nsdg_land_clear(b.ctx, 0, b.ny, 6, b.adv(k, 0)), "nsdg_land_clear");
            if (thermo) {
                check(nsdg_land_clear(b.ctx, 0, b.ny, 1, b.col(C_HSNOW)), "nsdg_land_clear");
                check(nsdg_land_clear(b.ctx, 0, b.ny, 1, b.col(C_NEWICE)), "nsdg_land_clear");
            }
            check(nsdg_land_clear_nodes(b.ctx, b.d[Ua], b.d[Va]), "nsdg_land_clear_nodes");
        }
        if (m_history) { // one plane of the owned rows per output field; the first sample of a window stores: no memset
            const std::size_t n = m_history->config().ids.size() * (std::size_t)(b.j1 - b.j0) * b.nx;
            checkHip(hipMalloc(reinterpret_cast<void**>(&b.hist), n * sizeof(double)), "DynamicsStep: hipMalloc (history accumulator)");
            if (m_history->config().weighted())
                checkHip(hipMalloc(reinterpret_cast<void**>(&b.histWeight), (std::size_t)(b.j1 - b.j0) * b.nx * sizeof(double)),
                    "DynamicsStep: hipMalloc (history weights)");
        }
        if (m_series) // every slot is written before it is read: no memset
            checkHip(hipMalloc(reinterpret_cast<void**>(&b.series),
                         (std::size_t)m_series->config().buffer * m_series->config().ids.size() * (b.j1 - b.j0) * sizeof(double)),
                "DynamicsStep: hipMalloc (series buffer)");
        if (m_drifters && !m_drifterStart.empty()) { // every block holds the whole list; the partner is written before it is read
            const std::size_t bytes = m_drifterStart.size() * sizeof(double);
            for (double*& p : b.drift)
                checkHip(hipMalloc(reinterpret_cast<void**>(&p), bytes), "DynamicsStep: hipMalloc (drifters)");
            checkHip(hipMemcpy(b.drift[0], m_drifterStart.data(), bytes, hipMemcpyHostToDevice), "upload drifters");
            b.dpar = 0;
            if (const std::size_t nf = m_drifters->config().fieldIds.size()) { // written by the first step before anything reads it
                checkHip(hipMalloc(reinterpret_cast<void**>(&b.driftSamples), nf * (m_drifterStart.size() / 3) * sizeof(double)),
                    "DynamicsStep: hipMalloc (drifter samples)");
            }
        }
        if (m_stations && !m_stationXY.empty()) { // every slot is written before it is read: no memset
            const std::size_t n = m_stationXY.size() / 2;
            checkHip(hipMalloc(reinterpret_cast<void**>(&b.stationXY), 2 * n * sizeof(double)), "DynamicsStep: hipMalloc (stations)");
            checkHip(hipMemcpy(b.stationXY, m_stationXY.data(), 2 * n * sizeof(double), hipMemcpyHostToDevice), "upload stations");
            checkHip(hipMalloc(reinterpret_cast<void**>(&b.stations),
                         (std::size_t)m_stations->config().buffer * m_stations->config().ids.size() * n * sizeof(double)),
                "DynamicsStep: hipMalloc (station buffer)");
        }
        // driver plans
        nsdg_rb_mevp_desc m;
        std::memset(&m, 0, sizeof m);
        m.nx = b.nx, m.ny = b.ny, m.j0 = b.j0, m.j1 = b.j1, m.depth_below = b.depthBelow, m.depth_above = b.depthAbove;
        m.rank_below = b.peerBelow, m.rank_above = b.peerAbove;
        m.nsub = nsub, m.overlap = overlap, m.use_graph = graph;
        m.s11[0] = b.d[S11a], m.s12[0] = b.d[S12a], m.s22[0] = b.d[S22a], m.u[0] = b.d[Ua], m.v[0] = b.d[Va];
        m.s11[1] = b.d[S11b], m.s12[1] = b.d[S12b], m.s22[1] = b.d[S22b], m.u[1] = b.d[Ub], m.v[1] = b.d[Vb];
        m.packed = b.d[PACKED], m.pg = b.d[PG];
        if (m_brittle) // the brittle plan is made when the sub-iteration count of the step is known (subStep)
            check(nsdg_bbm_params_set(b.ctx, &m_brittle->params), "nsdg_bbm_params_set");
        else
            check(nsdg_rb_mevp_create(b.ctx, &m, &b.mevp), "nsdg_rb_mevp_create");
        nsdg_rb_transport_desc t;
        std::memset(&t, 0, sizeof t);
        t.nx = b.nx, t.ny = b.ny, t.j0 = b.j0, t.j1 = b.j1, t.depth_below = b.depthBelow, t.depth_above = b.depthAbove;
        t.rank_below = b.peerBelow, t.rank_above = b.peerAbove;
        t.order = 2, t.nfields = b.nfields;
        t.vx_dg = b.d[VXDG], t.vy_dg = b.d[VYDG], t.un_x = b.d[UNX], t.un_y = b.d[UNY];
        t.own_bounds = 1, t.nbounds = closure ? t.nfields : 0; // the closure travels with the plan (its own bounds, not the context's)
        for (int k = 0; k < NFIELD; ++k)
            if (const int at = b.slot[k]; at >= 0)
                t.phi[at] = b.adv(k, 0), t.t1[at] = b.adv(k, 1), t.t2[at] = b.adv(k, 2), t.bounds[at] = ADVECTED[k].bounds;
        check(nsdg_rb_transport_create(b.ctx, &t, &b.transport), "nsdg_rb_transport_create");
        b.par = b.tpar = 0;
    });
}

void DynamicsStep::iterate(const Iterator::Duration& dtSeconds)
{
    ScopedTimer timer("iterate");
    if (phaseTiming && m_iteratePath.empty())
        m_iteratePath = Timer::main.currentPath(); // where resolvePhaseTimes() hangs the phases
    if (m_blocks.empty())
        start(0);
    const double dt = dtSeconds;
    int n = substeps;
    if (n == 0) { // auto: from the state at the start of the model step, the same n on every block
        nsdg_mevp_params p;
        nsdg_mevp_default_params(&p);
        forEachBlock([&](DynamicsBlock& b) {
            checkHip(hipSetDevice(b.device), "hipSetDevice");
            check(nsdg_phase_mark(b.ctx, NSDG_PHASE_REDUCTION), "nsdg_phase_mark"); // (the marks do nothing unless model.phase_timing is on)
            check(nsdg_concentration_max(b.ctx, b.j0, b.j1, b.cur(FH), b.cur(FA), &b.amax), "nsdg_concentration_max");
        });
        double amax = 0.; // the blocks of this process are its threads: their maximum is taken here ...
        for (auto& b : m_blocks)
            amax = std::max(amax, b->amax);
        if (m_world > 1) // ... and the processes' through the communicator
            check(nsdg_comm_max_f64(m_blocks[0]->ctx, &amax), "nsdg_comm_max_f64");
        double c = 0.;
        int32_t k = 0;
        check(nsdg_substep_count(&p, amax, std::min(L / nxf, L / nyf), dt, substepCourant, maxSubsteps, &k, &c), "dynamics.substeps = auto");
        n = k;
        if (timing && n != m_lastSubsteps && m_rank == 0)
            std::printf("dynamics substeps: t=%.17g s n=%d amax=%.17g c=%.17g m/s\n", m_time, n, amax, c);
        m_lastSubsteps = n;
    }
    const double sub = dt / n;
    for (int k = 0; k < n; ++k) {
        subStep(sub, k + 1 == n);
        m_time += sub;
    }
    m_substepsRun += n;
    ++m_steps;
    if (m_series)
        sampleSeries((long)dtSeconds);
    if (m_history)
        sampleHistory((long)dtSeconds);
    if (m_stations)
        sampleStations((long)dtSeconds);
    if (m_drifters && m_drifters->step((long)dtSeconds))
        writeDrifters();
}

void DynamicsStep::writeDrifters()
{
    // every block holds the same list after the merge: row block 0 writes
    std::vector<double> planes(m_drifterStart.size()), samples(m_drifters->config().fieldIds.size() * (m_drifterStart.size() / 3));
    if (!planes.empty()) {
        DynamicsBlock& b = *m_blocks[0];
        checkHip(hipSetDevice(b.device), "hipSetDevice");
        check(nsdg_ctx_synchronize(b.ctx), "DynamicsStep: drifters output");
        checkHip(hipMemcpy(planes.data(), b.drift[b.dpar], planes.size() * sizeof(double), hipMemcpyDeviceToHost), "download drifters");
        if (!samples.empty()) {
            if (m_steps == 0) // nothing has sampled yet (a run of no step): the fields of the start positions are not known
                std::fill(samples.begin(), samples.end(), std::numeric_limits<double>::quiet_NaN());
            else
                checkHip(hipMemcpy(samples.data(), b.driftSamples, samples.size() * sizeof(double), hipMemcpyDeviceToHost), "download drifter samples");
        }
    }
    m_drifters->write(planes, samples);
}

// what a history sample and the row totals read: the current side of every ping-pong
static nsdg_history_sources historySources(const DynamicsBlock& b, bool thermo, bool advectColumn)
{ // (D: the current damage of a brittle run)
    nsdg_history_sources src;
    std::memset(&src, 0, sizeof src);
    src.H = b.cur(FH), src.A = b.cur(FA), src.u = b.curU(), src.v = b.curV();
    const int s = b.par == 0 ? S11a : S11b;
    src.s11 = b.d[s], src.s12 = b.d[s + 1], src.s22 = b.d[s + 2];
    if (thermo) // the snow plane the column step actually uses: plane 0 of S under dynamics.advect_column_state
        src.hsnow = advectColumn ? b.cur(FS) : b.col(C_HSNOW), src.tice = b.col(C_TICE);
    if (b.slot[FD] >= 0)
        src.D = b.cur(FD);
    return src;
}

void DynamicsStep::sampleHistory(long dt)
{
    // after the NSDG_PHASE_END mark of the step: the sample belongs to no phase, and it is never part of a captured graph
    const HistoryOutput::Action a = m_history->step(dt);
    if (a.sample) {
        const HistoryOutput::Config& c = m_history->config();
        const std::vector<int>& ids = c.ids;
        const bool stats = c.hasStats(); // bare names: the plain call, as ever
        forEachBlock([&](DynamicsBlock& b) {
            checkHip(hipSetDevice(b.device), "hipSetDevice");
            const nsdg_history_sources src = historySources(b, thermo, advectColumn);
            const int64_t stride = (int64_t)(b.j1 - b.j0) * b.nx;
            if (stats)
                check(nsdg_history_accumulate_stats(b.ctx, b.j0, b.j1, (int32_t)ids.size(), ids.data(), c.stats.data(), &src, a.store ? 1 : 0, b.j0, stride,
                          b.hist, b.histWeight),
                    "nsdg_history_accumulate_stats");
            else
                check(nsdg_history_accumulate(b.ctx, b.j0, b.j1, (int32_t)ids.size(), ids.data(), &src, a.store ? 1 : 0, b.j0, stride, b.hist),
                    "nsdg_history_accumulate");
        });
    }
    if (a.flush)
        flushHistory();
}

void DynamicsStep::sampleSeries(long dt)
{
    // like the history sample: after the step's last phase mark, outside every captured graph; the host counts the slots
    const std::vector<int>& ids = m_series->config().ids;
    const std::size_t slot = m_series->step(dt);
    forEachBlock([&](DynamicsBlock& b) {
        checkHip(hipSetDevice(b.device), "hipSetDevice");
        const nsdg_history_sources src = historySources(b, thermo, advectColumn);
        const int64_t rows = b.j1 - b.j0;
        check(nsdg_history_row_totals(b.ctx, b.j0, b.j1, (int32_t)ids.size(), ids.data(), &src, SeriesOutput::EXTENT_CONC, b.j0, rows,
                  b.series + slot * ids.size() * rows),
            "nsdg_history_row_totals");
    });
    if (m_series->full())
        flushSeries();
}

void DynamicsStep::sampleStations(long dt)
{
    // like the history sample: after the step's last phase mark, outside every captured graph; the host counts the slots
    const std::vector<int>& ids = m_stations->config().ids;
    const std::size_t slot = m_stations->step(dt);
    const int64_t n = (int64_t)(m_stationXY.size() / 2);
    if (n > 0)
        forEachBlock([&](DynamicsBlock& b) {
            checkHip(hipSetDevice(b.device), "hipSetDevice");
            const nsdg_history_sources src = historySources(b, thermo, advectColumn);
            check(nsdg_points_sample(b.ctx, b.j0, b.j1, 2, n, b.stationXY, b.stationXY + n, (int32_t)ids.size(), ids.data(), &src, n,
                      b.stations + slot * ids.size() * n),
                "nsdg_points_sample");
        });
    if (m_stations->full())
        flushStations();
}

void DynamicsStep::flushStations()
{
    const std::size_t count = m_stations->pending().size(), nf = m_stations->config().ids.size(), n = m_stationXY.size() / 2;
    if (count == 0) // (a second stop())
        return;
    ScopedTimer timer("stations flush");
    // a station belongs to the block whose rows hold its element; the others hold -inf: the maximum over the blocks is the table
    std::vector<double> table(count * nf * n, -std::numeric_limits<double>::infinity()), part(table.size());
    if (!table.empty())
        for (auto& bp : m_blocks) {
            DynamicsBlock& b = *bp;
            checkHip(hipSetDevice(b.device), "hipSetDevice");
            check(nsdg_ctx_synchronize(b.ctx), "DynamicsStep: stations flush");
            checkHip(hipMemcpy(part.data(), b.stations, part.size() * sizeof(double), hipMemcpyDeviceToHost), "download stations");
            for (std::size_t i = 0; i < table.size(); ++i)
                table[i] = (part[i] > table[i] || part[i] != part[i]) ? part[i] : table[i]; // (a NaN sample is kept)
        }
    m_stations->write(m_stationXY, table);
}

void DynamicsStep::flushSeries()
{
    const SeriesOutput::Config& c = m_series->config();
    const std::size_t count = m_series->pending().size(), nq = c.ids.size();
    if (count == 0) // (a second stop())
        return;
    ScopedTimer timer("series flush");
    int row0 = m_blocks[0]->r0, row1 = m_blocks[0]->r1;
    for (auto& bp : m_blocks)
        row0 = std::min(row0, bp->r0), row1 = std::max(row1, bp->r1);
    const std::size_t nrows = (std::size_t)(row1 - row0);
    std::vector<double> rows(count * nq * nrows), part;
    for (auto& bp : m_blocks) { // sequential: the blocks fill disjoint row ranges
        DynamicsBlock& b = *bp;
        checkHip(hipSetDevice(b.device), "hipSetDevice");
        check(nsdg_ctx_synchronize(b.ctx), "DynamicsStep: series flush");
        const std::size_t own = (std::size_t)(b.r1 - b.r0);
        part.resize(count * nq * own);
        checkHip(hipMemcpy(part.data(), b.series, part.size() * sizeof(double), hipMemcpyDeviceToHost), "download series");
        for (std::size_t s = 0; s < count * nq; ++s)
            std::copy(part.begin() + s * own, part.begin() + (s + 1) * own, rows.begin() + s * nrows + (b.r0 - row0));
    }
    std::vector<std::string> lines;
    for (std::size_t s = 0; s < count; ++s)
        lines.push_back(SeriesOutput::formatLine(m_series->pending()[s], SeriesOutput::totals(c.ids, rows.data() + s * nq * nrows, nrows, L / nxf, L / nyf)));
    SeriesOutput::append(c, lines);
    m_series->flushed();
}

void DynamicsStep::flushHistory()
{
    // the window ends: the owned rows of every block of this process into ONE host array, divided by the count, one record file
    const long samples = m_history->samples();
    if (samples > 0) {
        ScopedTimer timer("history flush");
        const HistoryOutput::Config& c = m_history->config();
        int row0 = m_blocks[0]->r0, row1 = m_blocks[0]->r1;
        for (auto& bp : m_blocks)
            row0 = std::min(row0, bp->r0), row1 = std::max(row1, bp->r1);
        HistoryOutput::Record r;
        r.timeStart = m_history->windowStart(), r.timeEnd = m_history->windowEnd(), r.samples = samples;
        r.kind = c.snapshot ? "snapshot" : "mean";
        r.fields = c.fields;
        r.x = nyf, r.y = nxf, r.row0 = row0, r.rows = row1 - row0;
        const std::size_t plane = (std::size_t)r.rows * nxf;
        r.data.assign(c.fields.size() * plane, 0.);
        for (auto& bp : m_blocks) { // sequential: the blocks fill disjoint row ranges
            DynamicsBlock& b = *bp;
            checkHip(hipSetDevice(b.device), "hipSetDevice");
            check(nsdg_ctx_synchronize(b.ctx), "DynamicsStep: history flush");
            const std::size_t count = (std::size_t)(b.r1 - b.r0) * b.nx;
            for (std::size_t k = 0; k < c.fields.size(); ++k)
                checkHip(hipMemcpy(r.data.data() + k * plane + (std::size_t)(b.r0 - row0) * b.nx, b.hist + k * count, count * sizeof(double), hipMemcpyDeviceToHost),
                    "download history");
        }
        std::vector<double> weights;
        if (c.weighted()) { // the summed weights of the ice-weighted means, the same rows
            weights.assign(plane, 0.);
            for (auto& bp : m_blocks) {
                DynamicsBlock& b = *bp;
                checkHip(hipSetDevice(b.device), "hipSetDevice");
                checkHip(hipMemcpy(weights.data() + (std::size_t)(b.r0 - row0) * b.nx, b.histWeight, (std::size_t)(b.r1 - b.r0) * b.nx * sizeof(double),
                             hipMemcpyDeviceToHost),
                    "download history weights");
            }
        }
        HistoryOutput::finish(c.stats, samples, plane, weights.empty() ? nullptr : weights.data(), r.data);
        HistoryOutput::write(HistoryOutput::recordPath(c.file, r.timeEnd, m_rank, m_world), c.file, r);
    }
    m_history->closeWindow();
}

void DynamicsStep::subStep(double dt, bool last)
{
    nsdg_mevp_params p;
    nsdg_mevp_default_params(&p);
    if (!m_brittle) { // (the brittle pass ignores alpha, beta and the adaptive constants)
        const SubcycleChoice sc = subcycleChoice(std::min(L / nxf, L / nyf), dt);
        p.alpha = sc.alpha, p.beta = sc.beta, p.delta_min = sc.deltaMin, p.aevp_c = sc.aevpC, p.aevp_alpha_min = sc.aevpAlphaMin;
    }
    p.min_conc = closure ? minConc : 0.;
    p.min_thick = closure ? minThick : 0.;
    // the sub-iterations of a brittle (sub-)step: dynamics.nsub as given, or the elastic-wave rule for this dt
    int bsub = nsub;
    if (m_brittle) {
        int32_t need = 0;
        check(nsdg_bbm_substep_count(&m_brittle->params, p.rho_ice, std::min(L / nxf, L / nyf), dt, m_brittle->courant, 100000000, &need), "dynamics.bbm_courant");
        if (!nsubGiven)
            bsub = need;
        else if (nsub < need && !m_brittle->warned && m_rank == 0) {
            std::printf("dynamics rheology bbm: WARNING dynamics.nsub = %d is below the %d sub-iterations the elastic-wave rule asks for at dt = %g s "
                        "(dynamics.bbm_courant = %g)\n", nsub, (int)need, dt, m_brittle->courant);
            m_brittle->warned = true;
        }
    }
    const double t = m_time;
    const int kind = forcing == "winter" ? NSDG_FORCING_WINTER : NSDG_FORCING_DUMMY;
    const ForcingFile* ff = m_forcingFile.get();
    std::size_t k0 = 0, k1 = 0;
    double w = 0.;
    if (ff)
        ff->bracket(t, k0, k1, w); // the records around the model time (throws outside the file's time range)
    forEachBlock([&](DynamicsBlock& b) {
        checkHip(hipSetDevice(b.device), "hipSetDevice");
        nsdg_ctx* ctx = b.ctx;
        check(nsdg_mevp_params_set(ctx, &p), "nsdg_mevp_params_set");
        check(nsdg_phase_mark(ctx, NSDG_PHASE_FORCING), "nsdg_phase_mark");
        if (!ff || !ff->hasWind())
            check(nsdg_boxtest_forcing(ctx, L, t, b.d[UA], b.d[VA], nullptr, nullptr), "nsdg_boxtest_forcing"); // the cyclone moves
        if (ff)
            sampleForcingFile(b, k0, k1, w);
        if (thermo) {
            if (forcing != "host") { // DummyExternalData's replacement, and the wind speed the reference never sets
                if (!ff)
                    check(nsdg_column_forcing(ctx, kind, t, b.col(C_TAIR), b.col(C_TDEW), b.col(C_SLP), b.col(C_QSW), b.col(C_QLW), b.col(C_MLD),
                              b.col(C_SNOWFALL)),
                        "nsdg_column_forcing");
                check(nsdg_column_wind(ctx, b.d[UA], b.d[VA], b.col(C_WIND)), "nsdg_column_wind");
            }
            check(nsdg_phase_mark(ctx, NSDG_PHASE_COLUMN), "nsdg_phase_mark");
            // the column physics needs no exchange: it runs on the ghost rows too, redundantly
            check(nsdg_column_step(ctx, b.N, dt, b.cur(FH), b.cur(FA), advectColumn ? b.cur(FS) : b.col(C_HSNOW), b.col(C_TICE), b.col(C_SST), b.col(C_SSS), b.col(C_TAIR),
                      b.col(C_TDEW), b.col(C_SLP), b.col(C_QSW), b.col(C_QLW), b.col(C_MLD), b.col(C_SNOWFALL), b.col(C_WIND), b.col(C_NEWICE),
                      nullptr),
                "nsdg_column_step");
            if (b.land) {
                // the column step computes on land elements too and its result there is discarded: the cell means of H, A (and S), the
                // snow and the new ice (still the column phase)
                for (double* plane : { b.cur(FH), b.cur(FA), advectColumn ? b.cur(FS) : b.col(C_HSNOW), b.col(C_NEWICE) })
                    check(nsdg_land_clear(ctx, 0, b.ny, 1, plane), "nsdg_land_clear");
                if (m_brittle) // and the damage with them
                    check(nsdg_land_clear(ctx, 0, b.ny, 6, b.cur(FD)), "nsdg_land_clear");
            }
        }
        check(nsdg_phase_mark(ctx, NSDG_PHASE_PREPARE), "nsdg_phase_mark");
        int32_t out = 0;
        if (m_brittle) {
            // the Gauss arrays of the brittle sub-cycle and the mEVP packing for the sub-iteration's dt with u0 = v0 = 0: no ice strength
            check(nsdg_bbm_prepare(ctx, 0, b.ny, b.cur(FH), b.cur(FA), b.d[HG], b.d[EG], b.d[PM]), "nsdg_bbm_prepare");
            check(nsdg_mevp_prepare(ctx, bsub > 0 ? dt / bsub : dt, b.cur(FH), b.cur(FA), b.d[UA], b.d[VA], b.d[UO], b.d[VO], b.d[ZERO], b.d[ZERO], b.d[PACKED]),
                "nsdg_mevp_prepare");
            if (!b.bbm || b.bbmNsub != bsub) { // the plan holds the count: a new one when the rule gives another (another dt)
                check(nsdg_ctx_synchronize(ctx), "DynamicsStep: brittle plan");
                nsdg_rb_bbm_destroy(b.bbm);
                b.bbm = nullptr;
                nsdg_rb_bbm_desc m;
                std::memset(&m, 0, sizeof m);
                m.nx = b.nx, m.ny = b.ny, m.j0 = b.j0, m.j1 = b.j1, m.depth_below = b.depthBelow, m.depth_above = b.depthAbove;
                m.rank_below = b.peerBelow, m.rank_above = b.peerAbove;
                m.nsub = bsub, m.overlap = overlap;
                m.complete_nodes = b.drift[0] != nullptr; // the drifters' predictor may sit in the ghost row above
                m.s11[0] = b.d[S11a], m.s12[0] = b.d[S12a], m.s22[0] = b.d[S22a], m.u[0] = b.d[Ua], m.v[0] = b.d[Va];
                m.s11[1] = b.d[S11b], m.s12[1] = b.d[S12b], m.s22[1] = b.d[S22b], m.u[1] = b.d[Ub], m.v[1] = b.d[Vb];
                m.packed = b.d[PACKED], m.hg = b.d[HG], m.eg = b.d[EG], m.pm = b.d[PM];
                // the transport's two buffers of D, and its stage buffer of D -- free between two transport steps -- as the partner
                m.D[0] = b.adv(FD, 0), m.D[1] = b.adv(FD, 1), m.D_work = b.adv(FD, 2);
                check(nsdg_rb_bbm_create(ctx, &m, &b.bbm), "nsdg_rb_bbm_create");
                b.bbmNsub = bsub;
            }
            check(nsdg_phase_mark(ctx, NSDG_PHASE_SUBCYCLE), "nsdg_phase_mark");
            check(nsdg_rb_bbm_run(ctx, b.bbm, b.par, b.tpar, &out), "nsdg_rb_bbm_run");
        } else {
            check(nsdg_ice_strength(ctx, 0, b.ny, b.cur(FH), b.cur(FA), b.d[PG]), "nsdg_ice_strength");
            check(nsdg_mevp_prepare(ctx, dt, b.cur(FH), b.cur(FA), b.d[UA], b.d[VA], b.d[UO], b.d[VO], b.curU(), b.curV(), b.d[PACKED]), "nsdg_mevp_prepare");
            check(nsdg_phase_mark(ctx, NSDG_PHASE_SUBCYCLE), "nsdg_phase_mark");
            check(nsdg_rb_mevp_run(ctx, b.mevp, b.par, &out), "nsdg_rb_mevp_run");
        }
        b.par = out;
        check(nsdg_phase_mark(ctx, NSDG_PHASE_TRANSPORT), "nsdg_phase_mark");
        check(nsdg_prepare_advection(ctx, 2, b.curU(), b.curV(), b.d[VXDG], b.d[VYDG], b.d[UNX], b.d[UNY]), "nsdg_prepare_advection");
        // the surface temperature travels as Q = H tice0 (every local row: element-local, the ghost rows stay equal to their owners)
        if (advectColumn)
            check(nsdg_tracer_weight(ctx, 2, 0, b.ny, b.cur(FH), b.col(C_TICE), b.cur(FQ)), "nsdg_tracer_weight");
        check(nsdg_rb_transport_run(ctx, b.transport, dt, b.tpar, &out), "nsdg_rb_transport_run");
        b.tpar = out;
        if (advectColumn)
            check(nsdg_tracer_recover(ctx, 2, 0, b.ny, b.cur(FH), b.cur(FA), b.cur(FQ), p.min_conc, p.min_thick, b.col(C_TICE)), "nsdg_tracer_recover");
        if (b.drift[0]) {
            // the drifters of the owned rows move with the velocity the sub-cycle left (its ghost node rows are complete: the mEVP plan's
            // ghost zones are (v k, v k - 1) deep, the brittle plan ends with the exchange of every node row: complete_nodes) and the concentration the transport left; then the blocks' lists are merged.  No phase of
            // its own: inside the span, before its end mark
            const int64_t n = (int64_t)(m_drifterStart.size() / 3);
            check(nsdg_drifters_advance(ctx, b.j0, b.j1, dt, m_drifters->config().minConc, n, b.curU(), b.curV(), b.cur(FA), b.drift[b.dpar], b.drift[1 - b.dpar]),
                "nsdg_drifters_advance");
            b.dpar = 1 - b.dpar;
            if (b.world > 1)
                check(nsdg_comm_max_f64_array(ctx, b.drift[b.dpar], 3 * n), "nsdg_comm_max_f64_array");
            if (b.driftSamples) {
                // model.drifters_fields: the merged list is sampled at its NEW positions from the state the step left -- every block the
                // points of its own rows, -inf for the others -- and one more maximum makes the whole table
                const std::vector<int>& ids = m_drifters->config().fieldIds;
                const nsdg_history_sources src = historySources(b, thermo, advectColumn);
                check(nsdg_points_sample(ctx, b.j0, b.j1, 2, n, b.drift[b.dpar], b.drift[b.dpar] + n, (int32_t)ids.size(), ids.data(), &src, n, b.driftSamples),
                    "nsdg_points_sample");
                if (b.world > 1)
                    check(nsdg_comm_max_f64_array(ctx, b.driftSamples, (int64_t)ids.size() * n), "nsdg_comm_max_f64_array");
            }
        }
        if (last) // the model step ends here: what follows until its next mark belongs to no phase
            check(nsdg_phase_mark(ctx, NSDG_PHASE_END), "nsdg_phase_mark");
    });
}

void DynamicsStep::resolvePhaseTimes()
{
    // once, after the run: the only place where the host waits for the marks (nsdg_phase_times; stop() has drained the streams already)
    std::vector<PhaseBlockTimes> tables;
    for (auto& bp : m_blocks) {
        DynamicsBlock& b = *bp;
        checkHip(hipSetDevice(b.device), "hipSetDevice");
        PhaseBlockTimes t;
        t.block = b.rank;
        check(nsdg_phase_times(b.ctx, &t.table, 0), "nsdg_phase_times");
        t.hasExchange = b.peerBelow >= 0 || b.peerAbove >= 0;
        if (t.hasExchange) {
            if (b.bbm) // (the plan of the last sub-iteration count)
                check(nsdg_rb_bbm_stats(b.ctx, b.bbm, &t.subcycleExchange, 0), "nsdg_rb_bbm_stats");
            else if (b.mevp)
                check(nsdg_rb_mevp_stats(b.ctx, b.mevp, &t.subcycleExchange, 0), "nsdg_rb_mevp_stats");
            check(nsdg_rb_transport_stats(b.ctx, b.transport, &t.transportExchange, 0), "nsdg_rb_transport_stats");
        }
        tables.push_back(t);
    }
    if (!m_iteratePath.empty())
        PhaseTiming::toTimer(Timer::main, m_iteratePath, tables);
    const std::string path = PhaseTiming::file();
    if (!path.empty())
        PhaseTiming::write(path, m_rank, m_world, m_steps, m_substepsRun, tables);
}

void DynamicsStep::sampleForcingFile(DynamicsBlock& b, std::size_t k0, std::size_t k1, double w)
{
    const ForcingFile& ff = *m_forcingFile;
    const std::vector<std::string> vars = ff.variables();
    const std::size_t plane = (std::size_t)ff.nxr() * ff.nyr(), slot = vars.size() * plane;
    // the two records around the model time stay resident: a record is uploaded when the model time crosses into it, into a slot
    // whose record is no longer needed (after the work queued on the context, which may still read that slot)
    int at[2] = { -1, -1 };
    for (int i = 0; i < 2; ++i) {
        const long k = (long)(i == 0 ? k0 : k1);
        for (int s = 0; s < 2; ++s)
            if (b.recordOf[s] == k)
                at[i] = s;
    }
    for (int i = 0; i < 2; ++i) {
        if (at[i] >= 0)
            continue;
        const long k = (long)(i == 0 ? k0 : k1), other = (long)(i == 0 ? k1 : k0);
        const int s = b.recordOf[0] == other ? 1 : 0; // never the slot of the other record of the pair
        std::vector<double> host(slot);
        for (std::size_t v = 0; v < vars.size(); ++v)
            std::copy(ff.record(vars[v], (std::size_t)k), ff.record(vars[v], (std::size_t)k) + plane, host.begin() + v * plane);
        check(nsdg_ctx_synchronize(b.ctx), "DynamicsStep: forcing record upload");
        checkHip(hipMemcpy(b.records + s * slot, host.data(), slot * sizeof(double), hipMemcpyHostToDevice), "upload forcing record");
        b.recordOf[s] = k;
        at[i] = s;
        if (k0 == k1)
            at[1] = s;
    }
    auto rec = [&](int i, const std::string& var) -> const double* {
        std::size_t v = 0;
        while (vars[v] != var)
            ++v;
        return b.records + at[i] * slot + v * plane;
    };
    // one launch per lattice: the wind and ocean pairs at the CG2 nodes, the column planes at the element centres
    std::vector<const double*> r0, r1;
    std::vector<double*> out;
    for (const auto& pr : { std::make_pair("wind_u", UA), std::make_pair("wind_v", VA), std::make_pair("ocean_u", UO), std::make_pair("ocean_v", VO) })
        if (ff.has(pr.first)) {
            r0.push_back(rec(0, pr.first)), r1.push_back(rec(1, pr.first)), out.push_back(b.d[pr.second]);
        }
    if (!out.empty())
        check(nsdg_forcing_sample(b.ctx, NSDG_AT_NODES, ff.nxr(), ff.nyr(), (int32_t)out.size(), r0.data(), r1.data(), w, out.data()),
            "nsdg_forcing_sample (nodes)");
    if (thermo) {
        r0.clear(), r1.clear(), out.clear();
        const int planes[7] = { C_TAIR, C_TDEW, C_SLP, C_QSW, C_QLW, C_MLD, C_SNOWFALL };
        for (int c = 0; c < 7; ++c) {
            const std::string& var = ForcingFile::columnVariables()[c];
            r0.push_back(rec(0, var)), r1.push_back(rec(1, var)), out.push_back(b.col(planes[c]));
        }
        check(nsdg_forcing_sample(b.ctx, NSDG_AT_ELEMENTS, ff.nxr(), ff.nyr(), 7, r0.data(), r1.data(), w, out.data()),
            "nsdg_forcing_sample (elements)");
    }
}

void DynamicsStep::stop(const Iterator::TimePoint&)
{
    ScopedTimer timer("stop (download)");
    if (m_blocks.empty())
        return;
    if (m_history) // a run that stops inside a window writes it with the samples it has; an empty window (a second stop()) writes nothing
        flushHistory();
    if (m_series)
        flushSeries();
    if (m_stations)
        flushStations();
    if (m_drifters && m_drifters->dueAtStop()) // the block of the last time, once (stop() comes twice: the iterator's, the restart file's)
        writeDrifters();
    FieldStore& f = pStructure->fields();
    std::vector<double> umax(m_blocks.size(), 0.);
    bool finite = true;
    std::size_t idx = 0;
    for (auto& bp : m_blocks) { // sequential: the blocks write disjoint row ranges of the host structure
        DynamicsBlock& b = *bp;
        checkHip(hipSetDevice(b.device), "hipSetDevice");
        check(nsdg_ctx_synchronize(b.ctx), "DynamicsStep::stop");
        uint32_t gaveUp = 0; // bounded waits of the mEVP pipeline that hit their bound: the fields would be wrong
        check(nsdg_mevp_pipeline_health(b.ctx, &gaveUp), "nsdg_mevp_pipeline_health");
        if (gaveUp)
            throw std::runtime_error("DynamicsStep: " + std::to_string(gaveUp) + " wait(s) of the mEVP pipeline gave up: the fields are not to be trusted");
        const std::size_t first = (std::size_t)b.r0 * b.nx, count = (std::size_t)(b.r1 - b.r0) * b.nx, skip = (std::size_t)b.j0 * b.nx;
        if (thermo) {
            if (!advectColumn) // (otherwise f.hsnow receives the mean of S below: S is advected only under thermodynamics)
                checkHip(hipMemcpy(f.hsnow.data() + first, b.col(C_HSNOW) + skip, count * sizeof(double), hipMemcpyDeviceToHost), "download hsnow");
            checkHip(hipMemcpy(f.tice.data() + first, b.col(C_TICE) + skip, count * sizeof(double), hipMemcpyDeviceToHost), "download tice");
            checkHip(hipMemcpy(f.newice.data() + first, b.col(C_NEWICE) + skip, count * sizeof(double), hipMemcpyDeviceToHost), "download newice");
        }
        // owned node rows: [2 j0, 2 j1) plus the top boundary row on the last block
        const long nn = 2L * b.nx + 1;
        const long rows = 2L * (b.j1 - b.j0) + (b.peerAbove < 0 ? 1 : 0);
        // the rest of the state a restart needs (FieldStore::dyn): higher DG2 coefficients, velocity, stress of the owned rows
        DynamicsState& dy = f.dyn;
        const std::size_t NG = (std::size_t)nxf * nyf;
        if (dy.hdg.size() != 5 * NG)
            dy.resize((std::size_t)nyf, (std::size_t)nxf);
        for (int k = 0; k < NFIELD; ++k) {
            const AdvectedField& a = ADVECTED[k];
            if (!a.stored())
                continue;
            if (a.full) { // all six planes in one host array, which exists only while the field is advected
                (dy.*a.full).resize(b.slot[k] >= 0 ? 6 * NG : 0, 0.);
                for (int c = 0; c < 6 && b.slot[k] >= 0; ++c)
                    checkHip(hipMemcpy((dy.*a.full).data() + (std::size_t)c * NG + first, b.cur(k) + (long)c * b.N + skip, count * sizeof(double), hipMemcpyDeviceToHost), "download DG coefficients");
                continue;
            }
            // the higher coefficients of a field exist only while it is advected: otherwise nothing of them is written
            (dy.*a.higher).resize(b.slot[k] >= 0 ? 5 * NG : 0, 0.);
            if (b.slot[k] < 0)
                continue;
            checkHip(hipMemcpy((f.*a.mean).data() + first, b.cur(k) + skip, count * sizeof(double), hipMemcpyDeviceToHost), "download cell means");
            for (int c = 1; c < 6; ++c)
                checkHip(hipMemcpy((dy.*a.higher).data() + (std::size_t)(c - 1) * NG + first, b.cur(k) + (long)c * b.N + skip, count * sizeof(double), hipMemcpyDeviceToHost), "download DG coefficients");
        }
        checkHip(hipMemcpy(dy.u.data() + 2L * b.r0 * nn, b.curU() + 2L * b.j0 * nn, rows * nn * sizeof(double), hipMemcpyDeviceToHost), "download u");
        checkHip(hipMemcpy(dy.v.data() + 2L * b.r0 * nn, b.curV() + 2L * b.j0 * nn, rows * nn * sizeof(double), hipMemcpyDeviceToHost), "download v");
        std::vector<double> t((std::size_t)nsdg_tiled_len(b.nx, b.ny, 8));
        for (int k = 0; k < 3; ++k) {
            checkHip(hipMemcpy(t.data(), b.d[(b.par == 0 ? S11a : S11b) + k], t.size() * sizeof(double), hipMemcpyDeviceToHost), "download stress");
            untileRows(t, b.nx, b.j0, b.j1 - b.j0, (dy.*STRESS[k]).data(), NG, (std::size_t)b.r0);
        }
        for (long k = 2L * b.r0 * nn; k < (2L * b.r0 + rows) * nn; ++k) {
            umax[idx] = std::max(umax[idx], std::max(std::fabs(dy.u[k]), std::fabs(dy.v[k])));
            finite = finite && std::isfinite(dy.u[k]) && std::isfinite(dy.v[k]);
        }
        ++idx;
    }
    f.dyn.present = true;
    if (phaseTiming)
        resolvePhaseTimes();
    m_umax = *std::max_element(umax.begin(), umax.end());
    m_sumH = m_sumA = 0;
    for (auto& bp : m_blocks)
        for (long e = (long)bp->r0 * nxf; e < (long)bp->r1 * nxf; ++e) {
            m_sumH += f.hice[e];
            m_sumA += f.cice[e];
        }
    // A run that has left the physical range (profiles/r04_soak_divergence_cause.md) must fail loudly: the
    // caller gets an exception (non-zero exit of nextsim_amd) and -- because writeRestartFile() comes through here first -- no
    // restart file full of NaN is written.  (The reference never checks its fields; it also has no dynamics to go unstable.)
    if (!finite || !std::isfinite(m_sumH) || !std::isfinite(m_sumA))
        throw std::runtime_error("DynamicsStep: the run left the physical range (non-finite velocity, thickness or concentration after "
            + std::to_string(m_steps) + " steps); no restart file is written");
}

NSDG_REGISTER_MODULE(IModelStep, DynamicsStep, "Nextsim::IModelStep", "Nextsim::DynamicsStep");

void DynamicsStep::writeRestartFile(const std::string& filePath)
{
    if (!pStructure)
        throw std::logic_error("DynamicsStep::writeRestartFile: setInitialData() was not called");
    if (m_world <= 1) {
        stop(0);
        pStructure->dump(filePath);
        return;
    }
    // A rank holds only its own rows up to date: they travel to rank 0, which writes the ONE restart file (every row of it
    // current) and ACKNOWLEDGES it: no rank returns before rank 0 has written the file, and if anything fails -- a rank's
    // fields are non-finite (stop() throws), a rank has died, the write fails -- EVERY rank throws, so that a run without a
    // restart file never exits with status 0 on some of its ranks.  The waits are bounded by the communicator's deadline
    // (NSDG_COMM_TIMEOUT_S, the same variable the library and bench.py read; 0 = for ever; default 120 s here).
    const char* tv = std::getenv("NSDG_COMM_TIMEOUT_S");
    const int timeout = (tv && *tv) ? std::atoi(tv) : 120;
    const RankEnvironment env = RankEnvironment::fromEnv();
    std::exception_ptr own;
    try {
        stop(0);
    } catch (...) {
        own = std::current_exception();
    }
    if (own && m_rank != 0) {
        reportFailureToRankZero(env, std::min(timeout > 0 ? timeout : 86400, 30));
        std::rethrow_exception(own);
    }
    FieldStore& f = pStructure->fields();
    int r0, r1;
    splitRows(nyf, m_world, m_rank, r0, r1);
    const std::vector<double> mine = (m_rank == 0 || own) ? std::vector<double>() : packRows(f, thermo, nxf, r0, r1);
    gatherToRankZero(
        env, mine.data(), mine.size() * sizeof(double),
        [&](int rank, const char* data, std::size_t bytes) {
            if (own)
                return; // rank 0 itself failed: the rows are received and dropped, the senders are told below
            int a, b;
            splitRows(nyf, m_world, rank, a, b);
            placeRows(f, thermo, nxf, a, b, reinterpret_cast<const double*>(data), bytes / sizeof(double));
        },
        timeout,
        [&]() {
            if (own)
                std::rethrow_exception(own);
            pStructure->dump(filePath);
        });
}

namespace {
// What a rank sends for its rows [r0, r1), in order: fn(array, offset, length) for the rows of every prognostic plane a run changes; then,
// unless state < 0, of what DynamicsState owns of DYNAMICS_VARIABLES with the optional ones whose bit is set in `state` (bit i: the i-th
// optional variable of the table) -- the rows of every element plane, and of a nodal array the node rows the block owns: [2 r0, 2 r1) and
// the top boundary row on the last block
template <class F> void forPayload(FieldStore& f, bool thermodynamics, int nx, int r0, int r1, int state, F&& fn)
{
    const std::size_t first = (std::size_t)r0 * nx, rows = (std::size_t)(r1 - r0) * nx, nn = 2 * (std::size_t)nx + 1;
    for (auto* p : { &f.hice, &f.cice, &f.hsnow, &f.tice, &f.newice })
        if (thermodynamics || p == &f.hice || p == &f.cice) // (the column model's planes change only with it)
            fn(*p, first, rows);
    if (state < 0)
        return;
    int bit = 0;
    for (const DynamicsVariable& v : DYNAMICS_VARIABLES) {
        if (v.optional() && !((state >> bit++) & 1))
            continue;
        if (!v.state)
            continue; // a plane of the FieldStore: it has travelled above, or does not travel
        if (v.shape == DynamicsVariable::NODAL)
            fn(v.in(f), 2 * (std::size_t)r0 * nn, (2 * (std::size_t)(r1 - r0) + ((std::size_t)r1 * nx == f.n ? 1 : 0)) * nn);
        for (int c = 0; c < v.elementPlanes(); ++c)
            fn(v.in(f), (std::size_t)c * f.n + first, rows);
    }
}
} // namespace

std::vector<double> DynamicsStep::packRows(FieldStore& f, bool thermodynamics, int nx, int r0, int r1)
{
    int state = f.dyn.present ? 0 : -1, bit = 0; // the state of the dynamics travels with the rows, with the optional variables it holds
    for (const DynamicsVariable& v : DYNAMICS_VARIABLES)
        if (v.optional())
            state |= (f.dyn.present && !v.in(f).empty() ? 1 : 0) << bit++;
    std::vector<double> out;
    forPayload(f, thermodynamics, nx, r0, r1, state, [&](std::vector<double>& a, std::size_t at, std::size_t length) { out.insert(out.end(), a.begin() + at, a.begin() + at + length); });
    return out;
}

void DynamicsStep::placeRows(FieldStore& f, bool thermodynamics, int nx, int r0, int r1, const double* data, std::size_t count)
{
    // what a rank sent shows in the size alone: its planes, or also the state of the dynamics with one of the sets of its optional
    // variables (their sizes differ, and a run holds the snow or the damage, never both: the first set that fits is the one)
    const int optional = (int)std::count_if(std::begin(DYNAMICS_VARIABLES), std::end(DYNAMICS_VARIABLES), [](const DynamicsVariable& v) { return v.optional(); });
    std::string sizes;
    int state = -2; // as forPayload reads it, once found
    for (int k = -1; k < (1 << optional) && state < -1; ++k) {
        std::size_t size = 0;
        forPayload(f, thermodynamics, nx, r0, r1, k, [&](std::vector<double>&, std::size_t, std::size_t length) { size += length; });
        if (size == count)
            state = k;
        sizes += " " + std::to_string(size);
    }
    if (state < -1)
        throw std::runtime_error("DynamicsStep: a rank delivered " + std::to_string(count) + " values for its rows, expected one of" + sizes
            + " (its planes alone, with the state of the dynamics, with each set of the optional variables of that as well)");
    int bit = 0;
    for (const DynamicsVariable& v : DYNAMICS_VARIABLES) { // whatever of the delivered state nothing has filled yet starts at zero
        const bool sent = !v.optional() || (state >= 0 && ((state >> bit) & 1));
        bit += v.optional();
        if (state >= 0 && v.state && sent && v.in(f).size() != v.size(f.n / nx, (std::size_t)nx))
            v.in(f).assign(v.size(f.n / nx, (std::size_t)nx), 0.);
    }
    f.dyn.present = f.dyn.present || state >= 0;
    forPayload(f, thermodynamics, nx, r0, r1, state, [&](std::vector<double>& a, std::size_t at, std::size_t length) {
        std::copy(data, data + length, a.begin() + at);
        data += length;
    });
}

} // namespace Nextsim
