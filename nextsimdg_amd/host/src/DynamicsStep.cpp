#include "DynamicsStep.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cctype>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <sstream>
#include <stdexcept>

#include "DynamicsBlock.hpp"
#include "DynamicsOutputs.hpp"
#include "ForcingFile.hpp"
#include "BathymetryFile.hpp"
#include "LandMaskFile.hpp"
#include "ModuleLoader.hpp"
#include "PhaseTiming.hpp"
#include "PhysicsModules.hpp"
#include "Rendezvous.hpp"
#include "Timer.hpp"

namespace Nextsim {

namespace {
std::atomic<long> g_localGroup { 1 }; // ids of the in-process communicator groups of this process
} // namespace

template <>
const std::map<int, std::string> Configured<DynamicsStep>::keyMap = { { 0, "dynamics.domain_size" }, { 1, "dynamics.nsub" },
    { 2, "dynamics.alpha" }, { 3, "dynamics.beta" }, { 4, "dynamics.thermodynamics" }, { 5, "dynamics.row_blocks" },
    { 6, "dynamics.passes_per_exchange" }, { 7, "dynamics.overlap" }, { 8, "dynamics.graph" }, { 9, "dynamics.forcing" },
    { 10, "dynamics.devices" }, { 11, "dynamics.loopback_world" }, { 12, "dynamics.closure" }, { 13, "dynamics.min_conc" },
    { 14, "dynamics.min_thick" }, { 15, "dynamics.delta_min" }, { 16, "dynamics.subcycle" }, { 17, "dynamics.substeps" },
    { 18, "dynamics.substep_courant" }, { 19, "dynamics.max_substeps" }, { 20, "dynamics.forcing_file" },
    { 21, "dynamics.advect_column_state" }, { 22, "dynamics.land_mask_file" }, { 23, "dynamics.rheology" },
    { 24, "dynamics.bbm_courant" }, { 25, "dynamics.tracers" }, { 26, "dynamics.tracer_init" },
    { 27, "dynamics.bathymetry_file" }, { 28, "dynamics.slab_ocean" }, { 29, "dynamics.snow_load" }, { 30, "dynamics.rho_snow" },
    { 31, "dynamics.tilt" }, { 32, "dynamics.gravity" } };

// dynamics.rheology = bbm
struct DynamicsStep::Brittle {
    nsdg_bbm_params params;
    double courant = NSDG_BBM_COURANT;
    bool warned = false; // the line about an explicit dynamics.nsub below the rule's value has been printed
};
// the four outputs (DynamicsOutputs.hpp), each null when its keys leave it off
struct DynamicsStep::Outputs {
    std::unique_ptr<HistoryChannel> history;
    std::unique_ptr<SeriesChannel> series;
    std::unique_ptr<DriftersChannel> drifters;
    std::unique_ptr<StationsChannel> stations;
    std::unique_ptr<BudgetChannel> budget; // (it also launches inside every sub-step: DynamicsOutputs.hpp)
    //! f(output) for every output that is on: history, series, drifters, stations
    template <class F> void each(F&& f)
    {
        if (history)
            f(*history);
        if (series)
            f(*series);
        if (drifters)
            f(*drifters);
        if (stations)
            f(*stations);
        if (budget)
            f(*budget);
    }
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
// [basal]: one key per member of nsdg_basal_params (include/nsdg_basal.h)
struct BasalKey {
    const char* key;
    double nsdg_basal_params::*member;
};
// [slabocean]: one key per member of nsdg_slab_params (include/nsdg_ocean.h)
struct SlabKey {
    const char* key;
    double nsdg_slab_params::*member;
};
const SlabKey SLAB_KEYS[] = { { "slabocean.relax_t", &nsdg_slab_params::relax_t }, { "slabocean.relax_s", &nsdg_slab_params::relax_s },
    { "slabocean.ice_salinity", &nsdg_slab_params::ice_salinity } };
const BasalKey BASAL_KEYS[] = { { "basal.k1", &nsdg_basal_params::k1 }, { "basal.k2", &nsdg_basal_params::k2 },
    { "basal.alpha_b", &nsdg_basal_params::alpha_b }, { "basal.u0", &nsdg_basal_params::u0 } };
} // namespace

std::vector<std::string> DynamicsStep::tracerNames(const std::string& value)
{
    const std::string key = "dynamics.tracers";
    // what a restart file, the state of the dynamics and the column model already call something
    static const char* const TAKEN[] = { "hice", "cice", "hsnow", "sst", "sss", "tice", "newice", "hice_dg", "cice_dg", "hsnow_dg", "damage", "u", "v",
        "s11", "s12", "s22", "H", "A", "S", "Q", "D", "tice0", "tracers" };
    std::vector<std::string> names;
    std::stringstream ss(value);
    for (std::string name; std::getline(ss, name, ',');) {
        name.erase(0, name.find_first_not_of(" \t"));
        name.erase(name.find_last_not_of(" \t") + 1);
        bool identifier = !name.empty() && !std::isdigit((unsigned char)name[0]);
        for (const char c : name)
            identifier = identifier && (std::isalnum((unsigned char)c) || c == '_');
        if (!identifier)
            throw std::invalid_argument(key + ": \"" + name + "\" is not an identifier (letters, digits and _, not starting with a digit)");
        for (const char* taken : TAKEN)
            if (name == taken)
                throw std::invalid_argument(key + ": \"" + name + "\" collides with a name of the state");
        if (std::find(names.begin(), names.end(), name) != names.end())
            throw std::invalid_argument(key + ": \"" + name + "\" is named more than once");
        names.push_back(name);
    }
    if (names.size() > NSDG_TRACERS_MAX)
        throw std::invalid_argument(key + ": " + std::to_string(names.size()) + " names; the tracer group carries at most " + std::to_string(NSDG_TRACERS_MAX));
    return names;
}

const std::vector<std::string>& DynamicsStep::tiltKeys()
{
    static const std::vector<std::string> keys = { keyMap.at(31), keyMap.at(32) };
    return keys;
}

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

DynamicsStep::DynamicsStep() : m_out(std::make_unique<Outputs>()) { }
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
    // landfast ice (include/nsdg_basal.h): the water depth, checked against the mask just read, and the [basal] parameters -- the rule of
    // nsdg_basal_params_set, applied here, before any device is touched
    m_bathymetry.reset();
    nsdg_basal_default_params(&m_basal);
    {
        const std::string path = getConfiguration(keyMap.at(27), std::string(""));
        bool given = false;
        for (const BasalKey& k : BASAL_KEYS) {
            const double value = getConfiguration(std::string(k.key), m_basal.*k.member);
            given = given || value != m_basal.*k.member;
            m_basal.*k.member = value;
            if (!std::isfinite(value) || value < 0. || (value == 0. && (k.member == &nsdg_basal_params::k1 || k.member == &nsdg_basal_params::u0)))
                throw std::invalid_argument(std::string("[basal]: ") + k.key + " = " + std::to_string(value)
                    + ": need k1 > 0, k2 >= 0, alpha_b >= 0 and u0 > 0, all finite");
        }
        if (path.empty() && given)
            throw std::invalid_argument("[basal]: the grounding scheme's parameters need dynamics.bathymetry_file");
        if (!path.empty()) {
            m_bathymetry = std::make_shared<const BathymetryFile>(path, m_landMask.get());
            if (pStructure)
                m_bathymetry->checkShape((std::size_t)pStructure->nx(), (std::size_t)pStructure->ny());
        }
    }
    // slab ocean (include/nsdg_ocean.h): the mode and the [slabocean] parameters -- the rule of nsdg_slab_params_set, applied here, before
    // any device is touched
    slabOcean = getConfiguration(keyMap.at(28), false);
    if (slabOcean && !thermo)
        throw std::invalid_argument("dynamics.slab_ocean needs dynamics.thermodynamics = true: the mixed layer follows the fluxes of the "
                                    "column step, and without the column model there are none");
    nsdg_slab_default_params(&m_slab);
    for (const SlabKey& k : SLAB_KEYS) {
        std::string raw;
        if (Configurator::lookup(k.key, raw) && !slabOcean)
            throw std::invalid_argument(std::string("[slabocean]: ") + k.key + " needs dynamics.slab_ocean = true");
        const double value = getConfiguration(std::string(k.key), m_slab.*k.member);
        m_slab.*k.member = value;
        if (!std::isfinite(value) || value < 0.)
            throw std::invalid_argument(std::string("[slabocean]: ") + k.key + " = " + std::to_string(value)
                + ": need relax_t >= 0, relax_s >= 0 and ice_salinity >= 0, all finite");
    }
    // snow load (include/nsdg_snow.h): the momentum equation feels the snow's weight -- the rule of nsdg_snow_load_set, applied here, before
    // any device is touched
    snowLoad = getConfiguration(keyMap.at(29), false);
    if (snowLoad && !thermo)
        throw std::invalid_argument("dynamics.snow_load needs dynamics.thermodynamics = true: without the column model there is no snow to weigh");
    {
        std::string raw;
        if (Configurator::lookup(keyMap.at(30), raw) && !snowLoad)
            throw std::invalid_argument("dynamics.rho_snow needs dynamics.snow_load = true");
        rhoSnow = getConfiguration(keyMap.at(30), (double)NSDG_SNOW_DENSITY);
        if (!std::isfinite(rhoSnow) || rhoSnow < 0.)
            throw std::invalid_argument("dynamics.rho_snow = " + std::to_string(rhoSnow) + ": need a finite density >= 0");
    }
    // sea-surface tilt (include/nsdg_tilt.h): from the geostrophic current, as ever, or from a sea-surface height -- the rule of
    // nsdg_tilt_set and what the forcing file must hold, applied here, before any device is touched
    {
        const std::string tilt = getConfiguration(keyMap.at(31), std::string("geostrophic"));
        if (tilt != "geostrophic" && tilt != "ssh")
            throw std::invalid_argument("dynamics.tilt must be geostrophic or ssh, got \"" + tilt + "\"");
        tiltSsh = tilt == "ssh";
        std::string raw;
        if (Configurator::lookup(keyMap.at(32), raw) && !tiltSsh)
            throw std::invalid_argument("dynamics.gravity needs dynamics.tilt = ssh");
        gravity = getConfiguration(keyMap.at(32), (double)NSDG_GRAVITY);
        if (!std::isfinite(gravity) || !(gravity > 0.))
            throw std::invalid_argument("dynamics.gravity = " + std::to_string(gravity) + ": need a finite gravity > 0");
        if (m_forcingFile && m_forcingFile->hasSsh() && !tiltSsh)
            throw std::invalid_argument("dynamics.forcing_file " + m_forcingFile->path() + " holds ssh: it needs dynamics.tilt = ssh");
        if (m_forcingFile && tiltSsh && m_forcingFile->hasOcean() && !m_forcingFile->hasSsh())
            throw std::invalid_argument("dynamics.tilt = ssh: dynamics.forcing_file " + m_forcingFile->path() + " holds ocean_u / ocean_v but no ssh -- "
                                        "the current is then the drag velocity alone and the tilt needs the height");
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
    // ice tracers (include/nsdg.h "ice tracers"): the names and the files of their initial values, read and checked here
    m_tracers = tracerNames(getConfiguration(keyMap.at(25), std::string("")));
    m_tracerInit.assign(m_tracers.size(), std::vector<double>());
    {
        const std::string key = keyMap.at(26), value = getConfiguration(key, std::string(""));
        std::vector<std::string> files;
        std::stringstream ss(value);
        for (std::string item; std::getline(ss, item, ',');)
            files.push_back(item);
        if (!value.empty() && files.size() != m_tracers.size())
            throw std::invalid_argument(key + ": " + std::to_string(files.size()) + " entries for the " + std::to_string(m_tracers.size())
                + " names of dynamics.tracers (a .npy file or - for each)");
        for (std::size_t k = 0; k < files.size(); ++k) {
            if (files[k] == "-")
                continue;
            Npy a;
            try {
                a = readNpy(files[k]);
            } catch (const std::exception& e) {
                throw std::invalid_argument(key + ": " + e.what());
            }
            if (a.shape.size() != 2 || (pStructure && (a.shape[0] != (std::uint64_t)pStructure->nx() || a.shape[1] != (std::uint64_t)pStructure->ny())))
                throw std::invalid_argument(key + ": " + files[k] + " does not have the shape (rectgrid.nx, rectgrid.ny) of the structure's planes");
            m_tracerInit[k] = std::move(a.values);
        }
    }
    configureOutputs();
}

void DynamicsStep::configureOutputs()
{
    // history output (include/HistoryOutput.hpp): the keys are read and checked here, before any device is touched; period 0 = off
    *m_out = Outputs();
    const SampledState sampled { thermo, advectColumn };
    const HistoryOutput::Config hc = HistoryOutput::fromConfiguration(thermo, m_brittle != nullptr);
    if (hc.on())
        m_out->history = std::make_unique<HistoryChannel>(hc, sampled);
    // the time series of the domain totals (SeriesOutput): the same; a multi-process run is refused here, nothing gathers its rows
    const SeriesOutput::Config sc = SeriesOutput::fromConfiguration(thermo, RankEnvironment::fromEnv().world);
    if (sc.on())
        m_out->series = std::make_unique<SeriesChannel>(sc, sampled, L);
    // drifters (include/Drifters.hpp): the keys and the input file are read and checked here, before any device is touched; a
    // multi-process run is refused here
    const DriftersOutput::Config dc = DriftersOutput::fromConfiguration(RankEnvironment::fromEnv().world, loopbackWorld != 0, thermo, m_brittle != nullptr);
    if (dc.on())
        m_out->drifters = std::make_unique<DriftersChannel>(dc, sampled, DriftersOutput::read(dc.file, L, L));
    // stations (include/Stations.hpp): the same
    const StationsOutput::Config stc = StationsOutput::fromConfiguration(RankEnvironment::fromEnv().world, loopbackWorld != 0, thermo, m_brittle != nullptr);
    if (stc.on())
        m_out->stations = std::make_unique<StationsChannel>(stc, sampled, StationsOutput::read(stc.file, L, L));
    // the momentum budget (include/BudgetOutput.hpp): the same; a multi-process run and the brittle rheology are refused here
    const BudgetOutput::Config bc = BudgetOutput::fromConfiguration(RankEnvironment::fromEnv().world, m_brittle != nullptr);
    if (bc.on())
        m_out->budget = std::make_unique<BudgetChannel>(bc);
}

void DynamicsStep::init()
{
    configure();
    const RankEnvironment env = RankEnvironment::fromEnv();
    m_world = env.world, m_rank = env.rank;
    setMultiProcess(m_world > 1);
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

void DynamicsStep::makeBlocks()
{
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
    std::vector<int> ranks;
    if (m_world > 1)
        ranks.push_back(m_rank);
    else if (loop)
        ranks.push_back(loopbackWorld / 2);
    else
        for (int r = 0; r < world; ++r)
            ranks.push_back(r);
    for (std::size_t i = 0; i < ranks.size(); ++i)
        m_blocks.push_back(std::make_unique<DynamicsBlock>((int)i, ranks[i], world, devs[i % devs.size()], nxf, nyf, depthBelow, depthAbove, loop));
}

void DynamicsStep::communicatorId(unsigned char* commId)
{
    std::memset(commId, 0, NSDG_COMM_ID_BYTES);
    if (m_world > 1 || loopbackWorld > 0) {
        if (m_rank == 0)
            check(nsdg_comm_unique_id(commId), "nsdg_comm_unique_id");
        if (m_world > 1)
            broadcastFromRankZero(RankEnvironment::fromEnv(), commId, NSDG_COMM_ID_BYTES);
    }
}

void DynamicsStep::start(const Iterator::TimePoint& startTime)
{
    ScopedTimer timer("start (upload)");
    if (!pStructure)
        throw std::logic_error("DynamicsStep: setInitialData() was not called");
    if (!m_inited)
        init();
    const FieldStore& f = pStructure->fields();
    nxf = pStructure->ny(); // fast dimension of the x-major index i*ny + j
    nyf = pStructure->nx();
    m_time = (double)startTime;
    const std::size_t nblocks = (m_world > 1 || loopbackWorld > 0) ? 1 : (std::size_t)rowBlocks; // what makeBlocks() will make
    m_out->each([&](auto& output) { output.start((long)startTime, nblocks); });
    if (m_landMask) {
        m_landMask->checkShape((std::size_t)nyf, (std::size_t)nxf);
        if (m_rank == 0)
            std::printf("dynamics land mask: %zu of %zu elements are land (%s)\n", m_landMask->landElements(), (std::size_t)nxf * nyf,
                m_landMask->path().c_str());
    }
    if (m_bathymetry) {
        m_bathymetry->checkShape((std::size_t)nyf, (std::size_t)nxf);
        if (m_rank == 0)
            std::printf("dynamics bathymetry: the shallowest ocean element has %g m of water; k1 = %g, k2 = %g N m^-3, alpha_b = %g, u0 = %g m/s (%s)\n",
                m_bathymetry->shallowest(), m_basal.k1, m_basal.k2, m_basal.alpha_b, m_basal.u0, m_bathymetry->path().c_str());
    }
    if (slabOcean && m_rank == 0)
        std::printf("dynamics slab ocean: relax_t = %g s, relax_s = %g s, ice_salinity = %g; relaxation targets: %s\n", m_slab.relax_t, m_slab.relax_s,
            m_slab.ice_salinity,
            !(m_slab.relax_t > 0 || m_slab.relax_s > 0) ? "none" : (m_forcingFile && m_forcingFile->hasSlabTargets() ? "the forcing file's sst, sss" : "the initial sst, sss"));
    for (std::size_t k = 0; k < m_tracers.size(); ++k)
        if (!m_tracerInit[k].empty() && m_tracerInit[k].size() != (std::size_t)nxf * nyf)
            throw std::invalid_argument("dynamics.tracer_init: the array of \"" + m_tracers[k] + "\" does not have the shape (rectgrid.nx, rectgrid.ny) of the structure's planes");
    makeBlocks();
    const long group = g_localGroup++;
    unsigned char commId[NSDG_COMM_ID_BYTES];
    communicatorId(commId);

    forEachBlock(m_blocks, [&](DynamicsBlock& b) {
        // ---- context
        b.createContext(phaseTiming);
        nsdg_ctx* ctx = b.ctx.get();
        if (b.world > 1) {
            if (m_world > 1)
                check(nsdg_comm_init(ctx, m_rank, m_world, commId), "nsdg_comm_init");
            else if (loopbackWorld > 0)
                check(nsdg_comm_init(ctx, 0, 1, commId), "nsdg_comm_init (loopback)");
            else
                check(nsdg_comm_init_local(ctx, group, b.rank, b.world), "nsdg_comm_init_local");
        }
        if (thermo) {
            nsdg_column_params p;
            IPhysics1d& phys = ModuleLoader::getLoader().getImplementation<IPhysics1d>();
            phys.describe(p);
            check(nsdg_column_params_set(ctx, &p), "nsdg_column_params_set");
        }
        // ---- arrays
        b.allocate(m_brittle != nullptr, advectColumn, (int)m_tracers.size(), tiltSsh);
        check(nsdg_grid_set(ctx, b.nx, b.ny, L / nxf, L / nyf), "nsdg_grid_set");
        check(nsdg_block_set(ctx, b.lo, b.nyGlobal), "nsdg_block_set");
        // ---- land mask, upload
        if (m_landMask)
            b.setLandMask(*m_landMask);
        if (m_bathymetry)
            b.setBathymetry(*m_bathymetry, m_basal);
        b.upload(f, thermo, b.index == 0 && m_rank == 0);
        b.uploadTracers(f, m_tracers, m_tracerInit, b.index == 0 && m_rank == 0);
        if (slabOcean) // (after the upload: the relaxation targets start as the initial sst, sss)
            b.setSlabOcean(m_slab);
        // ---- forcing: the analytic box test, evaluated on the device (ocean once, wind at the current model time every step); a forcing
        // file's wind and ocean pairs replace it at every step
        check(nsdg_boxtest_forcing(ctx, L, m_time, b.d[UA], b.d[VA], b.d[UO], b.d[VO]), "nsdg_boxtest_forcing");
        if (tiltSsh) { // the height whose geostrophic current is that gyre; a forcing file's ssh replaces it at every step
            nsdg_mevp_params p;
            nsdg_mevp_default_params(&p);
            check(nsdg_boxtest_ssh(ctx, L, p.fc, gravity, b.d[SSH]), "nsdg_boxtest_ssh");
        }
        if (m_forcingFile) // two records of every variable
            b.allocateRecords(2 * m_forcingFile->variables().size() * (std::size_t)m_forcingFile->nxr() * m_forcingFile->nyr());
        if (m_landMask)
            b.clearLand(thermo);
        // ---- outputs
        m_out->each([&](auto& output) { output.allocate(b); });
        // ---- plans
        if (m_brittle) // the brittle plan is made when the sub-iteration count of the step is known (subStep)
            check(nsdg_bbm_params_set(ctx, &m_brittle->params), "nsdg_bbm_params_set");
        else
            b.makeMevpPlan(nsub, overlap, graph);
        b.makeTransportPlan(closure);
        if (b.ntracers > 0)
            b.makeTracerPlan();
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
        forEachBlock(m_blocks, [&](DynamicsBlock& b) {
            check(nsdg_phase_mark(b.ctx.get(), NSDG_PHASE_REDUCTION), "nsdg_phase_mark"); // (the marks do nothing unless model.phase_timing is on)
            check(nsdg_concentration_max(b.ctx.get(), b.j0, b.j1, b.cur(FH), b.cur(FA), &b.amax), "nsdg_concentration_max");
        });
        double amax = 0.; // the blocks of this process are its threads: their maximum is taken here ...
        for (auto& b : m_blocks)
            amax = std::max(amax, b->amax);
        if (m_world > 1) // ... and the processes' through the communicator
            check(nsdg_comm_max_f64(m_blocks[0]->ctx.get(), &amax), "nsdg_comm_max_f64");
        double c = 0.;
        int32_t k = 0;
        check(nsdg_substep_count(&p, amax, cellSize(), dt, substepCourant, maxSubsteps, &k, &c), "dynamics.substeps = auto");
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
    if (m_out->series)
        m_out->series->afterStep((long)dtSeconds, m_blocks);
    if (m_out->history)
        m_out->history->afterStep((long)dtSeconds, m_blocks);
    if (m_out->stations)
        m_out->stations->afterStep((long)dtSeconds, m_blocks);
    if (m_out->drifters)
        m_out->drifters->afterStep((long)dtSeconds, m_blocks);
    if (m_out->budget)
        m_out->budget->afterStep((long)dtSeconds, m_blocks);
}

int DynamicsStep::brittleSubIterations(double dt, double rhoIce)
{
    int32_t need = 0;
    check(nsdg_bbm_substep_count(&m_brittle->params, rhoIce, cellSize(), dt, m_brittle->courant, 100000000, &need), "dynamics.bbm_courant");
    if (!nsubGiven)
        return need;
    if (nsub < need && !m_brittle->warned && m_rank == 0) {
        std::printf("dynamics rheology bbm: WARNING dynamics.nsub = %d is below the %d sub-iterations the elastic-wave rule asks for at dt = %g s "
                    "(dynamics.bbm_courant = %g)\n", nsub, (int)need, dt, m_brittle->courant);
        m_brittle->warned = true;
    }
    return nsub;
}

void DynamicsStep::subStep(double dt, bool last)
{
    nsdg_mevp_params p;
    nsdg_mevp_default_params(&p);
    if (!m_brittle) { // (the brittle pass ignores alpha, beta and the adaptive constants)
        const SubcycleChoice sc = subcycleChoice(cellSize(), dt);
        p.alpha = sc.alpha, p.beta = sc.beta, p.delta_min = sc.deltaMin, p.aevp_c = sc.aevpC, p.aevp_alpha_min = sc.aevpAlphaMin;
    }
    p.min_conc = closure ? minConc : 0.;
    p.min_thick = closure ? minThick : 0.;
    const int bsub = m_brittle ? brittleSubIterations(dt, p.rho_ice) : nsub;
    const double t = m_time;
    const int kind = forcing == "winter" ? NSDG_FORCING_WINTER : NSDG_FORCING_DUMMY;
    const ForcingFile* ff = m_forcingFile.get();
    std::size_t k0 = 0, k1 = 0;
    double w = 0.;
    if (ff)
        ff->bracket(t, k0, k1, w); // the records around the model time (throws outside the file's time range)
    DriftersChannel* drifters = m_out->drifters && m_out->drifters->any() ? m_out->drifters.get() : nullptr;
    forEachBlock(m_blocks, [&](DynamicsBlock& b) {
        nsdg_ctx* ctx = b.ctx.get();
        double* tr[NSDG_TRACERS_MAX] = {}; // dynamics.tracers: the planes of the tracers and the current buffers of their products
        double* tq[NSDG_TRACERS_MAX] = {};
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
            if (b.ntracers > 0) // the mean thickness the column step starts from (nsdg_tracers_dilute below)
                check(nsdg_copy_f64(ctx, b.thicknessBefore(), b.cur(FH), b.N), "nsdg_copy_f64");
            // the column physics needs no exchange: it runs on the ghost rows too, redundantly
            if (slabOcean) // the fused step: sst and sss follow the fluxes; land elements (the block's land bytes) keep theirs
                check(nsdg_column_step_ocean(ctx, b.N, dt, b.cur(FH), b.cur(FA), advectColumn ? b.cur(FS) : b.col(C_HSNOW), b.col(C_TICE), b.col(C_SST),
                          b.col(C_SSS), b.col(C_TAIR), b.col(C_TDEW), b.col(C_SLP), b.col(C_QSW), b.col(C_QLW), b.col(C_MLD), b.col(C_SNOWFALL),
                          b.col(C_WIND), b.col(C_NEWICE), b.sstExt, b.sssExt, b.land.get()),
                    "nsdg_column_step_ocean");
            else
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
            if (b.ntracers > 0) { // ice that grew carries the value 0 (every local row: element-local, as the column step)
                for (int k = 0; k < b.ntracers; ++k)
                    tr[k] = b.tracer(k);
                check(nsdg_tracers_dilute(ctx, 0, b.ny, b.thicknessBefore(), b.cur(FH), b.ntracers, tr), "nsdg_tracers_dilute");
            }
        }
        check(nsdg_phase_mark(ctx, NSDG_PHASE_PREPARE), "nsdg_phase_mark");
        if (snowLoad) // the snow as it stands after this step's column step; the transport's ping-pong moves S: set before every packing
            check(nsdg_snow_load_set(ctx, advectColumn ? b.cur(FS) : b.col(C_HSNOW), advectColumn ? 6 : 1, rhoSnow), "nsdg_snow_load_set");
        if (tiltSsh) // the block's sea-surface height: the packing below reads it
            check(nsdg_tilt_set(ctx, b.d[SSH], gravity), "nsdg_tilt_set");
        int32_t out = 0;
        if (m_brittle) {
            // the Gauss arrays of the brittle sub-cycle and the mEVP packing for the sub-iteration's dt with u0 = v0 = 0: no ice strength
            check(nsdg_bbm_prepare(ctx, 0, b.ny, b.cur(FH), b.cur(FA), b.d[HG], b.d[EG], b.d[PM]), "nsdg_bbm_prepare");
            check(nsdg_mevp_prepare(ctx, bsub > 0 ? dt / bsub : dt, b.cur(FH), b.cur(FA), b.d[UA], b.d[VA], b.d[UO], b.d[VO], b.d[ZERO], b.d[ZERO], b.d[PACKED]),
                "nsdg_mevp_prepare");
            if (!b.bbm || b.bbmNsub != bsub) // the plan holds the count: a new one when the rule gives another (another dt)
                b.makeBbmPlan(bsub, overlap, drifters != nullptr); // (the drifters' predictor may sit in the ghost row above: complete nodes)
            check(nsdg_phase_mark(ctx, NSDG_PHASE_SUBCYCLE), "nsdg_phase_mark");
            check(nsdg_rb_bbm_run(ctx, b.bbm.get(), b.par, b.tpar, &out), "nsdg_rb_bbm_run");
        } else {
            check(nsdg_ice_strength(ctx, 0, b.ny, b.cur(FH), b.cur(FA), b.d[PG]), "nsdg_ice_strength");
            check(nsdg_mevp_prepare(ctx, dt, b.cur(FH), b.cur(FA), b.d[UA], b.d[VA], b.d[UO], b.d[VO], b.curU(), b.curV(), b.d[PACKED]), "nsdg_mevp_prepare");
            check(nsdg_phase_mark(ctx, NSDG_PHASE_SUBCYCLE), "nsdg_phase_mark");
            check(nsdg_rb_mevp_run(ctx, b.mevp.get(), b.par, &out), "nsdg_rb_mevp_run");
        }
        b.par = out;
        if (m_out->budget) // still the sub-cycle's phase: H, A and the packing are the sub-cycle's
            m_out->budget->launch(b);
        check(nsdg_phase_mark(ctx, NSDG_PHASE_TRANSPORT), "nsdg_phase_mark");
        check(nsdg_prepare_advection(ctx, 2, b.curU(), b.curV(), b.d[VXDG], b.d[VYDG], b.d[UNX], b.d[UNY]), "nsdg_prepare_advection");
        // the surface temperature travels as Q = H tice0 (every local row: element-local, the ghost rows stay equal to their owners)
        if (advectColumn)
            check(nsdg_tracer_weight(ctx, 2, 0, b.ny, b.cur(FH), b.col(C_TICE), b.cur(FQ)), "nsdg_tracer_weight");
        if (b.ntracers > 0) { // the tracers' products, with the thickness the step starts from (every local row, as above)
            for (int k = 0; k < b.ntracers; ++k)
                tr[k] = b.tracer(k), tq[k] = b.tracerQ(k, b.qpar);
            check(nsdg_tracers_weight(ctx, 2, 0, b.ny, b.cur(FH), b.ntracers, tr, tq), "nsdg_tracers_weight");
        }
        check(nsdg_rb_transport_run(ctx, b.transport.get(), dt, b.tpar, &out), "nsdg_rb_transport_run");
        b.tpar = out;
        if (advectColumn)
            check(nsdg_tracer_recover(ctx, 2, 0, b.ny, b.cur(FH), b.cur(FA), b.cur(FQ), p.min_conc, p.min_thick, b.col(C_TICE)), "nsdg_tracer_recover");
        if (b.ntracers > 0) {
            // the second transport group: the same prepared velocity and dt, no bounds; then the division back, which ages `age` by dt
            check(nsdg_rb_transport_run(ctx, b.tracerTransport.get(), dt, b.qpar, &out), "nsdg_rb_transport_run (tracers)");
            b.qpar = out;
            int32_t kinds[NSDG_TRACERS_MAX] = {};
            for (int k = 0; k < b.ntracers; ++k)
                tq[k] = b.tracerQ(k, b.qpar), kinds[k] = m_tracers[k] == "age" ? NSDG_TRACER_AGE : NSDG_TRACER_PASSIVE;
            check(nsdg_tracers_recover(ctx, 2, 0, b.ny, b.cur(FH), b.cur(FA), b.ntracers, tq, kinds, dt, p.min_conc, p.min_thick, tr),
                "nsdg_tracers_recover");
        }
        if (drifters)
            drifters->advance(b, dt);
        if (last) // the model step ends here: what follows until its next mark belongs to no phase
            check(nsdg_phase_mark(ctx, NSDG_PHASE_END), "nsdg_phase_mark");
    });
}

void DynamicsStep::resolvePhaseTimes()
{
    // once, after the run: the only place where the host waits for the marks (nsdg_phase_times; stop() has drained the streams already)
    std::vector<PhaseBlockTimes> tables;
    forEachBlockInTurn(m_blocks, [&](DynamicsBlock& b) {
        PhaseBlockTimes t;
        t.block = b.rank;
        check(nsdg_phase_times(b.ctx.get(), &t.table, 0), "nsdg_phase_times");
        t.hasExchange = b.peerBelow >= 0 || b.peerAbove >= 0;
        if (t.hasExchange) {
            if (b.bbm) // (the plan of the last sub-iteration count)
                check(nsdg_rb_bbm_stats(b.ctx.get(), b.bbm.get(), &t.subcycleExchange, 0), "nsdg_rb_bbm_stats");
            else if (b.mevp)
                check(nsdg_rb_mevp_stats(b.ctx.get(), b.mevp.get(), &t.subcycleExchange, 0), "nsdg_rb_mevp_stats");
            check(nsdg_rb_transport_stats(b.ctx.get(), b.transport.get(), &t.transportExchange, 0), "nsdg_rb_transport_stats");
        }
        tables.push_back(t);
    });
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
        check(nsdg_ctx_synchronize(b.ctx.get()), "DynamicsStep: forcing record upload");
        checkHip(hipMemcpy(b.records.get() + s * slot, host.data(), slot * sizeof(double), hipMemcpyHostToDevice), "upload forcing record");
        b.recordOf[s] = k;
        at[i] = s;
        if (k0 == k1)
            at[1] = s;
    }
    auto rec = [&](int i, const std::string& var) -> const double* {
        std::size_t v = 0;
        while (vars[v] != var)
            ++v;
        return b.records.get() + at[i] * slot + v * plane;
    };
    // one launch per lattice: the wind and ocean pairs at the CG2 nodes, the column planes at the element centres
    std::vector<const double*> r0, r1;
    std::vector<double*> out;
    for (const auto& pr : { std::make_pair("wind_u", UA), std::make_pair("wind_v", VA), std::make_pair("ocean_u", UO), std::make_pair("ocean_v", VO),
             std::make_pair("ssh", SSH) })
        if (ff.has(pr.first)) {
            r0.push_back(rec(0, pr.first)), r1.push_back(rec(1, pr.first)), out.push_back(b.d[pr.second]);
        }
    if (!out.empty())
        check(nsdg_forcing_sample(b.ctx.get(), NSDG_AT_NODES, ff.nxr(), ff.nyr(), (int32_t)out.size(), r0.data(), r1.data(), w, out.data()),
            "nsdg_forcing_sample (nodes)");
    if (thermo) {
        r0.clear(), r1.clear(), out.clear();
        const int planes[7] = { C_TAIR, C_TDEW, C_SLP, C_QSW, C_QLW, C_MLD, C_SNOWFALL };
        for (int c = 0; c < 7; ++c) {
            const std::string& var = ForcingFile::columnVariables()[c];
            r0.push_back(rec(0, var)), r1.push_back(rec(1, var)), out.push_back(b.col(planes[c]));
        }
        check(nsdg_forcing_sample(b.ctx.get(), NSDG_AT_ELEMENTS, ff.nxr(), ff.nyr(), 7, r0.data(), r1.data(), w, out.data()),
            "nsdg_forcing_sample (elements)");
        // dynamics.slab_ocean: the file's pair sst, sss into the relaxation targets that exist, a launch of their own
        r0.clear(), r1.clear(), out.clear();
        if (slabOcean && ff.hasSlabTargets())
            for (const auto& pr : { std::make_pair("sst", b.sstExt), std::make_pair("sss", b.sssExt) })
                if (pr.second) {
                    r0.push_back(rec(0, pr.first)), r1.push_back(rec(1, pr.first)), out.push_back(pr.second);
                }
        if (!out.empty())
            check(nsdg_forcing_sample(b.ctx.get(), NSDG_AT_ELEMENTS, ff.nxr(), ff.nyr(), (int32_t)out.size(), r0.data(), r1.data(), w, out.data()),
                "nsdg_forcing_sample (slab ocean targets)");
    }
}

void DynamicsStep::stop(const Iterator::TimePoint&)
{
    ScopedTimer timer("stop (download)");
    if (m_blocks.empty())
        return;
    if (m_out->history) // (stop() comes twice -- the iterator's, the restart file's --: nothing is written twice)
        m_out->history->atStop(m_blocks);
    if (m_out->series)
        m_out->series->atStop(m_blocks);
    if (m_out->stations)
        m_out->stations->atStop(m_blocks);
    if (m_out->drifters)
        m_out->drifters->atStop(m_blocks);
    if (m_out->budget)
        m_out->budget->atStop(m_blocks);
    FieldStore& f = pStructure->fields();
    std::vector<double> umax(m_blocks.size(), 0.);
    bool finite = true;
    forEachBlockInTurn(m_blocks, [&](DynamicsBlock& b) { // the blocks write disjoint row ranges of the host structure
        check(nsdg_ctx_synchronize(b.ctx.get()), "DynamicsStep::stop");
        uint32_t gaveUp = 0; // bounded waits of the mEVP pipeline that hit their bound: the fields would be wrong
        check(nsdg_mevp_pipeline_health(b.ctx.get(), &gaveUp), "nsdg_mevp_pipeline_health");
        if (gaveUp)
            throw std::runtime_error("DynamicsStep: " + std::to_string(gaveUp) + " wait(s) of the mEVP pipeline gave up: the fields are not to be trusted");
        b.download(f, thermo, advectColumn, slabOcean);
        b.downloadTracers(f, m_tracers);
        // owned node rows: [2 r0, 2 r1) plus the top boundary row on the last block
        const long nn = 2L * b.nx + 1, rows = 2L * b.ownedRows() + (b.peerAbove < 0 ? 1 : 0);
        for (long k = 2L * b.r0 * nn; k < (2L * b.r0 + rows) * nn; ++k) {
            umax[b.index] = std::max(umax[b.index], std::max(std::fabs(f.dyn.u[k]), std::fabs(f.dyn.v[k])));
            finite = finite && std::isfinite(f.dyn.u[k]) && std::isfinite(f.dyn.v[k]);
        }
    });
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
    const std::vector<double> mine = (m_rank == 0 || own) ? std::vector<double>() : packRows(f, thermo, nxf, r0, r1, slabOcean);
    gatherToRankZero(
        env, mine.data(), mine.size() * sizeof(double),
        [&](int rank, const char* data, std::size_t bytes) {
            if (own)
                return; // rank 0 itself failed: the rows are received and dropped, the senders are told below
            int a, b;
            splitRows(nyf, m_world, rank, a, b);
            placeRows(f, thermo, nxf, a, b, reinterpret_cast<const double*>(data), bytes / sizeof(double), slabOcean);
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
template <class F> void forPayload(FieldStore& f, bool thermodynamics, bool slabOcean, int nx, int r0, int r1, int state, F&& fn)
{
    const std::size_t first = (std::size_t)r0 * nx, rows = (std::size_t)(r1 - r0) * nx, nn = 2 * (std::size_t)nx + 1;
    for (auto* p : { &f.hice, &f.cice, &f.hsnow, &f.tice, &f.newice })
        if (thermodynamics || p == &f.hice || p == &f.cice) // (the column model's planes change only with it)
            fn(*p, first, rows);
    if (slabOcean) // (the mixed layer changes only with dynamics.slab_ocean: every rank runs the same mode)
        for (auto* p : { &f.sst, &f.sss })
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
    for (DynamicsState::NamedPlane& t : f.dyn.tracers) // dynamics.tracers: every rank runs the same names, so both ends hold the same planes
        fn(t.values, first, rows);
}
} // namespace

std::vector<double> DynamicsStep::packRows(FieldStore& f, bool thermodynamics, int nx, int r0, int r1, bool slabOcean)
{
    int state = f.dyn.present ? 0 : -1, bit = 0; // the state of the dynamics travels with the rows, with the optional variables it holds
    for (const DynamicsVariable& v : DYNAMICS_VARIABLES)
        if (v.optional())
            state |= (f.dyn.present && !v.in(f).empty() ? 1 : 0) << bit++;
    std::vector<double> out;
    forPayload(f, thermodynamics, slabOcean, nx, r0, r1, state, [&](std::vector<double>& a, std::size_t at, std::size_t length) { out.insert(out.end(), a.begin() + at, a.begin() + at + length); });
    return out;
}

void DynamicsStep::placeRows(FieldStore& f, bool thermodynamics, int nx, int r0, int r1, const double* data, std::size_t count, bool slabOcean)
{
    // what a rank sent shows in the size alone: its planes, or also the state of the dynamics with one of the sets of its optional
    // variables (their sizes differ, and a run holds the snow or the damage, never both: the first set that fits is the one)
    const int optional = (int)std::count_if(std::begin(DYNAMICS_VARIABLES), std::end(DYNAMICS_VARIABLES), [](const DynamicsVariable& v) { return v.optional(); });
    std::string sizes;
    int state = -2; // as forPayload reads it, once found
    for (int k = -1; k < (1 << optional) && state < -1; ++k) {
        std::size_t size = 0;
        forPayload(f, thermodynamics, slabOcean, nx, r0, r1, k, [&](std::vector<double>&, std::size_t, std::size_t length) { size += length; });
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
    forPayload(f, thermodynamics, slabOcean, nx, r0, r1, state, [&](std::vector<double>& a, std::size_t at, std::size_t length) {
        std::copy(data, data + length, a.begin() + at);
        data += length;
    });
}

} // namespace Nextsim
