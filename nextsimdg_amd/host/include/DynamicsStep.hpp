// DynamicsStep.hpp -- IModelStep implementation of the dynamics core: per time step the mEVP stress/velocity
// sub-cycle followed by the DG2 transport of the mean thickness H and concentration A, optionally preceded by
// the column thermodynamics (BASELINE config 5 coupling).  Everything numerical happens behind the C ABI
// (include/nsdg.h); this class owns the row blocks and the call sequence across them.  Who owns what: a row block (src/DynamicsBlock.hpp)
// owns its context, its device arrays and its driver plans and builds them from its geometry; each of the four outputs
// (src/DynamicsOutputs.hpp) owns its host object, its input list and its buffers on every block; configure(), start(), iterate(), subStep()
// and stop() here are the sequence of named steps over them.
//
// The reference has no dynamics component (CMakeLists.txt:43-46); the class plugs into the reference's
// batched seam (IModelStep, core/src/include/IModelStep.hpp:16-34) exactly like HipStep does and is selected with
//     [Modules] Nextsim::IModelStep = Nextsim::DynamicsStep
// The rectangular mesh is split into ROW BLOCKS with ghost rows; every block has its own context and is advanced
// by the row-block drivers of the ABI (nsdg_rb_mevp_run / nsdg_rb_transport_run: kernel passes and ghost-row
// exchanges of a step in one call each).  Three ways to run:
//   * one block (default): the whole grid on one GPU;
//   * dynamics.row_blocks = N: N blocks in THIS process, one host thread each, ghost rows through the in-process
//     transport (nsdg_comm_init_local) -- devices round-robin over dynamics.devices (default: all on device 0);
//   * one process per GPU under a launcher that sets WORLD_SIZE / RANK / LOCAL_RANK / MASTER_ADDR / MASTER_PORT
//     (Rendezvous.hpp): every process owns ONE block, ghost rows over RCCL send/recv (nsdg_comm_init).  Every rank
//     reads the same initial state; at the end the owned rows of every rank travel to rank 0 (TCP, once per run),
//     which writes ONE restart file -- the same file a single-process run writes.
// Configuration keys (all optional):
//     dynamics.domain_size   side of the square box in m        (512e3)
//     dynamics.nsub          mEVP sub-iterations per step        (120)
//     dynamics.subcycle      how the sub-cycle satisfies its stability bound (nsdg_mevp_stable_params, include/nsdg.h): adaptive (default
//                            since round 6: local, solution-adaptive alpha and beta at the literature's Delta_min, alpha_min = 50) |
//                            adaptive_converged (alpha_min from the mesh so that the sub-cycle converges; wants a time step that fits
//                            the mesh) | keep_alpha (round 5:
//                            uniform alpha = beta = dynamics.alpha or 1500, Delta_min raised to what the mesh needs for it) |
//                            keep_delta_min (rounds 1-4: uniform alpha = beta from the bound for dynamics.delta_min or 2e-9)
//     dynamics.alpha/.beta   uniform mEVP parameters (keep_alpha; 0 = 1500, the BASELINE's value); given WITHOUT dynamics.subcycle they
//                            select keep_alpha and are used as they are
//     dynamics.delta_min     regularisation of Delta [1/s] (0 = the literature's 2e-9)
//     dynamics.closure       ridging cap + scaling limiter in the transport, free drift at ice-free nodes (default true)
//     dynamics.min_conc/.min_thick   the ice-free-node rule's thresholds (defaults 1e-12, 0.01: the column model's cut-off)
//     dynamics.thermodynamics  run the column physics first       (false)
//     dynamics.advect_column_state  the snow and the ice surface temperature move with the ice (false; needs thermodynamics): the snow
//                            is a DG2 field S advected with H and A (plane 0 = hsnow), tice0 travels as Q = H tice0 (nsdg_tracer_weight
//                            before the transport, nsdg_tracer_recover after it: include/nsdg.h "column state transport"); a restart
//                            then also holds hsnow_dg, the higher coefficients of S
//     dynamics.forcing       thermodynamic forcing: host (the structure's planes, constant in time) | dummy | winter
//                            (generated on the device at every step's model time, wind speed from the dynamics' wind) | file
//                            (records of dynamics.forcing_file, sampled on the device at every (sub-)step's model time: bilinear in
//                            space, linear in time -- nsdg_forcing_sample; the file's wind_u / wind_v and ocean_u / ocean_v pairs, where
//                            present, replace the box test's cyclone and gyre; host/include/ForcingFile.hpp has the file layout)
//     dynamics.forcing_file  the forcing file of forcing = file; read and checked when the step is configured
//     dynamics.land_mask_file  a .npy array of uint8 or bool, shape (rectgrid.nx, rectgrid.ny) like the structure's planes, 1 = land
//                            (include/LandMaskFile.hpp; include/nsdg.h "land mask"): the nodes of land elements hold u = v = 0, H, A, the
//                            snow and the new ice are cleared on land at the start and after every column step; read and checked when the
//                            step is configured.  The restart file holds no mask: a resumed run names the same file
//     dynamics.bathymetry_file  a .npy array of float64, the water depth in metres per element, shape and orientation of the mask
//                            (include/BathymetryFile.hpp; include/nsdg_basal.h): finite and >= 0 at ocean
//                            elements, stored as 0 on land; ice whose keels reach the seabed feels a basal stress in the momentum update
//                            and stays fast over a shoal.  Read and checked when the step is configured; the restart file holds no copy
//     [basal] k1, k2, alpha_b, u0  the grounding scheme's parameters, one key per member of nsdg_basal_params (defaults: the published 8,
//                            15 N m^-3, 20, 5e-5 m/s; k1 > 0, k2 >= 0, alpha_b >= 0, u0 > 0, all finite); they need dynamics.bathymetry_file
//     dynamics.substeps      sub-steps per model step: an integer >= 1 (default 1: the unsplit step, bit for bit) or auto -- n decided at
//                            the start of every model step from the state's strength wave speed, the same on every block
//                            (nsdg_concentration_max, nsdg_comm_max_f64, nsdg_substep_count: include/nsdg.h "sub-stepping"); the whole
//                            step (forcing, column, strength, sub-cycle, transport) runs n times with dt / n
//     dynamics.substep_courant  cells the strength wave may cross per sub-step under auto (1.5)
//     dynamics.max_substeps  the largest n auto may choose (16); a state that needs more stops the run with the needed n
//     model.phase_timing, model.phase_timing_file   per-phase device time of the step (include/PhaseTiming.hpp)
//     model.output_period, model.output_file, model.output_fields, model.output_kind   history output: time means or snapshots of element
//                            fields, accumulated on the device after every model step and written once per window
//                            (include/HistoryOutput.hpp; include/nsdg.h "history output"); period 0 (default): off, nothing changes
//     model.drifters_file, model.drifters_output, model.drifters_period, model.drifters_min_conc   Lagrangian drifters moved by the ice
//                            velocity after every transport step and written as text blocks (include/Drifters.hpp; include/nsdg.h
//                            "drifters"); works with dynamics.row_blocks (block 0 writes), refused in a multi-process run; no file
//                            (default): off, nothing changes
//     model.drifters_fields  history field names sampled AT every drifter's new position after every (sub-)step and written as further
//                            columns (include/Drifters.hpp; include/nsdg.h "point samples"); not given (default): the file is as it was
//     model.stations_file, model.stations_output, model.stations_fields, model.stations_buffer   the same fields at fixed points after every
//                            model step, after the NSDG_PHASE_END mark like the history, one block of lines per step
//                            (include/Stations.hpp); block 0 writes the maximum over the row blocks; refused in a multi-process run
//     dynamics.rheology      mevp (default: every run without the key is byte for byte what it was) | bbm -- the brittle Bingham-Maxwell
//                            sub-cycle (include/nsdg.h "brittle rheology") through the row-block plan nsdg_rb_bbm_*:
//                            ghost depth (1, 1), one sub-iteration per pass, nsub explicit sub-iterations of dt / nsub; the damage D is a
//                            third advected field (bounds 0, 1, no cap), cleared on land, written to the restart file as `damage` (six
//                            planes; a file without it: the run starts undamaged) and offered to the history output as `damage`.
//                            dynamics.passes_per_exchange, .alpha, .beta and .subcycle do not apply.  Refused with
//                            dynamics.advect_column_state (five fields), dynamics.substeps = auto (that rule is the mEVP strength wave)
//                            and dynamics.graph
//     [bbm] young, nu, p0, lambda0, tan_phi, cohesion_lab, compr_strength, t_heal, d_max, relax_exponent   the members of
//                            nsdg_bbm_params (defaults: nsdg_bbm_default_params), checked by nsdg_bbm_params_check when the step is configured
//     dynamics.bbm_courant   cells the elastic wave may cross per sub-iteration (NSDG_BBM_COURANT = 0.25): without an explicit
//                            dynamics.nsub the count is nsdg_bbm_substep_count for the (sub-)step's dt; an explicit dynamics.nsub is used
//                            as given, with one warning line if it is below the rule's value
//     dynamics.tracers       names of up to NSDG_TRACERS_MAX ice tracers, comma-separated (include/nsdg.h "ice tracers"):
//                            intensive planes that ride on the ice as Q = H T in a transport run of their own after the run of H and A
//                            (nsdg_tracers_weight, a second transport plan without bounds, nsdg_tracers_recover); `age` grows by the
//                            (sub-)step's dt where there is ice, every other name is passive; with thermodynamics, ice that grows carries
//                            the value 0 (nsdg_tracers_dilute after the column step).  Names are identifiers, given once, and none of the
//                            restart file's own names.  A restart file holds them as `tracer_<name>`; one without a dataset starts that
//                            tracer at zero.  Not given (default): nothing changes
//     dynamics.tracer_init   their initial values, one entry per name: a float64 .npy array of the shape (rectgrid.nx, rectgrid.ny) of the
//                            structure's planes, or - for zeros; a restart file with the state of the dynamics takes precedence
//     dynamics.slab_ocean    false (default: nothing changes) | true -- the mixed layer's sst and sss are prognostic (include/nsdg_ocean.h,
//                            DESIGN.md section 3.11): the column step is nsdg_column_step_ocean, with the block's land bytes as its skip
//                            mask; the restart file's sst, sss datasets then hold the evolved ocean.  Needs dynamics.thermodynamics = true
//     [slabocean] relax_t, relax_s, ice_salinity   the members of nsdg_slab_params (defaults: nsdg_slab_default_params), by the rule of
//                            nsdg_slab_params_set; refused without dynamics.slab_ocean.  The relaxation targets are the forcing file's
//                            optional pair sst, sss sampled on the device, or, without it, the initial sst, sss
//     dynamics.snow_load     false (default: nothing changes) | true -- the momentum equation feels the snow's weight (include/nsdg_snow.h,
//                            DESIGN.md section 3.12): before every coefficient packing the block's snow -- the DG field S under
//                            dynamics.advect_column_state, else the plane hsnow -- is set on the context (nsdg_snow_load_set), and the
//                            nodal mass is rho_i cgH + rho_snow max(cgS, 0) where the node is neither land nor ice-free; both rheologies.
//                            Needs dynamics.thermodynamics = true.  The restart file needs nothing new: the snow is in it
//     dynamics.rho_snow      the density of that snow [kg m^-3], finite and >= 0 (default 330, the column step's); refused without
//                            dynamics.snow_load
//     dynamics.tilt          geostrophic (default: nothing changes) | ssh -- the sea-surface tilt is -m g grad(eta) of a sea-surface
//                            height (include/nsdg_tilt.h) and (uo, vo) is the drag velocity alone: before every
//                            coefficient packing the block's height is set on the context (nsdg_tilt_set); both rheologies.  The height
//                            is the forcing file's optional variable ssh [m], sampled at the nodes with the wind and ocean pairs; with
//                            any other forcing it is the box test's (nsdg_boxtest_ssh).  Refused: a forcing file with ocean_u / ocean_v
//                            but no ssh, and ssh in the file without dynamics.tilt = ssh.  The restart file needs nothing new
//     dynamics.gravity       g [m s^-2] of that tilt, finite and > 0 (default 9.81); refused without dynamics.tilt = ssh
//     dynamics.row_blocks, dynamics.devices, dynamics.passes_per_exchange (2), dynamics.overlap (true),
//     dynamics.graph (false), dynamics.loopback_world (0: off; N: rehearse an interior block of N on one GPU with
//     real RCCL send/recv to the rank itself -- values wrap around, for timing and call-path checks only)
// The structure's cell means initialise the DG fields: H <- hice, A <- cice (coefficient 0; higher coefficients
// start at zero) and receive them back at stop().  Ocean current and wind come from the device-side forcing
// provider nsdg_boxtest_forcing (the wind is re-evaluated at every step's model time), or from a forcing file's pairs.
#pragma once
#include "../../../include/nsdg_basal.h"
#include "../../../include/nsdg_ocean.h"
#include "../../../include/nsdg_snow.h"
#include "../../../include/nsdg_tilt.h"
#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "Configured.hpp"
#include "IStructure.hpp"
#include "Iterator.hpp"

struct nsdg_ctx;

namespace Nextsim {

class ForcingFile;
class LandMaskFile;
class BathymetryFile;

class DynamicsBlock; // one row block: context, device arrays, driver plans (src/DynamicsBlock.hpp)

class DynamicsStep : public IModelStep, public Configured<DynamicsStep> {
public:
    DynamicsStep();
    ~DynamicsStep() override;
    DynamicsStep(const DynamicsStep&) = delete;
    DynamicsStep& operator=(const DynamicsStep&) = delete;

    void configure() override;
    void setInitialData(IStructure& dataStructure) override { pStructure = &dataStructure; }
    void writeRestartFile(const std::string& filePath) override;
    void init() override;
    void start(const Iterator::TimePoint& startTime) override;
    void iterate(const Iterator::Duration& dt) override;
    void stop(const Iterator::TimePoint& stopTime) override;
    long launches() const override { return m_steps; }

    //! diagnostics after stop(): max |u|, sum of the H and A cell means (of the rows this process owns)
    double maxSpeed() const { return m_umax; }
    double sumH() const { return m_sumH; }
    double sumA() const { return m_sumA; }
    int blocks() const { return (int)m_blocks.size(); }
    //! the sub-cycle parameters this configuration runs with on cells of size h and a time step dt (nsdg_mevp_stable_params: the one copy
    //! of the stability rule); returns the creep threshold in percent per day beside them
    struct SubcycleChoice {
        std::string mode;
        double alpha, beta, deltaMin, aevpC, aevpAlphaMin, creepPercentPerDay;
    };
    SubcycleChoice subcycleChoice(double h, double dt) const;

    //! rows [r0, r1) of block `rank` of `world` (the same split as nextsimdg_amd/rowblock.py split_rows)
    static void splitRows(int ny, int world, int rank, int& r0, int& r1);

    //! rows [r0, r1) (nx values each) of every prognostic plane a run changes (hice, cice; with thermodynamics hsnow, tice, newice; with a
    //! slab ocean sst, sss after them) and of the state of the dynamics, one after the other -- what a rank sends for the restart file ...
    static std::vector<double> packRows(FieldStore& f, bool thermodynamics, int nx, int r0, int r1, bool slabOcean = false);
    //! ... and how rank 0 puts it into its structure; throws std::runtime_error when the size is not that of the rows
    static void placeRows(FieldStore& f, bool thermodynamics, int nx, int r0, int r1, const double* data, std::size_t count, bool slabOcean = false);
    //! the keys of the brittle rheology (dynamics.rheology, dynamics.bbm_courant, bbm.*): a step that does not run it refuses them
    static const std::vector<std::string>& brittleKeys();
    //! dynamics.tilt and dynamics.gravity: the keys that Nextsim::HipStep, which has no momentum equation, refuses
    static const std::vector<std::string>& tiltKeys();
    //! the names of dynamics.tracers from its value; throws std::invalid_argument, naming the key, for more than NSDG_TRACERS_MAX names, a
    //! name given twice, one that is no identifier and one that a restart file or the state already uses
    static std::vector<std::string> tracerNames(const std::string& value);

private:
    void release();
    //! forcing at m_time, column step, ice strength, prepare, sub-cycle and transport with dt, each opened by its phase mark; `last`: the
    //! model step ends with this sub-step (NSDG_PHASE_END)
    void subStep(double dt, bool last);
    void resolvePhaseTimes(); //!< model.phase_timing: every block's table -> the timer tree and model.phase_timing_file (PhaseTiming.hpp)
    //! dynamics.forcing = file: records k0, k1 resident on the block's device, sampled with time weight w into the block's wind / ocean
    //! (the pairs the file holds) and, with thermodynamics, its column forcing planes
    void sampleForcingFile(DynamicsBlock& b, std::size_t k0, std::size_t k1, double w);
    void configureOutputs(); //!< configure(): the four outputs from their keys and input files, last, in the order history, series, drifters, stations
    void makeBlocks(); //!< start(): the geometry of the blocks of this process, on their devices
    void communicatorId(unsigned char* id); //!< start(): the RCCL communicator id travels before anything else (multi-process run)
    int brittleSubIterations(double dt, double rhoIce); //!< the sub-iterations of a brittle (sub-)step of dt: dynamics.nsub as given, or the elastic-wave rule
    double cellSize() const { return std::min(L / nxf, L / nyf); }
    IStructure* pStructure = nullptr;
    std::vector<std::unique_ptr<DynamicsBlock>> m_blocks;
    int nxf = 0, nyf = 0; // fast / slow grid dimensions as the dynamics ABI names them
    double L = 512e3, alpha = 0, beta = 0;
    int nsub = 120, rowBlocks = 1, passesPerExchange = 2, loopbackWorld = 0;
    bool thermo = false, overlap = true, graph = false, m_inited = false;
    bool advectColumn = false; // dynamics.advect_column_state: the snow and the surface temperature ride on the ice
    bool closure = true; // ridging cap + scaling limiter in the transport, free drift at ice-free nodes (dynamics.closure)
    double deltaMin = 0; // dynamics.delta_min; 0: the literature's 2e-9 (keep_alpha: raised to what the mesh needs)
    std::string subcycle = "adaptive"; // dynamics.subcycle
    double minConc = 1e-12, minThick = 0.01; // ice-free-node rule (dynamics.min_conc / min_thick; the column model's cut-off values)
    std::string forcing = "host", devices;
    std::shared_ptr<const ForcingFile> m_forcingFile; // dynamics.forcing = file: the records, read and checked in configure()
    std::shared_ptr<const LandMaskFile> m_landMask; // dynamics.land_mask_file: the element mask, read and checked in configure()
    std::shared_ptr<const BathymetryFile> m_bathymetry; // dynamics.bathymetry_file: the water depth, read and checked in configure()
    nsdg_basal_params m_basal; // [basal]: the grounding scheme's parameters (used with m_bathymetry)
    bool slabOcean = false; // dynamics.slab_ocean: sst and sss follow the ice (nsdg_column_step_ocean)
    bool snowLoad = false; // dynamics.snow_load: the packing takes the nodal mass from ice and snow (nsdg_snow_load_set before every packing)
    double rhoSnow = NSDG_SNOW_DENSITY; // dynamics.rho_snow
    bool tiltSsh = false; // dynamics.tilt = ssh: the packing takes the tilt from the block's sea-surface height (nsdg_tilt_set before every packing)
    double gravity = NSDG_GRAVITY; // dynamics.gravity
    nsdg_slab_params m_slab; // [slabocean]: relaxation times and the salinity of the ice (used with slabOcean)
    struct Outputs; // model.output_*, series_*, drifters_*, stations_*: the four outputs, each null when off (DynamicsStep.cpp)
    std::unique_ptr<Outputs> m_out;
    struct Brittle; // dynamics.rheology = bbm: the parameters and the sub-iteration rule (DynamicsStep.cpp); null: mEVP
    std::unique_ptr<Brittle> m_brittle;
    std::vector<std::string> m_tracers; // dynamics.tracers: the names, in order
    std::vector<std::vector<double>> m_tracerInit; // dynamics.tracer_init: one plane per name (empty: zeros), read and checked in configure()
    bool nsubGiven = false; // dynamics.nsub is in the configuration
    int substeps = 1; // dynamics.substeps; 0 = auto
    double substepCourant = 1.5; // dynamics.substep_courant (NSDG_SUBSTEP_COURANT)
    int maxSubsteps = 16; // dynamics.max_substeps
    bool timing = false; // model.timing: one line whenever auto changes n
    bool phaseTiming = false; // model.phase_timing: the contexts time the step's phases with stream events (PhaseTiming.hpp)
    std::vector<std::string> m_iteratePath; // the timer node of iterate()
    long m_substepsRun = 0;
    int m_lastSubsteps = 0; // n of the previous model step (auto)
    int m_world = 1, m_rank = 0; // multi-process run (one block per process)
    long m_steps = 0;
    double m_time = 0; // model time of the next step [s]
    double m_umax = 0, m_sumH = 0, m_sumA = 0;
};

} // namespace Nextsim
