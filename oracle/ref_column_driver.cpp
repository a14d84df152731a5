// ref_column_driver.cpp -- TEST INFRASTRUCTURE.
//
// extern "C" driver around the reference's own column physics, compiled IN PLACE from the reference
// sources (oracle/Makefile, target ref_column: the source list of physics/test/CMakeLists.txt,
// testNextsimPhysics, unmodified, with the module-loader .ipp files the reference's
// core/src/modules/moduleloader_builder.py generates and the Boost stand-in in oracle/refshim/).
// Nothing from the reference is copied into this repository; the library goes to oracle/_ref/
// (git-ignored).  tools/gen_ref_column_golden.py records its outputs in tests/golden/ref_column_v1.npz.
//
// Per element it runs the body of DevStep::iterate (core/src/DevStep.cpp:17-22):
//     updateDerivedData -> NextsimPhysics::calculate -> PrognosticData::updateAndIntegrate
// through ElementData (the data) and one NextsimPhysics instance (the IPhysics1d the module loader
// hands ElementData, core/src/ElementData.cpp:22), as physics/test/NextsimPhysics_test.cpp does.
//
// Configuration goes through the reference's own Configurator / ModuleLoader / ConfiguredModule, so
// every key is read by the reference's own code.  HiblerConcentration::freeze latches 1/h0 in a
// function-local static on its first call (physics/src/modules/HiblerConcentration.cpp:36):
// configure a process once, or h0 silently keeps the first value.
#include "include/ConfiguredModule.hpp"
#include "include/Configurator.hpp"
#include "include/ElementData.hpp"
#include "include/ModuleLoader.hpp"
#include "include/NextsimPhysics.hpp"

#include <memory>
#include <sstream>
#include <vector>

namespace {

// m_Qow, the open-water heat flux, has no accessor in NextsimPhysics (NextsimPhysics.hpp:224).  An
// explicit template instantiation may name a private member ([temp.explicit]/12), which is how the
// driver reads it without touching the reference's sources.
template <typename Tag, typename Tag::type M> struct Rob {
    friend typename Tag::type get(Tag) { return M; }
};
struct QowTag {
    typedef double Nextsim::NextsimPhysics::*type;
    friend type get(QowTag);
};
template struct Rob<QowTag, &Nextsim::NextsimPhysics::m_Qow>;

// Order of abi.DIAG / oracle/column_oracle.h ORACLE_D_*: every one has a reference counterpart.
enum { D_RHO, D_QA, D_QW, D_QI, D_CSPEC, D_TAU, D_HI, D_HS, D_CNEW, D_QIA, D_QIO, D_SUBL, D_DQDT, D_HIFROMS, D_QOW, NDIAG };

bool g_configured = false;

struct Element {
    Nextsim::ElementData data;
    Nextsim::NextsimPhysics phys;
};

}

extern "C" {

// ini: the configuration text, e.g. "[Modules]\nNextsim::IIceAlbedo = Nextsim::CCSMIceAlbedo\n[Hibler]\nh0 = 0.5\n".
// Returns 0, -1 on any exception, -2 when called a second time in one process (the h0 latch).
int ref_column_configure(const char* ini)
{
    if (g_configured)
        return -2;
    try {
        Nextsim::Configurator::clearStreams();
        Nextsim::Configurator::addStream(std::unique_ptr<std::istream>(new std::stringstream(ini)));
        ModuleLoader::getLoader().setAllDefaults();
        Nextsim::ConfiguredModule::parseConfigurator();
        Nextsim::ElementData data;
        data.configure(); // PrognosticData (IFreezingPoint) + IPhysics1d -> the physics modules and their keys
        g_configured = true;
        return 0;
    } catch (...) {
        return -1;
    }
}

// nsteps steps of DevStep::iterate on n elements, each with its own persistent NextsimPhysics (so
// m_newice carries over as in the reference).  State arrays are in/out; newice is out (the element
// starts with the reference's m_newice = 0, NextsimPhysics.cpp:43-47); diag (NDIAG planes of n, or
// NULL) is of the last step; record (nsteps x 5 planes of n: hice, cice, hsnow, tice0, newice after
// each step, or NULL).  Forcing element e of step s is at index s * fstride + e: fstride = 0 holds it
// fixed, fstride = n reads nsteps planes (the only way a carried m_newice shows: with fixed forcing
// the open-water flux, and so the new-ice branch, is the same every step).  sst and sss go in through
// PrognosticData::setSeaSurface.  Returns 0, -1 on any exception, -3 when not configured.
int ref_column_run(long n, int nsteps, double dt, long fstride, double* hice, double* cice, double* hsnow, double* tice0,
    const double* sst, const double* sss, const double* tair, const double* tdew, const double* slp,
    const double* qsw, const double* qlw, const double* mld, const double* snowfall, const double* wind,
    double* newice, double* diag, double* record)
{
    if (!g_configured)
        return -3;
    try {
        Nextsim::PrognosticData::setTimestep(dt);
        std::vector<std::unique_ptr<Element>> el(n);
        for (long e = 0; e < n; ++e) {
            el[e].reset(new Element);
            Nextsim::ElementData& d = el[e]->data;
            d = Nextsim::PrognosticGenerator().hice(hice[e]).cice(cice[e]).hsnow(hsnow[e]).tice({ tice0[e] }).sst(sst[e]).sss(sss[e]);
        }
        for (int s = 0; s < nsteps; ++s) {
            for (long e = 0; e < n; ++e) {
                Nextsim::ElementData& d = el[e]->data;
                Nextsim::NextsimPhysics& p = el[e]->phys;
                const long f = s * fstride + e;
                d.setSeaSurface(sst[f], sss[f]);
                d.airTemperature() = tair[f];
                d.dewPoint2m() = tdew[f];
                d.airPressure() = slp[f];
                d.incomingShortwave() = qsw[f];
                d.incomingLongwave() = qlw[f];
                d.mixedLayerDepth() = mld[f];
                d.snowfall() = snowfall[f];
                d.windSpeed() = wind[f];
                p.updateDerivedData(d, d, d);
                p.calculate(d, d, d);
                d.updateAndIntegrate(d);
                hice[e] = d.iceThickness();
                cice[e] = d.iceConcentration();
                hsnow[e] = d.snowThickness();
                tice0[e] = d.iceTemperature(0);
                newice[e] = p.newIce();
                if (record) {
                    double* r = record + (size_t)s * 5 * n;
                    r[0 * n + e] = hice[e];
                    r[1 * n + e] = cice[e];
                    r[2 * n + e] = hsnow[e];
                    r[3 * n + e] = tice0[e];
                    r[4 * n + e] = newice[e];
                }
                if (diag && s == nsteps - 1) {
                    const double v[NDIAG] = { d.airDensity(), d.specificHumidityAir(), d.specificHumidityWater(),
                        d.specificHumidityIce(), d.heatCapacityWetAir(), d.dragPressure(), d.updatedIceTrueThickness(),
                        d.updatedSnowTrueThickness(), d.updatedIceConcentration(), p.QIceAtmosphere(), p.QIceOceanHeat(),
                        p.sublimationRate(), p.QDerivativeWRTTemperature(), p.totalIceFromSnow(), p.*get(QowTag()) };
                    for (int k = 0; k < NDIAG; ++k)
                        diag[(size_t)k * n + e] = v[k];
                }
            }
        }
        return 0;
    } catch (...) {
        return -1;
    }
}

}
