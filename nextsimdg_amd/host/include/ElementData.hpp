// ElementData.hpp -- per-element view of the structure's fields.
//
// The reference stores one heap-allocated ElementData object per element (array of structs:
// core/src/include/ElementData.hpp:30-68 = PrognosticData + PhysicsData + ExternalData, ~0.5 KB each).
// Here the fields live in flat struct-of-arrays planes (FieldStore) that are copied to HBM as they
// are; ElementData is a light proxy (store pointer + index) that offers the reference's accessor
// names, so host code written against the reference (e.g. DummyExternalData::setAll,
// core/src/include/DummyExternalData.hpp:22-34, or the tests' PrognosticGenerator chains) reads the
// same.
#pragma once
#include <cstddef>
#include <string>
#include <vector>

namespace Nextsim {

//! What a dynamics run carries from one step to the next beyond the cell means hice / cice of the FieldStore: the higher DG2 coefficients of
//! the advected thickness and concentration, the CG2 velocity and the 24 stress coefficients.  The reference writes every prognostic field
//! it has into its restart file (core/src/DevGridIO.cpp:169-201, read back at :101-138); its snapshot has no dynamics, so these are
//! additional variables of the same group (DYNAMICS_VARIABLES below).  x = the slow index of the file, y the fast one.
struct DynamicsState {
    bool present = false; //!< false: a run starts from rest with piecewise-constant fields (a file of the reference, or of a column-only run)
    std::vector<double> hdg, adg; //!< coefficients 1..5 of H and A: [5][x][y]
    std::vector<double> u, v; //!< nodal velocity on the (2x+1) x (2y+1) lattice
    std::vector<double> s11, s12, s22; //!< stress coefficients: [8][x][y]
    //! coefficients 1..5 of the snow S of dynamics.advect_column_state: [5][x][y]; EMPTY without that mode (nothing of it is written)
    //! and after reading a file that does not hold it (the higher coefficients then start at zero)
    std::vector<double> sdg;
    //! all six coefficients of the damage D of dynamics.rheology = bbm: [6][x][y] (no FieldStore plane holds its mean); EMPTY without that
    //! rheology and after reading a file that does not hold it (a brittle run then starts undamaged)
    std::vector<double> damage;
    //! the ice tracers of dynamics.tracers, in the order of that key: one plane [x][y] each (include/nsdg.h "ice tracers"), dataset
    //! `tracer_<name>` of a restart file; EMPTY without the key, and a file's planes that the key does not name are not kept (either format)
    struct NamedPlane {
        std::string name;
        std::vector<double> values;
    };
    std::vector<NamedPlane> tracers;
    inline void resize(std::size_t nx, std::size_t ny); //!< every variable that is not optional: zeros of its shape
    inline void clear();
};

//! Struct-of-arrays field container: every plane has n = nx*ny doubles, element index i*ny' ... see IStructure.
struct FieldStore {
    std::size_t n = 0;
    int nLayers = 1;
    // prognostic (core/src/include/PrognosticData.hpp:86-92)
    std::vector<double> hice, cice, hsnow, sst, sss;
    std::vector<double> tice; // nLayers planes: tice[l*n + e]
    // external forcing (core/src/include/ExternalData.hpp:66-74)
    std::vector<double> tair, tdew, slp, mixrat, qsw, qlw, mld, snowfall;
    // physics input / persistent state (physics/src/include/PhysicsData.hpp:26; NextsimPhysics.hpp m_newice)
    std::vector<double> wind, newice;
    // state of the dynamics between two steps (absent until a dynamics run has stopped, or a restart file that holds it was read)
    DynamicsState dyn;

    void resize(std::size_t nElements, int nIceLayers);
};

//! One variable a restart file holds for a dynamics run beyond the reference's own hice .. tice.  The table below states them ONCE, in file
//! order: DynamicsState::resize / clear, both file formats (RectGrid::dump / init) and the ranks' payload (DynamicsStep::packRows) walk it.
struct DynamicsVariable {
    //! for x * y elements: DG2 coefficients 1..5 of an advected field (dg2 = 5, x, y) | the 8-function stress space (stress8 = 8, x, y) |
    //! a plane (x, y) | the CG2 lattice (xnode = 2x+1, ynode = 2y+1) | all six DG2 coefficients of a field without a mean plane (dg2full = 6, x, y); in
    //! brackets the named dimensions of an HDF5 file
    enum Shape { DG5, STRESS8, PLANE, NODAL, DG6 };
    const char* name; //!< the dataset in group `data` of an HDF5 file = the entry of the sidecar's variables= line
    Shape shape;
    //! where it lives: in FieldStore::dyn, or (state == nullptr) in a plane of the FieldStore itself, which the files list here but which
    //! is not DynamicsState's -- between the ranks it travels with the cell means (DynamicsStep::packRows), never again with the state
    std::vector<double> DynamicsState::*state;
    std::vector<double> FieldStore::*plane;
    //! nullptr: every file with the state holds it.  Otherwise it is OPTIONAL -- written when it is not empty, empty after a file without
    //! it -- and this sidecar header key announces it (an HDF5 file shows it by the dataset itself)
    const char* sidecarFlag;

    template <class Store> auto& in(Store& f) const { return state ? f.dyn.*state : f.*plane; } //!< its array in a (const) FieldStore
    bool optional() const { return sidecarFlag != nullptr; }
    int elementPlanes() const { return shape == DG5 ? 5 : shape == DG6 ? 6 : shape == STRESS8 ? 8 : shape == PLANE ? 1 : 0; } //!< planes of x * y values
    std::size_t size(std::size_t nx, std::size_t ny) const { return shape == NODAL ? (2 * nx + 1) * (2 * ny + 1) : elementPlanes() * nx * ny; }
};
inline constexpr DynamicsVariable DYNAMICS_VARIABLES[] = {
    { "hice_dg", DynamicsVariable::DG5, &DynamicsState::hdg, nullptr, nullptr }, // the advected thickness (coefficient 0 = hice)
    { "cice_dg", DynamicsVariable::DG5, &DynamicsState::adg, nullptr, nullptr }, // the advected concentration (coefficient 0 = cice)
    { "u", DynamicsVariable::NODAL, &DynamicsState::u, nullptr, nullptr },
    { "v", DynamicsVariable::NODAL, &DynamicsState::v, nullptr, nullptr },
    { "s11", DynamicsVariable::STRESS8, &DynamicsState::s11, nullptr, nullptr },
    { "s12", DynamicsVariable::STRESS8, &DynamicsState::s12, nullptr, nullptr },
    { "s22", DynamicsVariable::STRESS8, &DynamicsState::s22, nullptr, nullptr },
    { "newice", DynamicsVariable::PLANE, nullptr, &FieldStore::newice, nullptr }, // the column model's new-ice volume (NextsimPhysics::m_newice)
    { "hsnow_dg", DynamicsVariable::DG5, &DynamicsState::sdg, nullptr, "data.snow_dg" }, // dynamics.advect_column_state: the advected snow (coefficient 0 = hsnow)
    { "damage", DynamicsVariable::DG6, &DynamicsState::damage, nullptr, "data.damage" }, // dynamics.rheology = bbm: the damage D, all six coefficients
};

void DynamicsState::resize(std::size_t nx, std::size_t ny)
{
    for (const DynamicsVariable& v : DYNAMICS_VARIABLES)
        if (v.state && !v.optional())
            (this->*v.state).assign(v.size(nx, ny), 0.);
}
void DynamicsState::clear()
{
    present = false;
    for (const DynamicsVariable& v : DYNAMICS_VARIABLES)
        if (v.state)
            (this->*v.state).clear();
    tracers.clear();
}

//! Builder with the reference's method names (core/src/include/PrognosticGenerator.hpp:17-90).
class PrognosticGenerator {
public:
    PrognosticGenerator& hice(double v) { m_hice = v; return *this; }
    PrognosticGenerator& cice(double v) { m_cice = v; return *this; }
    PrognosticGenerator& hsnow(double v) { m_hsnow = v; return *this; }
    PrognosticGenerator& sst(double v) { m_sst = v; return *this; }
    PrognosticGenerator& sss(double v) { m_sss = v; return *this; }
    PrognosticGenerator& tice(const std::vector<double>& v) { m_tice = v; return *this; }
    double m_hice = 0, m_cice = 0, m_hsnow = 0, m_sst = 0, m_sss = 0;
    std::vector<double> m_tice;
};

class ElementData {
public:
    ElementData(FieldStore* store, std::size_t index)
        : s(store)
        , e(index)
    {
    }
    ElementData& operator=(const PrognosticGenerator& g);

    // PrognosticData surface
    double& iceThickness() { return s->hice[e]; }
    double& iceConcentration() { return s->cice[e]; }
    double& snowThickness() { return s->hsnow[e]; }
    double& seaSurfaceTemperature() { return s->sst[e]; }
    double& seaSurfaceSalinity() { return s->sss[e]; }
    double& iceTemperature(int layer) { return s->tice[(std::size_t)layer * s->n + e]; }
    double iceTrueThickness() const { return s->cice[e] != 0 ? s->hice[e] / s->cice[e] : 0; } // PrognosticData.hpp:56
    double snowTrueThickness() const { return s->cice[e] != 0 ? s->hsnow[e] / s->cice[e] : 0; } // :75
    int nIceLayers() const { return s->nLayers; }
    // ExternalData surface
    double& airTemperature() { return s->tair[e]; }
    double& dewPoint2m() { return s->tdew[e]; }
    double& airPressure() { return s->slp[e]; }
    double& mixingRatio() { return s->mixrat[e]; }
    double& incomingShortwave() { return s->qsw[e]; }
    double& incomingLongwave() { return s->qlw[e]; }
    double& mixedLayerDepth() { return s->mld[e]; }
    double& snowfall() { return s->snowfall[e]; }
    double mixedLayerBulkHeatCapacity() const { return s->mld[e] * 1025. * 4186.84; } // ExternalData.hpp:60
    // PhysicsData surface (input only; derived quantities live in registers on the GPU)
    double& windSpeed() { return s->wind[e]; }
    double& newIce() { return s->newice[e]; }

    std::size_t index() const { return e; }

private:
    FieldStore* s;
    std::size_t e;
};

} // namespace Nextsim
