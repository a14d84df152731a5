#include "RectGrid.hpp"

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <fstream>
#include <map>
#include <set>
#include <sstream>
#include <stdexcept>

#include "DynamicsStep.hpp"
#include "Hdf5Subset.hpp"
#include "ModuleLoader.hpp"

namespace Nextsim {

void FieldStore::resize(std::size_t nElements, int nIceLayers)
{
    n = nElements;
    nLayers = nIceLayers;
    for (auto* v : { &hice, &cice, &hsnow, &sst, &sss, &tair, &tdew, &slp, &mixrat, &qsw, &qlw, &mld, &snowfall, &wind, &newice })
        v->assign(n, 0.);
    tice.assign(n * (std::size_t)nLayers, 0.);
    dyn.clear();
}

ElementData& ElementData::operator=(const PrognosticGenerator& g)
{
    iceThickness() = g.m_hice;
    iceConcentration() = g.m_cice;
    snowThickness() = g.m_hsnow;
    seaSurfaceTemperature() = g.m_sst;
    seaSurfaceSalinity() = g.m_sss;
    for (int l = 0; l < s->nLayers; ++l) // missing layers repeat the last given one (PrognosticData.cpp:82-94)
        iceTemperature(l) = g.m_tice.empty() ? 0. : g.m_tice[std::min<std::size_t>(l, g.m_tice.size() - 1)];
    return *this;
}

void DummyExternalData::setAll(IStructure& is)
{
    for (is.cursor = 0; is.cursor; ++is.cursor) {
        is.cursor->airTemperature() = -1;
        is.cursor->dewPoint2m() = -4;
        is.cursor->airPressure() = 1e5;
        is.cursor->mixingRatio() = -1.;
        is.cursor->incomingShortwave() = 0;
        is.cursor->incomingLongwave() = 311;
        is.cursor->mixedLayerDepth() = 10;
        is.cursor->snowfall() = 0;
    }
}

RectGrid::RectGrid()
    : m_nx(0)
    , m_ny(0)
    , m_current(&m_store, 0)
{
    resize(10, 10, 1);
}

void RectGrid::resize(int nx, int ny, int nLayers)
{
    if (nx <= 0 || ny <= 0 || nLayers <= 0)
        throw std::invalid_argument("RectGrid: nx, ny and nLayers must be positive");
    m_nx = nx;
    m_ny = ny;
    m_store.resize((std::size_t)nx * ny, nLayers);
    resetCursor();
}

template <> const std::map<int, std::string> Configured<RectGrid>::keyMap = { { 0, "rectgrid.nx" }, { 1, "rectgrid.ny" }, { 2, "rectgrid.nLayers" } };

void RectGrid::configure()
{
    const int nx = getConfiguration(keyMap.at(0), m_nx);
    const int ny = getConfiguration(keyMap.at(1), m_ny);
    const int nl = getConfiguration(keyMap.at(2), m_store.nLayers);
    if (nx != m_nx || ny != m_ny || nl != m_store.nLayers)
        resize(nx, ny, nl);
}

int RectGrid::resetCursor()
{
    m_cursor = 0;
    m_current = ElementData(&m_store, 0);
    return 0;
}

void RectGrid::incrCursor()
{
    ++m_cursor;
    m_current = ElementData(&m_store, m_cursor);
}

namespace {
const char* MAGIC = "NSDG-RESTART 1";
const std::string TRACER_FLAG = "data.tracer."; // sidecar header: data.tracer.<name>=1, one line per tracer plane, in file order
const std::string TRACER_DATASET = "tracer_"; // the dataset (HDF5) / the entry of variables= (sidecar) of a tracer: tracer_<name>
//! `on`: receives every other key of the header whose value is 1 (data.dynamics and the flags of the optional variables); `tracers`: the
//! names of the data.tracer.<name>=1 lines, in their order
bool readHeader(std::istream& f, std::string& type, int& nx, int& ny, int& nl, std::set<std::string>* on = nullptr,
    std::vector<std::string>* tracers = nullptr)
{
    std::string line;
    if (!std::getline(f, line) || line != MAGIC)
        return false;
    type.clear();
    nx = ny = nl = 0;
    while (std::getline(f, line) && line != "END-HEADER") {
        const auto eq = line.find('=');
        if (eq == std::string::npos)
            continue;
        const std::string k = line.substr(0, eq), v = line.substr(eq + 1);
        if (k == "structure.type")
            type = v;
        else if (k == "data.x")
            nx = std::stoi(v);
        else if (k == "data.y")
            ny = std::stoi(v);
        else if (k == "data.nLayers")
            nl = std::stoi(v);
        else if (tracers && v == "1" && k.compare(0, TRACER_FLAG.size(), TRACER_FLAG) == 0)
            tracers->push_back(k.substr(TRACER_FLAG.size()));
        else if (on && v == "1")
            on->insert(k);
    }
    return nx > 0 && ny > 0 && nl > 0;
}
} // namespace

std::string RectGrid::typeInFile(const std::string& filePath, bool throwOnError)
{
    if (Hdf5File::isHdf5(filePath)) { // the reference's NetCDF-4 layout: group "structure", attribute "type" (StructureFactory.cpp:46-58)
        try {
            return Hdf5File(filePath).stringAttribute("/" + metadataNodeName(), typeNodeName());
        } catch (const Hdf5Error&) {
            if (throwOnError)
                throw; // a corrupt or unsupported file must stop the run with the reader's message
            return std::string();
        }
    }
    std::ifstream f(filePath, std::ios::binary);
    std::string type;
    int a, b, c;
    return (f && readHeader(f, type, a, b, c)) ? type : std::string();
}

namespace {
const char* const PLANE_NAMES[5] = { "hice", "cice", "hsnow", "sst", "sss" }; // core/src/DevGridIO.cpp:35-40
const char* const DYNAMICS_FLAG = "data.dynamics"; // sidecar header: the variables of DYNAMICS_VARIABLES follow tice
// the named dimensions of each DynamicsVariable::Shape in an HDF5 file, slowest first (x, y: the grid's own)
const std::vector<const char*> SHAPE_DIMENSIONS[] = { { "dg2", "x", "y" }, { "stress8", "x", "y" }, { "x", "y" }, { "xnode", "ynode" }, { "dg2full", "x", "y" } };
// the variables of the dynamics state a file of `f` holds: all of them, the optional ones when they are not empty
bool written(const DynamicsVariable& v, const FieldStore& f) { return !v.optional() || !v.in(f).empty(); }
} // namespace

void RectGrid::dump(const std::string& filePath) const
{
    // tice is (x, y, nLayers) in the file, layer-major planes in memory
    std::vector<double> t(m_store.tice.size());
    for (std::size_t e = 0; e < m_store.n; ++e)
        for (int l = 0; l < m_store.nLayers; ++l)
            t[e * m_store.nLayers + l] = m_store.tice[(std::size_t)l * m_store.n + e];
    if (Hdf5File::hasHdf5Extension(filePath)) { // groups, names and dimensions of core/src/DevGridIO.cpp:150-201
        Hdf5Writer w;
        w.group("/" + metadataNodeName());
        w.stringAttribute("/" + metadataNodeName(), typeNodeName(), structureType());
        const std::string data = "/" + dataNodeName();
        w.group(data);
        // the named dimensions of core/src/DevGridIO.cpp:169-172 (NetCDF-4 stores them as HDF5 dimension scales)
        w.dimension(data, "x", (std::uint64_t)m_nx, 0);
        w.dimension(data, "y", (std::uint64_t)m_ny, 1);
        w.dimension(data, "nLayers", (std::uint64_t)m_store.nLayers, 2);
        const std::vector<double>* planes[5] = { &m_store.hice, &m_store.cice, &m_store.hsnow, &m_store.sst, &m_store.sss };
        for (int k = 0; k < 5; ++k) {
            w.dataset(data + "/" + PLANE_NAMES[k], { (std::uint64_t)m_nx, (std::uint64_t)m_ny }, *planes[k]);
            w.attachDimensions(data + "/" + PLANE_NAMES[k], { data + "/x", data + "/y" }); // DevGridIO.cpp:174-190
        }
        w.dataset(data + "/tice", { (std::uint64_t)m_nx, (std::uint64_t)m_ny, (std::uint64_t)m_store.nLayers }, t);
        w.attachDimensions(data + "/tice", { data + "/x", data + "/y", data + "/nLayers" }); // DevGridIO.cpp:192-201
        if (m_store.dyn.present) { // the state of the dynamics: further variables of the same group (DYNAMICS_VARIABLES)
            const std::uint64_t X = (std::uint64_t)m_nx, Y = (std::uint64_t)m_ny;
            const std::map<std::string, std::uint64_t> length = { { "x", X }, { "y", Y }, { "dg2", 5 }, { "stress8", 8 }, { "xnode", 2 * X + 1 }, { "ynode", 2 * Y + 1 }, { "dg2full", 6 } };
            int dimid = 3; // the further dimensions follow x, y, nLayers
            for (const char* d : { "dg2", "stress8", "xnode", "ynode" })
                w.dimension(data, d, length.at(d), dimid++);
            for (const DynamicsVariable& v : DYNAMICS_VARIABLES) // the dimension of the damage exists only in a file that holds it
                if (v.shape == DynamicsVariable::DG6 && written(v, m_store))
                    w.dimension(data, "dg2full", length.at("dg2full"), dimid++);
            for (const DynamicsVariable& v : DYNAMICS_VARIABLES) {
                if (!written(v, m_store))
                    continue;
                std::vector<std::uint64_t> dims;
                std::vector<std::string> scales;
                for (const char* d : SHAPE_DIMENSIONS[v.shape])
                    dims.push_back(length.at(d)), scales.push_back(data + "/" + d);
                w.dataset(data + "/" + v.name, dims, v.in(m_store));
                w.attachDimensions(data + "/" + v.name, scales);
            }
            for (const DynamicsState::NamedPlane& t : m_store.dyn.tracers) { // dynamics.tracers: one plane each
                w.dataset(data + "/" + TRACER_DATASET + t.name, { X, Y }, t.values);
                w.attachDimensions(data + "/" + TRACER_DATASET + t.name, { data + "/x", data + "/y" });
            }
        }
        w.write(filePath);
        return;
    }
    std::ofstream f(filePath, std::ios::binary);
    if (!f)
        throw std::runtime_error("cannot write restart file " + filePath);
    f << MAGIC << "\n"
      << metadataNodeName() << "." << typeNodeName() << "=" << structureType() << "\n"
      << dataNodeName() << ".x=" << m_nx << "\n"
      << dataNodeName() << ".y=" << m_ny << "\n"
      << dataNodeName() << ".nLayers=" << m_store.nLayers << "\n";
    std::string variables = "variables=hice,cice,hsnow,sst,sss,tice";
    if (m_store.dyn.present) { // its flag, the flags of its optional variables, and every name in the order the arrays follow
        f << DYNAMICS_FLAG << "=1\n";
        for (const DynamicsVariable& v : DYNAMICS_VARIABLES)
            if (written(v, m_store)) {
                if (v.optional())
                    f << v.sidecarFlag << "=1\n";
                variables += std::string(",") + v.name;
            }
        for (const DynamicsState::NamedPlane& t : m_store.dyn.tracers) {
            f << TRACER_FLAG << t.name << "=1\n";
            variables += "," + TRACER_DATASET + t.name;
        }
    }
    f << variables << "\nEND-HEADER\n";
    for (const auto* v : { &m_store.hice, &m_store.cice, &m_store.hsnow, &m_store.sst, &m_store.sss })
        f.write(reinterpret_cast<const char*>(v->data()), (std::streamsize)(v->size() * sizeof(double)));
    f.write(reinterpret_cast<const char*>(t.data()), (std::streamsize)(t.size() * sizeof(double)));
    if (m_store.dyn.present) {
        for (const DynamicsVariable& v : DYNAMICS_VARIABLES)
            if (written(v, m_store))
                f.write(reinterpret_cast<const char*>(v.in(m_store).data()), (std::streamsize)(v.in(m_store).size() * sizeof(double)));
        for (const DynamicsState::NamedPlane& t : m_store.dyn.tracers)
            f.write(reinterpret_cast<const char*>(t.values.data()), (std::streamsize)(t.values.size() * sizeof(double)));
    }
}

void RectGrid::init(const std::string& filePath)
{
    tryConfigure(*this);
    if (filePath.empty()) { // constants, defaults = run/dev_res.py:10-20 of the reference
        typedef Configured<RectGrid> C;
        const double hice = C::getConfiguration("init.hice", 0.1), cice = C::getConfiguration("init.cice", 0.5);
        const double hsnow = C::getConfiguration("init.hsnow", 0.0), sst = C::getConfiguration("init.sst", -1.0);
        const double sss = C::getConfiguration("init.sss", 32.0), tice = C::getConfiguration("init.tice", -1.0);
        for (cursor = 0; cursor; ++cursor)
            *cursor = PrognosticGenerator().hice(hice).cice(cice).hsnow(hsnow).sst(sst).sss(sss).tice({ tice });
        return;
    }
    if (Hdf5File::isHdf5(filePath)) {
        // NetCDF-4 restart file of the reference (core/src/DevGridIO.cpp:93-147): group "data", variables
        // hice, cice, hsnow, sst, sss (x, y) and tice (x, y, nLayers); the number of layers is taken from
        // the third dimension of tice (DevGridIO.cpp:97-99), element (i, j) has the linear index i*ny + j
        const Hdf5File h(filePath);
        const std::string g = "/" + dataNodeName() + "/";
        const std::vector<std::uint64_t> d = h.dims(g + "tice");
        if (d.size() != 3)
            throw std::runtime_error("restart file " + filePath + ": tice must have the dimensions (x, y, nLayers)");
        if (structureType() == "devgrid" && (d[0] != 10 || d[1] != 10))
            throw std::runtime_error("devgrid restart files must be 10x10");
        resize((int)d[0], (int)d[1], (int)d[2]);
        std::vector<double>* planes[5] = { &m_store.hice, &m_store.cice, &m_store.hsnow, &m_store.sst, &m_store.sss };
        for (int k = 0; k < 5; ++k) {
            std::vector<double> v = h.readDoubles(g + PLANE_NAMES[k]);
            if (v.size() != m_store.n)
                throw std::runtime_error("restart file " + filePath + ": " + PLANE_NAMES[k] + " does not have x*y elements");
            planes[k]->swap(v);
        }
        const std::vector<double> t = h.readDoubles(g + "tice");
        for (std::size_t e = 0; e < m_store.n; ++e)
            for (int l = 0; l < m_store.nLayers; ++l)
                m_store.tice[(std::size_t)l * m_store.n + e] = t[e * m_store.nLayers + l];
        const auto held = [&](const DynamicsVariable& v) { return h.exists(g + v.name); };
        if (std::any_of(std::begin(DYNAMICS_VARIABLES), std::end(DYNAMICS_VARIABLES), [&](const DynamicsVariable& v) { return !v.optional() && held(v); })) {
            // the state of a dynamics run (all of it or none of it); an optional variable the file does not hold stays empty
            m_store.dyn.resize((std::size_t)m_nx, (std::size_t)m_ny);
            for (const DynamicsVariable& v : DYNAMICS_VARIABLES) {
                if (v.optional() && !held(v))
                    continue;
                std::vector<double> a = h.readDoubles(g + v.name);
                if (a.size() != v.size((std::size_t)m_nx, (std::size_t)m_ny))
                    throw std::runtime_error("restart file " + filePath + ": " + v.name + " does not have the size the grid asks for");
                v.in(m_store).swap(a);
            }
            // the tracers the configuration names (DynamicsStep::tracerNames: the one reading of dynamics.tracers), in its order; one the
            // file does not hold is left out, one it holds beside them is not read
            for (const std::string& name : DynamicsStep::tracerNames(Configured<RectGrid>::getConfiguration("dynamics.tracers", std::string("")))) {
                if (!h.exists(g + TRACER_DATASET + name))
                    continue;
                std::vector<double> a = h.readDoubles(g + TRACER_DATASET + name);
                if (a.size() != m_store.n)
                    throw std::runtime_error("restart file " + filePath + ": " + TRACER_DATASET + name + " does not have x*y elements");
                m_store.dyn.tracers.push_back({ name, std::move(a) });
            }
            m_store.dyn.present = true;
        }
        resetCursor();
        return;
    }
    std::ifstream f(filePath, std::ios::binary);
    std::string type;
    int nx, ny, nl;
    std::set<std::string> on;
    std::vector<std::string> tracers;
    if (!f || !readHeader(f, type, nx, ny, nl, &on, &tracers))
        throw std::runtime_error("cannot read restart file " + filePath);
    if (structureType() == "devgrid" && (nx != 10 || ny != 10))
        throw std::runtime_error("devgrid restart files must be 10x10");
    resize(nx, ny, nl);
    for (auto* v : { &m_store.hice, &m_store.cice, &m_store.hsnow, &m_store.sst, &m_store.sss })
        f.read(reinterpret_cast<char*>(v->data()), (std::streamsize)(v->size() * sizeof(double)));
    std::vector<double> t(m_store.tice.size());
    f.read(reinterpret_cast<char*>(t.data()), (std::streamsize)(t.size() * sizeof(double)));
    if (on.count(DYNAMICS_FLAG)) {
        m_store.dyn.resize((std::size_t)nx, (std::size_t)ny);
        for (const DynamicsVariable& v : DYNAMICS_VARIABLES) {
            if (v.optional() && !on.count(v.sidecarFlag))
                continue; // stays empty
            v.in(m_store).resize(v.size((std::size_t)nx, (std::size_t)ny));
            f.read(reinterpret_cast<char*>(v.in(m_store).data()), (std::streamsize)(v.in(m_store).size() * sizeof(double)));
        }
        // as from an HDF5 file: the tracers the configuration names, in its order; the file's other tracer planes are passed over
        std::map<std::string, std::vector<double>> held;
        for (const std::string& name : tracers) {
            std::vector<double>& a = held[name];
            a.resize(m_store.n);
            f.read(reinterpret_cast<char*>(a.data()), (std::streamsize)(m_store.n * sizeof(double)));
        }
        for (const std::string& name : DynamicsStep::tracerNames(Configured<RectGrid>::getConfiguration("dynamics.tracers", std::string(""))))
            if (held.count(name))
                m_store.dyn.tracers.push_back({ name, std::move(held[name]) });
        m_store.dyn.present = true;
    }
    if (!f)
        throw std::runtime_error("restart file " + filePath + " is truncated");
    for (std::size_t e = 0; e < m_store.n; ++e)
        for (int l = 0; l < nl; ++l)
            m_store.tice[(std::size_t)l * m_store.n + e] = t[e * nl + l];
}

// registration order = default order: devgrid first, as in core/src/modules/modules.json:9-14
NSDG_REGISTER_MODULE(IStructure, DevGrid, "Nextsim::IStructure", "Nextsim::DevGrid");
NSDG_REGISTER_MODULE(IStructure, RectGrid, "Nextsim::IStructure", "Nextsim::RectGrid");

std::shared_ptr<IStructure> StructureFactory::generate(const std::string& structureName)
{
    ModuleLoader& loader = ModuleLoader::getLoader();
    for (const std::string& impl : loader.listImplementations("Nextsim::IStructure")) {
        loader.setImplementation("Nextsim::IStructure", impl);
        std::shared_ptr<IStructure> s(loader.getInstance<IStructure>().release());
        if (s->structureTypeCheck(structureName))
            return s;
    }
    throw std::invalid_argument("StructureFactory::generate: no structure type named " + structureName);
}

std::shared_ptr<IStructure> StructureFactory::generateFromFile(const std::string& filePath)
{
    {
        std::ifstream probe(filePath, std::ios::binary);
        if (!probe)
            throw std::runtime_error("StructureFactory::generateFromFile: cannot open " + filePath);
    }
    const std::string type = RectGrid::typeInFile(filePath, true);
    if (type.empty())
        throw std::invalid_argument("StructureFactory::generateFromFile: no structure type in " + filePath);
    return generate(type);
}

} // namespace Nextsim
