// BathymetryFile.hpp -- the water depth of dynamics.bathymetry_file (DynamicsStep; include/nsdg_basal.h): a .npy
// array of float64, one depth in metres per element, of the shape of the structure's planes -- (rectgrid.nx, rectgrid.ny), the second
// index fastest, the order of the restart file and of dynamics.land_mask_file.  Ice whose keels reach the seabed feels a basal stress and
// stays fast over a shoal.  The depth must be finite and >= 0 at ocean elements; what stands on land is not looked at and stored as 0.
// The depth is configuration, as the mask is: the restart file holds no copy, a resumed run names the same file.
// Every check happens before a device is touched; each error names the key, the file and the first offending element.  Header-only.
#pragma once
#include <cmath>
#include <cstdint>
#include <sstream>
#include <string>
#include <vector>

#include "LandMaskFile.hpp"
#include "NpyFile.hpp"

namespace Nextsim {

class BathymetryFile {
public:
    //! Reads the file, a two-dimensional float64 array, and checks its values where `mask` (null: no land) says ocean.
    //! Throws std::runtime_error.
    BathymetryFile(const std::string& path, const LandMaskFile* mask)
        : m_path(path)
    {
        const std::string where = "dynamics.bathymetry_file " + path + ": ";
        Npy a;
        try {
            a = readNpy(path);
        } catch (const std::exception& e) {
            throw std::runtime_error(where + e.what());
        }
        if (a.shape.size() != 2 || a.shape[0] < 1 || a.shape[1] < 1)
            throw std::runtime_error(where + "the depth must be two-dimensional, it has " + std::to_string(a.shape.size()) + " dimension(s)");
        m_rows = a.shape[0], m_cols = a.shape[1];
        if (mask && (mask->rows() != m_rows || mask->cols() != m_cols))
            throw std::runtime_error(where + "the depth has the shape (" + std::to_string(m_rows) + ", " + std::to_string(m_cols)
                + "), the mask of dynamics.land_mask_file (" + std::to_string(mask->rows()) + ", " + std::to_string(mask->cols()) + ")");
        m_depth = std::move(a.values);
        for (std::size_t i = 0; i < m_depth.size(); ++i) {
            if (mask && mask->data()[i]) {
                m_depth[i] = 0.; // land: stored as 0
                continue;
            }
            if (!(std::isfinite(m_depth[i]) && m_depth[i] >= 0.)) {
                std::ostringstream v;
                v << m_depth[i];
                throw std::runtime_error(where + "value " + v.str() + " at (" + std::to_string(i / m_cols) + ", " + std::to_string(i % m_cols)
                    + "): the depth must be finite and >= 0 at ocean elements");
            }
            m_shallowest = (m_ocean++ == 0) ? m_depth[i] : std::fmin(m_shallowest, m_depth[i]);
        }
    }
    //! Throws unless the array has `rows` x `cols` values (the structure's slow and fast dimensions).
    void checkShape(std::size_t rows, std::size_t cols) const
    {
        if (m_rows != rows || m_cols != cols)
            throw std::runtime_error("dynamics.bathymetry_file " + m_path + ": the depth has the shape (" + std::to_string(m_rows) + ", "
                + std::to_string(m_cols) + "), the grid (rectgrid.nx, rectgrid.ny) = (" + std::to_string(rows) + ", " + std::to_string(cols) + ")");
    }
    const std::string& path() const { return m_path; }
    std::size_t rows() const { return m_rows; }
    std::size_t cols() const { return m_cols; }
    double shallowest() const { return m_shallowest; } //!< the smallest depth of an ocean element
    const double* data() const { return m_depth.data(); } //!< rows x cols, the column index fastest; 0 on land

private:
    std::string m_path;
    std::size_t m_rows = 0, m_cols = 0, m_ocean = 0;
    double m_shallowest = 0.;
    std::vector<double> m_depth;
};

} // namespace Nextsim
