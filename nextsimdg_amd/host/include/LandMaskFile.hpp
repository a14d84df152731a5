// LandMaskFile.hpp -- the land mask of dynamics.land_mask_file (DynamicsStep; include/nsdg.h "land mask"): a .npy array of uint8 or
// bool, one value per element, 1 = land, 0 = ocean, of the shape of the structure's planes -- (rectgrid.nx, rectgrid.ny), the second
// index fastest, the order of the restart file.  The nodes of land elements hold u = v = 0 (a no-slip coast); H, A and the column
// state are kept at 0 there.  The mask is configuration: the restart file holds no copy, a resumed run names the same file.
// Every check happens when the file is opened, before a device is touched; each error names the key and the file.  Header-only.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "NpyFile.hpp"

namespace Nextsim {

class LandMaskFile {
public:
    //! Reads and checks the file: a two-dimensional uint8 / bool array of zeros and ones.  Throws std::runtime_error.
    explicit LandMaskFile(const std::string& path)
        : m_path(path)
    {
        const std::string where = "dynamics.land_mask_file " + path + ": ";
        NpyRaw raw;
        try {
            raw = readNpyRaw(path, [](const std::string& descr, const std::string&) -> std::size_t {
                if (descr != "|u1" && descr != "|b1" && descr != "u1" && descr != "b1" && descr != "<u1" && descr != "?")
                    throw std::runtime_error("the mask must be uint8 ('|u1') or bool ('|b1'), the header says '" + descr + "'");
                return 1;
            });
        } catch (const std::exception& e) {
            throw std::runtime_error(where + e.what());
        }
        if (raw.shape.size() != 2 || raw.shape[0] < 1 || raw.shape[1] < 1)
            throw std::runtime_error(where + "the mask must be two-dimensional, it has " + std::to_string(raw.shape.size()) + " dimension(s)");
        m_rows = raw.shape[0], m_cols = raw.shape[1];
        m_mask.resize(raw.data.size());
        for (std::size_t i = 0; i < m_mask.size(); ++i) {
            const unsigned v = (unsigned char)raw.data[i];
            if (v > 1)
                throw std::runtime_error(where + "value " + std::to_string(v) + " at (" + std::to_string(i / m_cols) + ", " + std::to_string(i % m_cols)
                    + "): the mask holds 1 (land) and 0 (ocean) only");
            m_mask[i] = (std::uint8_t)v;
            m_land += v;
        }
    }
    //! Throws unless the mask has `rows` x `cols` values (the structure's slow and fast dimensions).
    void checkShape(std::size_t rows, std::size_t cols) const
    {
        if (m_rows != rows || m_cols != cols)
            throw std::runtime_error("dynamics.land_mask_file " + m_path + ": the mask has the shape (" + std::to_string(m_rows) + ", " + std::to_string(m_cols)
                + "), the grid (rectgrid.nx, rectgrid.ny) = (" + std::to_string(rows) + ", " + std::to_string(cols) + ")");
    }
    const std::string& path() const { return m_path; }
    std::size_t rows() const { return m_rows; }
    std::size_t cols() const { return m_cols; }
    std::size_t landElements() const { return m_land; }
    const std::uint8_t* data() const { return m_mask.data(); } //!< rows x cols, the column index fastest

private:
    std::string m_path;
    std::size_t m_rows = 0, m_cols = 0, m_land = 0;
    std::vector<std::uint8_t> m_mask;
};

} // namespace Nextsim
