// ForcingFile.hpp -- forcing records read from a file for dynamics.forcing = file (DynamicsStep), sampled on the device by
// nsdg_forcing_sample (include/nsdg.h "forcing from a file").
//
// File layout (HDF5, the subset Hdf5Subset reads; host/build/make_forcing writes it from .npy arrays), root-level datasets:
//     time                                  (nt)            model seconds, the clock of model.start; strictly increasing
//     tair tdew slp qsw qlw mld snowfall    (nt, nyr, nxr)  the column forcing planes, units of the structure's planes
//     wind_u wind_v, ocean_u ocean_v        (nt, nyr, nxr)  optional, each pair complete or absent [m/s]
//     sst sss                               (nt, nyr, nxr)  optional, a pair: the relaxation targets of dynamics.slab_ocean [deg C, psu]
//     ssh                                   (nt, nyr, nxr)  optional: the sea-surface height of dynamics.tilt = ssh [m]
// All variables share one lattice: cell-centred over the model's square domain, point i at x / L = (i + 1/2) / nxr.  There are
// no coordinate variables: lon/lat or other lattices, chunked or compressed datasets and unknown variables are refused.
// Every check happens when the file is opened, before a device is touched; each error names the file, the variable and the
// record or index.
#pragma once
#include <cstddef>
#include <map>
#include <string>
#include <vector>

namespace Nextsim {

class ForcingFile {
public:
    static const std::vector<std::string>& columnVariables(); //!< tair tdew slp qsw qlw mld snowfall
    static const std::vector<std::string>& knownVariables(); //!< the column variables, wind_u wind_v, ocean_u ocean_v, sst sss, ssh

    //! Reads and checks the file; needColumn: the seven column variables must be present (dynamics.thermodynamics = true).
    //! Throws std::runtime_error naming the file.
    ForcingFile(const std::string& path, bool needColumn);

    const std::string& path() const { return m_path; }
    std::size_t records() const { return m_time.size(); }
    const std::vector<double>& times() const { return m_time; }
    int nxr() const { return m_nxr; }
    int nyr() const { return m_nyr; }
    bool has(const std::string& var) const { return m_vars.count(var) != 0; }
    bool hasColumn() const;
    bool hasWind() const { return has("wind_u"); }
    bool hasOcean() const { return has("ocean_u"); }
    bool hasSlabTargets() const { return has("sst"); } //!< the pair sst, sss
    bool hasSsh() const { return has("ssh"); } //!< the sea-surface height of dynamics.tilt = ssh
    std::vector<std::string> variables() const; //!< present variables, in the order of knownVariables()

    //! The records around model time t: k0 = the last record with time[k0] <= t, k1 = k0 + 1, w = (t - time[k0]) / (time[k1] - time[k0]);
    //! at the last record itself k1 = k0 and w = 0.  A t outside [time[0], time[nt - 1]] throws: there is no extrapolation.
    void bracket(double t, std::size_t& k0, std::size_t& k1, double& w) const;
    //! record k of a variable: nyr x nxr values, x fastest
    const double* record(const std::string& var, std::size_t k) const;

private:
    std::string m_path;
    std::vector<double> m_time;
    int m_nxr = 0, m_nyr = 0;
    std::map<std::string, std::vector<double>> m_vars;
};

} // namespace Nextsim
