// NpyFile.hpp -- reader of .npy arrays (format versions 1-3, little-endian or single-byte items, C order): what make_forcing builds a
// forcing file from (float64) and what dynamics.land_mask_file names (uint8 or bool; LandMaskFile.hpp).  Header-only.
#pragma once
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <stdexcept>
#include <string>
#include <vector>

namespace Nextsim {

struct NpyRaw {
    std::string descr; //!< the header's descr without its quotes, e.g. "<f8", "|u1", "|b1"
    std::vector<std::uint64_t> shape;
    std::vector<char> data; //!< the items, C order
};

struct Npy {
    std::vector<std::uint64_t> shape;
    std::vector<double> values;
};

//! header and bytes of a .npy file; itemSize: bytes per item of the descr the caller accepts (the data length is checked against it)
inline NpyRaw readNpyRaw(const std::string& path, std::size_t (*itemSize)(const std::string& descr, const std::string& path))
{
    std::ifstream f(path, std::ios::binary);
    if (!f)
        throw std::runtime_error("cannot open " + path);
    const std::vector<char> b((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    if (b.size() < 10 || std::memcmp(b.data(), "\x93NUMPY", 6) != 0)
        throw std::runtime_error(path + " is not a .npy file");
    const int major = (unsigned char)b[6];
    std::size_t hlen = 0, start = 0;
    if (major == 1) {
        hlen = (unsigned char)b[8] | ((std::size_t)(unsigned char)b[9] << 8), start = 10;
    } else if (major == 2 || major == 3) {
        if (b.size() < 12)
            throw std::runtime_error(path + ": truncated header");
        for (int i = 0; i < 4; ++i)
            hlen |= (std::size_t)(unsigned char)b[8 + i] << (8 * i);
        start = 12;
    } else
        throw std::runtime_error(path + ": .npy format version " + std::to_string(major) + " is not supported");
    if (start + hlen > b.size())
        throw std::runtime_error(path + ": truncated header");
    const std::string h(b.data() + start, hlen);
    auto value = [&](const std::string& key) {
        const std::size_t k = h.find("'" + key + "'");
        if (k == std::string::npos)
            throw std::runtime_error(path + ": no " + key + " in the header");
        std::size_t p = h.find(':', k);
        while (p + 1 < h.size() && h[p + 1] == ' ')
            ++p;
        return p + 1;
    };
    NpyRaw out;
    const std::size_t d = value("descr");
    const std::size_t dq = d < h.size() && h[d] == '\'' ? h.find('\'', d + 1) : std::string::npos;
    if (dq == std::string::npos)
        throw std::runtime_error(path + ": unreadable descr (structured arrays are not supported)");
    out.descr = h.substr(d + 1, dq - d - 1);
    const std::size_t item = itemSize(out.descr, path);
    if (h.compare(value("fortran_order"), 5, "False") != 0)
        throw std::runtime_error(path + ": the array must be in C order");
    const std::size_t s = value("shape");
    const std::size_t e = h.find(')', s);
    if (h[s] != '(' || e == std::string::npos)
        throw std::runtime_error(path + ": unreadable shape");
    std::uint64_t n = 1;
    for (std::size_t p = s + 1; p < e;) {
        while (p < e && (h[p] == ' ' || h[p] == ','))
            ++p;
        if (p >= e)
            break;
        char* end = nullptr;
        const unsigned long long v = std::strtoull(h.c_str() + p, &end, 10);
        if (end == h.c_str() + p)
            throw std::runtime_error(path + ": unreadable shape");
        out.shape.push_back(v);
        n *= v;
        p = end - h.c_str();
    }
    const std::size_t data = start + hlen;
    if (b.size() - data != n * item)
        throw std::runtime_error(path + ": " + std::to_string(b.size() - data) + " bytes of data for " + std::to_string(n) + " items of " + std::to_string(item) + " byte(s)");
    out.data.assign(b.begin() + data, b.end());
    return out;
}

//! a float64 .npy file
inline Npy readNpy(const std::string& path)
{
    const NpyRaw raw = readNpyRaw(path, [](const std::string& descr, const std::string& p) -> std::size_t {
        if (descr != "<f8" && descr != "f8")
            throw std::runtime_error(p + ": the array must be float64 ('<f8'), the header says '" + descr + "'");
        return sizeof(double);
    });
    Npy out;
    out.shape = raw.shape;
    out.values.resize(raw.data.size() / sizeof(double));
    std::memcpy(out.values.data(), raw.data.data(), raw.data.size());
    return out;
}

} // namespace Nextsim
