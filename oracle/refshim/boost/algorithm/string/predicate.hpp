// refshim/boost/algorithm/string/predicate.hpp -- TEST INFRASTRUCTURE.
//
// Stand-in for the one function of <boost/algorithm/string/predicate.hpp> the reference calls
// (core/src/modules/include/IStructure.hpp:57): case-insensitive string equality.  Written for
// this repository; only used to compile the reference's column physics into oracle/_ref/.
#ifndef REFSHIM_BOOST_ALGORITHM_STRING_PREDICATE_HPP
#define REFSHIM_BOOST_ALGORITHM_STRING_PREDICATE_HPP

#include <cctype>
#include <string>

namespace boost {
namespace algorithm {

    inline bool iequals(const std::string& a, const std::string& b)
    {
        if (a.size() != b.size())
            return false;
        for (std::size_t i = 0; i < a.size(); ++i)
            if (std::tolower(static_cast<unsigned char>(a[i])) != std::tolower(static_cast<unsigned char>(b[i])))
                return false;
        return true;
    }

} // namespace algorithm
} // namespace boost

#endif
