// refshim/boost/program_options.hpp -- TEST INFRASTRUCTURE.
//
// Stand-in for the part of <boost/program_options.hpp> the reference's configuration path calls
// (core/src/include/Configured.hpp:76-123, core/src/Configurator.cpp:18-55,
// core/src/ConfiguredModule.cpp:24-34), written for this repository.  Only used to compile the
// reference's column physics into oracle/_ref/libref_column.so (oracle/Makefile, ref_column).
//
// Semantics kept from the documented library: store() never replaces a value that was given
// explicitly (first source wins) but does replace a default; an option absent from every source
// takes its default_value(); a config file is INI text, "[section]" prefixes "section." to the keys
// below it, '#' starts a comment; unregistered keys are skipped when allowed.  Values convert from
// text with the C library (strtod / strtol); bool accepts true/false, yes/no, on/off, 1/0.
#ifndef REFSHIM_BOOST_PROGRAM_OPTIONS_HPP
#define REFSHIM_BOOST_PROGRAM_OPTIONS_HPP

#include <any>
#include <cstdlib>
#include <istream>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

namespace boost {
namespace program_options {

    class error : public std::logic_error {
    public:
        explicit error(const std::string& what)
            : std::logic_error(what)
        {
        }
    };

    class validation_error : public error {
    public:
        enum kind_t { multiple_values_not_allowed = 30, at_least_one_value_required, invalid_bool_value, invalid_option_value, invalid_option };
        explicit validation_error(kind_t kind, const std::string& = "", const std::string& = "", int = 0)
            : error("validation error")
            , m_kind(kind)
        {
        }
        kind_t kind() const { return m_kind; }

    private:
        kind_t m_kind;
    };

    namespace command_line_style {
        enum style_t { unix_style = 1 };
    }

    namespace detail {
        inline std::string trim(const std::string& s)
        {
            const char* ws = " \t\r\n";
            std::size_t b = s.find_first_not_of(ws);
            if (b == std::string::npos)
                return "";
            return s.substr(b, s.find_last_not_of(ws) - b + 1);
        }
        inline void from_text(const std::string& s, std::string& out) { out = s; }
        inline void from_text(const std::string& s, double& out)
        {
            char* end = nullptr;
            out = std::strtod(s.c_str(), &end);
            if (s.empty() || *end)
                throw validation_error(validation_error::invalid_option_value);
        }
        inline void from_text(const std::string& s, int& out)
        {
            char* end = nullptr;
            out = static_cast<int>(std::strtol(s.c_str(), &end, 10));
            if (s.empty() || *end)
                throw validation_error(validation_error::invalid_option_value);
        }
        inline void from_text(const std::string& s, bool& out)
        {
            if (s == "true" || s == "yes" || s == "on" || s == "1")
                out = true;
            else if (s == "false" || s == "no" || s == "off" || s == "0")
                out = false;
            else
                throw validation_error(validation_error::invalid_bool_value);
        }
    } // namespace detail

    class value_semantic {
    public:
        virtual ~value_semantic() = default;
        virtual bool apply_default(std::any& out) const = 0;
        virtual std::any parse(const std::vector<std::string>& tokens) const = 0;
    };

    template <typename T> class typed_value : public value_semantic {
    public:
        typed_value* default_value(const T& v)
        {
            m_default = v;
            m_hasDefault = true;
            return this;
        }
        typed_value* multitoken() { return this; }
        bool apply_default(std::any& out) const override
        {
            if (m_hasDefault)
                out = m_default;
            return m_hasDefault;
        }
        std::any parse(const std::vector<std::string>& tokens) const override
        {
            T v {};
            detail::from_text(tokens.back(), v);
            return v;
        }

    private:
        T m_default {};
        bool m_hasDefault = false;
    };

    template <typename T> class typed_value<std::vector<T>> : public value_semantic {
    public:
        typed_value* multitoken() { return this; }
        bool apply_default(std::any&) const override { return false; }
        std::any parse(const std::vector<std::string>& tokens) const override
        {
            std::vector<T> v(tokens.size());
            for (std::size_t i = 0; i < tokens.size(); ++i)
                detail::from_text(tokens[i], v[i]);
            return v;
        }
    };

    template <typename T> typed_value<T>* value() { return new typed_value<T>(); }

    class options_description {
    public:
        options_description() = default;
        explicit options_description(const std::string&) { }

        class easy_init {
        public:
            explicit easy_init(options_description* o)
                : m_owner(o)
            {
            }
            easy_init& operator()(const char* name, const value_semantic* s, const char* = "")
            {
                m_owner->m_options[name] = std::shared_ptr<const value_semantic>(s);
                return *this;
            }

        private:
            options_description* m_owner;
        };
        easy_init add_options() { return easy_init(this); }

        const value_semantic* find(const std::string& name) const
        {
            auto it = m_options.find(name);
            return it == m_options.end() ? nullptr : it->second.get();
        }
        const std::map<std::string, std::shared_ptr<const value_semantic>>& options() const { return m_options; }

    private:
        std::map<std::string, std::shared_ptr<const value_semantic>> m_options;
    };

    struct option {
        std::string string_key;
        std::vector<std::string> value;
    };

    struct parsed_options {
        explicit parsed_options(const options_description* d)
            : description(d)
        {
        }
        std::vector<option> options;
        const options_description* description;
    };

    class variable_value {
    public:
        variable_value() = default;
        variable_value(const std::any& v, bool defaulted)
            : m_value(v)
            , m_defaulted(defaulted)
        {
        }
        template <typename T> const T& as() const { return std::any_cast<const T&>(m_value); }
        bool empty() const { return !m_value.has_value(); }
        bool defaulted() const { return m_defaulted; }

    private:
        std::any m_value;
        bool m_defaulted = false;
    };

    class variables_map : public std::map<std::string, variable_value> {
    public:
        const variable_value& operator[](const std::string& name) const
        {
            static const variable_value none;
            auto it = find(name);
            return it == end() ? none : it->second;
        }
    };

    // Explicit values replace absent or defaulted ones only; then every still-absent option with a default gets it.
    inline void store(const parsed_options& parsed, variables_map& vm)
    {
        for (const option& o : parsed.options) {
            const value_semantic* s = parsed.description->find(o.string_key);
            if (!s)
                continue;
            auto it = vm.find(o.string_key);
            if (it != vm.end() && !it->second.defaulted())
                continue;
            vm.insert_or_assign(o.string_key, variable_value(s->parse(o.value), false));
        }
        for (const auto& kv : parsed.description->options()) {
            if (vm.find(kv.first) != vm.end())
                continue;
            std::any d;
            if (kv.second->apply_default(d))
                vm.insert_or_assign(kv.first, variable_value(d, true));
        }
    }

    // "--name=value" / "--name value" long options only; the reference passes a bare program name.
    class command_line_parser {
    public:
        command_line_parser(int argc, char** argv)
            : m_args(argv + (argc > 0 ? 1 : 0), argv + (argc > 0 ? argc : 0))
        {
        }
        command_line_parser& options(const options_description& d)
        {
            m_desc = &d;
            return *this;
        }
        command_line_parser& style(int) { return *this; }
        command_line_parser& allow_unregistered()
        {
            m_allowUnregistered = true;
            return *this;
        }
        parsed_options run()
        {
            parsed_options p(m_desc);
            for (std::size_t i = 0; i < m_args.size(); ++i) {
                const std::string& a = m_args[i];
                if (a.compare(0, 2, "--") != 0)
                    continue;
                std::string key = a.substr(2), val;
                std::size_t eq = key.find('=');
                if (eq != std::string::npos) {
                    val = key.substr(eq + 1);
                    key = key.substr(0, eq);
                } else if (i + 1 < m_args.size()) {
                    val = m_args[++i];
                }
                if (!m_desc->find(key) && !m_allowUnregistered)
                    throw error("unrecognised option " + key);
                p.options.push_back(option { key, { val } });
            }
            return p;
        }

    private:
        std::vector<std::string> m_args;
        const options_description* m_desc = nullptr;
        bool m_allowUnregistered = false;
    };

    inline parsed_options parse_config_file(std::istream& is, const options_description& d, bool allow_unregistered = false)
    {
        parsed_options p(&d);
        std::string line, prefix;
        while (std::getline(is, line)) {
            std::size_t hash = line.find('#');
            if (hash != std::string::npos)
                line.erase(hash);
            line = detail::trim(line);
            if (line.empty())
                continue;
            if (line.front() == '[' && line.back() == ']') {
                prefix = detail::trim(line.substr(1, line.size() - 2)) + ".";
                continue;
            }
            std::size_t eq = line.find('=');
            if (eq == std::string::npos)
                throw error("config line without '=': " + line);
            std::string key = prefix + detail::trim(line.substr(0, eq));
            if (!d.find(key)) {
                if (!allow_unregistered)
                    throw error("unrecognised option " + key);
                continue;
            }
            p.options.push_back(option { key, { detail::trim(line.substr(eq + 1)) } });
        }
        return p;
    }

} // namespace program_options
} // namespace boost

#endif
