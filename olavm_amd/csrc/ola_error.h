// The exception every layer below the C ABI throws: an OLA_E_* code and the text ola_gpu_last_error() returns.  Host only (no HIP), so
// that the host-side stages (challenger_host.h, airset_host.h, verify_host.h) compile without the HIP headers.
#pragma once
#include <stdexcept>
#include <string>

namespace ola {

struct OlaError : public std::runtime_error {
    int code;
    OlaError(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

}  // namespace ola
