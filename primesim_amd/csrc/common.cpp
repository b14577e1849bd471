// common.cpp — the error text of the C ABI: one message per thread, set by
// whatever fails (pu::set_error) and read back by pu_last_error().  No HIP.

#include <string>

#include "../../include/primeuncore.h"
#include "common.h"

namespace pu {

static thread_local std::string g_err;

int set_error(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

const std::string& last_error() { return g_err; }

}  // namespace pu

extern "C" const char* pu_last_error(void) { return pu::g_err.c_str(); }
