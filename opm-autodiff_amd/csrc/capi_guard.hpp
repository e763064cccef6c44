// The exception fence of the assembly half's entry points (capi_asm.cpp, capi_std_wells.cpp): nothing thrown crosses the C ABI.
#pragma once
#include <exception>

#include "internal.hpp"

namespace opmhip {

template <class F>
int guarded(opmhip_ctx* c, F&& f) {
    try {
        return f();
    } catch (const std::exception& e) {
        return fail(c, OPMHIP_UNKNOWN_ERROR, "exception: %s", e.what());
    } catch (...) {
        return fail(c, OPMHIP_UNKNOWN_ERROR, "unknown exception");
    }
}

}  // namespace opmhip
