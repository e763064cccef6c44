// The exception fence of every entry point (capi*.cpp): nothing thrown crosses the C ABI.
#pragma once
#include <exception>
#include <new>

#include "internal.hpp"

namespace opmhip {

template <class F>
int guarded(opmhip_ctx* c, F&& f) {
    try {
        return f();
    } catch (const std::bad_alloc&) {
        return fail(c, OPMHIP_UNKNOWN_ERROR, "out of host memory");
    } catch (const std::exception& e) {
        return fail(c, OPMHIP_UNKNOWN_ERROR, "exception: %s", e.what());
    } catch (...) {
        return fail(c, OPMHIP_UNKNOWN_ERROR, "unknown exception");
    }
}

}  // namespace opmhip
