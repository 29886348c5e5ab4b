// How a failure inside the library becomes a TLAB_E* code of include/tlab_amd.h: ONE exception type that carries its code, and ONE guard that every
// C entry point puts around its body, so that no exception leaves an extern "C" function.  Header-only, host code; libtlab_amd_comm.so (comm.hip)
// uses it too and takes tlab_set_error / tlab_device_ready from the core library.
#pragma once
#include <hip/hip_runtime.h>

#include <new>
#include <stdexcept>
#include <string>
#include <type_traits>

#include "internal.hpp"

namespace tlab {

struct Fail : std::runtime_error {
    int code;
    Fail(int c, const std::string &s) : std::runtime_error(s), code(c) {}
};
// the result of a nested C-ABI call: its code, its text behind `what`
inline void ok(int rc, const char *what) {
    if (rc != TLAB_OK) throw Fail(rc, std::string(what) + ": " + tlab_last_error());
}
// ... passed on as it is
inline void ok(int rc) {
    if (rc != TLAB_OK) throw Fail(rc, tlab_last_error());
}
inline void hk(hipError_t e, const char *what) {
    if (e != hipSuccess) throw Fail(TLAB_EHIP, std::string(what) + ": " + hipGetErrorString(e));
}

// The body of an entry point (it returns nothing, or the code of a refusal it has put into words itself): a Fail becomes its code, with its text
// in tlab_last_error(); a failed host allocation TLAB_ENOMEM; any other std::exception (the helper files throw std::runtime_error) becomes `other`.
template <class F>
int catch_fail(F f, int other) {
    try {
        if constexpr (std::is_void_v<decltype(f())>) {
            f();
            return TLAB_OK;
        } else {
            return f();
        }
    } catch (const Fail &e) {
        tlab_set_error(e.what());
        return e.code;
    } catch (const std::bad_alloc &) {
        tlab_set_error("out of memory");
        return TLAB_ENOMEM;
    } catch (const std::exception &e) {
        tlab_set_error(e.what());
        return other;
    }
}
// ... of an entry point that is refused before tlab_init
template <class F>
int guarded(F f) {
    return catch_fail([&] {
        if (!tlab_device_ready()) throw Fail(TLAB_EHIP, "tlab_init has not been called (no CPU fallback exists)");
        f();
    }, TLAB_EINVAL);
}
// ... of an entry point before which a recorded substep runs (deferred.cpp), and whose answer is that substep's failure if it fails
template <class F>
int flushed(F f) {
    const int rcd = tlab_internal_deferred_flush();
    if (rcd != TLAB_OK) return rcd;
    return catch_fail(f, TLAB_EINVAL);
}

}  // namespace tlab
