// C ABI of include/tlab_amd.h: the runtime -- error string, device, stream, memory -- and DeviceArray.
#include "../../include/tlab_amd.h"

#include <hip/hip_runtime.h>

#include <string>

#include "errors.hpp"
#include "internal.hpp"
#include "plan.hpp"

using namespace tlab;

namespace {

thread_local std::string g_err;
int g_device = -1;

}  // namespace

// The library's stream.  Nothing but tlab_current_stream() and tlab_set_stream() can name it (the compiler sees to that), so every launch of the
// library takes it through the accessor, which runs a recorded substep first (csrc/deferred.cpp).  The tlab_internal_* fused variants that the drivers
// call from INSIDE such a replay go the same way: tlab_internal_deferred_flush() returns at once while a flush is under way (its g_busy).
class tlab_stream_holder {
    static hipStream_t s;
    friend hipStream_t (::tlab_current_stream)();
    friend int (::tlab_set_stream)(void *);
};
hipStream_t tlab_stream_holder::s = nullptr;

// hooks for the other translation units (internal.hpp)
hipStream_t tlab_current_stream() {
    (void)tlab_internal_deferred_flush();
    return tlab_stream_holder::s;
}
void tlab_set_error(const std::string &s) { g_err = s; }
bool tlab_device_ready() { return g_device >= 0; }

// ------------------------------------------------------------------------------------------------
// DeviceArray
// ------------------------------------------------------------------------------------------------
namespace tlab {
DeviceArray::~DeviceArray() {
    if (p) (void)hipFree(p);
}
void DeviceArray::upload(const std::vector<double> &h) {
    if (p) hk(hipFree(p), "hipFree");
    p = nullptr;
    n = h.size();
    if (n == 0) return;
    hk(hipMalloc((void **)&p, n * sizeof(double)), "hipMalloc(table)");
    hk(hipMemcpy(p, h.data(), n * sizeof(double), hipMemcpyHostToDevice), "hipMemcpy(table)");
}
void DeviceArray::alloc(size_t count) {
    if (p) hk(hipFree(p), "hipFree");
    p = nullptr;
    n = count;
    if (n) hk(hipMalloc((void **)&p, n * sizeof(double)), "hipMalloc(scratch)");
}
double *DeviceArray::reserve(size_t count, const char *what) {
    if (n < count) {
        if (p) hk(hipFree(p), "hipFree");
        p = nullptr;
        n = 0;
        hk(hipMalloc((void **)&p, count * sizeof(double)), what);
        n = count;
    }
    return p;
}
}  // namespace tlab

extern "C" {

const char *tlab_last_error(void) { return g_err.c_str(); }

int tlab_init(int device) {
    return catch_fail([&] {
        int count = 0;
        hk(hipGetDeviceCount(&count), "hipGetDeviceCount");
        if (count <= 0) throw Fail(TLAB_EHIP, "no HIP device visible: the MI355X kernels cannot run (there is no CPU fallback)");
        if (device < 0 || device >= count) throw Fail(TLAB_EINVAL, "tlab_init: bad device index");
        hk(hipSetDevice(device), "hipSetDevice");
        g_device = device;
    }, TLAB_EINVAL);
}

int tlab_finalize(void) {
    (void)tlab_deferred_enable(0);      // (runs what is still recorded)
    return catch_fail([&] {
        tlab_internal_operators_release();
    }, TLAB_EINVAL);
}

int tlab_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return n;
}

int tlab_set_stream(void *s) {
    (void)tlab_internal_deferred_flush();
    tlab_stream_holder::s = (hipStream_t)s;
    return TLAB_OK;
}

int tlab_sync(void) {
    const int rcd = tlab_internal_deferred_flush();
    const int rco = tlab_internal_deferred_take_error();      // a recorded substep that failed when another entry point made it run
    if (rcd != TLAB_OK) return rcd;
    if (rco != TLAB_OK) return rco;
    return catch_fail([&] { hk(hipStreamSynchronize(tlab_current_stream()), "hipStreamSynchronize"); }, TLAB_EINVAL);
}

int tlab_malloc(void **p, size_t bytes) {
    return catch_fail([&] {
        const hipError_t e = hipMalloc(p, bytes);
        if (e != hipSuccess) (void)hipGetLastError();      // a refused allocation is an answer, not a fault: the next launch's error check must not find it
        hk(e, "hipMalloc");                          // (TLab_AMD_Place_Arrays asks for candidates until the memory says no)
    }, TLAB_EINVAL);
}
int tlab_free(void *p) {
    (void)tlab_internal_deferred_flush();
    return catch_fail([&] { hk(hipFree(p), "hipFree"); }, TLAB_EINVAL);
}
int tlab_memcpy_h2d(void *dst, const void *src, size_t bytes) {
    return flushed([&] {
        const hipStream_t st = tlab_current_stream();
        hk(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st), "hipMemcpy h2d");
        hk(hipStreamSynchronize(st), "sync");
    });
}
int tlab_memcpy_d2h(void *dst, const void *src, size_t bytes) {
    return flushed([&] {
        const hipStream_t st = tlab_current_stream();
        hk(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st), "hipMemcpy d2h");
        hk(hipStreamSynchronize(st), "sync");
    });
}

}  // extern "C"
