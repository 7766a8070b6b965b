// occ_handle.hpp -- the scaffold of a side library's handle (libocc_basis.so, libocc_sim.so): the
// device and its one plain stream, the handle's error text, an arena of what it allocated, the deadline wait, the three
// early-return macros and the create / destroy wrappers of its C ABI.  A library derives its handle from occ::HandleBase and
// keeps its own fields, kernels and entry points.  Host code only, but it parses in the device pass too.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "occ_wait.hpp"

namespace occ {

// the status codes the macros and the wrappers return; a library asserts that its own are these (OCC_HANDLE_CODES)
constexpr int H_OK = 0, H_E_BADARG = -1, H_E_HIP = -2;
#define OCC_HANDLE_CODES(ok, e_badarg, e_hip) \
    static_assert((ok) == occ::H_OK && (e_badarg) == occ::H_E_BADARG && (e_hip) == occ::H_E_HIP, "occ_handle.hpp returns 0 / -1 / -2")

// inside a function that returns a status and has the handle as `h`
#define H_TRY(expr)                                                     \
    do {                                                                \
        const hipError_t e_ = (expr);                                   \
        if (e_ != hipSuccess) {                                         \
            h->err = std::string(#expr) + ": " + hipGetErrorString(e_); \
            return occ::H_E_HIP;                                        \
        }                                                               \
    } while (0)
#define H_WAIT(what) do { if (const int w_ = h->wait(what); w_ != occ::H_OK) return w_; } while (0)
#define H_ARG(cond, msg)            \
    do {                            \
        if (!(cond)) {              \
            h->err = (msg);         \
            return occ::H_E_BADARG; \
        }                           \
    } while (0)

struct HandleBase {
    int device = 0;
    hipStream_t st = nullptr;  // one plain stream per handle (not CU-masked, not from the engine's pool)
    std::string err;
    std::vector<void *> arena, pinned;  // what close() frees: device allocations, pinned host allocations

    // the device exists and is a gfx950; it becomes the thread's device and gets the handle's stream
    int open(int32_t device)
    {
        HandleBase *const h = this;
        h->device = device;
        int ndev = 0;
        H_TRY(hipGetDeviceCount(&ndev));
        H_ARG(device >= 0 && device < ndev, "no such device");
        H_TRY(hipSetDevice(device));
        hipDeviceProp_t prop;
        H_TRY(hipGetDeviceProperties(&prop, device));
        if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
            err = std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950";
            return H_E_HIP;
        }
        H_TRY(hipStreamCreateWithFlags(&h->st, hipStreamNonBlocking));
        return H_OK;
    }

    // the stream has drained, or the deadline has passed (occ_wait.hpp; the engine's wait_on is the other caller of the poll)
    int wait(const char *what)
    {
        const double limit = host_wait_limit_s();
        const WaitResult r = poll_until(
            [this] {
                const hipError_t q = hipStreamQuery(st);
                if (q == hipErrorNotReady) (void)hipGetLastError();  // (not ready is not an error to keep)
                return (int)q;
            },
            (int)hipErrorNotReady, limit);
        if (r.end == WaitEnd::done) return H_OK;
        char late[64];
        std::snprintf(late, sizeof(late), "the stream did not drain within %.0f s", limit);
        err = std::string(what) + ": " + (r.end == WaitEnd::failed ? hipGetErrorString((hipError_t)r.code) : late);
        return H_E_HIP;
    }

    // `count` elements on the device (at least one), owned by the handle; zero: filled on the stream, not waited for
    template <class T>
    int alloc(T **out, size_t count, bool zero)
    {
        HandleBase *const h = this;
        void *p = nullptr;
        const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
        H_TRY(hipMalloc(&p, bytes));
        arena.push_back(p);
        *out = (T *)p;
        if (zero) H_TRY(hipMemsetAsync(p, 0, bytes, h->st));
        return H_OK;
    }

    template <class T>
    int alloc_pinned(T **out, size_t count)
    {
        HandleBase *const h = this;
        void *p = nullptr;
        H_TRY(hipHostMalloc(&p, std::max<size_t>(count, 1) * sizeof(T), hipHostMallocDefault));
        pinned.push_back(p);
        *out = (T *)p;
        return H_OK;
    }

    // a host vector's copy on the device, waited for (the host vector may go away after this)
    template <class T, class S>
    int upload(T **dst, const std::vector<S> &src)
    {
        static_assert(sizeof(T) == sizeof(S), "upload: same width");
        HandleBase *const h = this;
        const int rc = alloc(dst, src.size(), false);
        if (rc != H_OK) return rc;
        if (!src.empty()) H_TRY(hipMemcpyAsync(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice, h->st));
        H_WAIT("upload");
        return H_OK;
    }

    // the last call before the handle is deleted
    void close(const char *what)
    {
        (void)hipSetDevice(device);
        if (st) {
            (void)wait(what);
            (void)hipStreamDestroy(st);
        }
        for (void *q : arena) (void)hipFree(q);
        for (void *q : pinned) (void)hipHostFree(q);
    }
};

// ---- destroy and create of a library's C ABI, around its own handle type H (derived from HandleBase) -----------------------
template <class H>
int handle_destroy(H *h, const char *what)
{
    if (!h) return H_OK;
    h->close(what);
    delete h;
    return H_OK;
}

// create_impl(h) fills a fresh handle; a failure leaves its text in `create_err` (the caller's thread-local) and no handle
template <class H, class Impl>
int handle_create(H **out, std::string &create_err, const char *destroy_what, Impl &&create_impl)
{
    if (!out) {
        create_err = "null output pointer";
        return H_E_BADARG;
    }
    *out = nullptr;
    H *h = new H();
    const int rc = create_impl(h);
    if (rc != H_OK) {
        create_err = h->err;
        (void)hipGetLastError();
        handle_destroy(h, destroy_what);
        return rc;
    }
    *out = h;
    return H_OK;
}

}  // namespace occ
