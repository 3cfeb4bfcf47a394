// staging.h -- how a C entry that takes host arrays puts them on the device: one grow-only device allocation per
// context (Arena) and a per-call binder over it (Staging) that ties each host array to its share of it once.  Shared
// by libmpcqp and libmpcplan; it knows neither library's codes nor messages: it reports bool or hipError_t and the
// entry words the failure.
//
//   staging::Staging S(c->arena);
//   if (!S.bind([&] { d_x0 = S.in(x0, 5 * nb); d_u0 = S.out(u0, 2 * nb); })) return fail(..., "... staging");
//   S.upload(stream);  <the device entry on d_x0, d_u0>;  S.fetch(stream);  S.sync(stream);
//
// bind() runs the entry's bindings twice: once to add up the sizes and, when the arena holds that much, once more to
// hand out the pointers.  So no entry computes an offset, and a binding's condition must not change between the
// passes: it tests the host arguments, never a pointer the first pass returned (those are null).  A context is not
// re-entrant, so neither is its arena: no lock.
#ifndef MPC_STAGING_H
#define MPC_STAGING_H

#include <hip/hip_runtime.h>

namespace staging {

// The context's device block.  All-zero bytes are the empty arena (mpc_ctx is calloc'ed); release() at *_destroy
struct Arena {
    void* base;
    size_t cap;     // bytes

    void release() {
        (void)hipFree(base);
        base = nullptr;
        cap = 0;
    }
    // Grow only.  Growth frees first: hipFree waits for the device, so no kernel still reads the old block.  A
    // failed growth leaves the capacity at zero and the arena usable
    bool reserve(size_t bytes) {
        if (bytes <= cap) return true;
        release();
        if (hipMalloc(&base, bytes) == hipSuccess) cap = bytes;
        else base = nullptr, (void)hipGetLastError();
        return cap != 0;
    }
};

class Staging {
public:
    enum { MAX_BIND = 16, ALIGN = 16 };     // copies per call; every sub-array starts at a multiple of ALIGN bytes

    explicit Staging(Arena& a) : arena_(a) {}
    Staging(const Staging&) = delete;
    Staging& operator=(const Staging&) = delete;

    // Runs `bindings` (calls of in / out / out_or_scratch / scratch) for the sizes, grows the arena, runs them again
    // for the pointers.  False: more than MAX_BIND copies were asked for, or the device allocation failed
    template <typename F>
    bool bind(F&& bindings) {
        for (int pass = 0; pass < 2; ++pass) {
            live_ = pass == 1;
            used_ = 0;
            n_ = 0;
            bindings();
            if (overflow_ || (!live_ && !arena_.reserve(used_))) return false;
        }
        return true;
    }

    // Device space for `count` elements that upload() fills from `host`; null for a null host
    template <typename T>
    T* in(const T* host, size_t count) { return host ? (T*)take(const_cast<T*>(host), count * sizeof(T), true) : nullptr; }
    // Device space for `count` elements that fetch() copies to `host`; null for a null host (the kernel skips it)
    template <typename T>
    T* out(T* host, size_t count) { return host ? (T*)take(host, count * sizeof(T), false) : nullptr; }
    // Device space that is never copied
    template <typename T>
    T* scratch(size_t count) { return (T*)take(nullptr, count * sizeof(T), false); }
    // As out(), for a kernel that writes the array whether the caller wants it or not: never null
    template <typename T>
    T* out_or_scratch(T* host, size_t count) { return host ? out(host, count) : scratch<T>(count); }

    // The recorded copies, in binding order.  With a stream: hipMemcpyAsync on it, and sync(stream) afterwards;
    // without one: blocking hipMemcpy (the null stream's order), and sync() is the device's
    hipError_t upload(hipStream_t s) { return copy(true, &s); }
    hipError_t fetch(hipStream_t s) { return copy(false, &s); }
    hipError_t sync(hipStream_t s) { return hipStreamSynchronize(s); }
    hipError_t upload() { return copy(true, nullptr); }
    hipError_t fetch() { return copy(false, nullptr); }
    hipError_t sync() { return hipDeviceSynchronize(); }

private:
    struct Bind { void *host, *dev; size_t bytes; bool up; };

    void* take(void* host, size_t bytes, bool up) {
        void* dev = live_ ? (char*)arena_.base + used_ : nullptr;
        used_ += (bytes + ALIGN - 1) / ALIGN * ALIGN;
        if (!host) return dev;
        // both passes count, so a table that is too small fails bind() before any pointer is handed out
        if (n_ == MAX_BIND) {
            overflow_ = true;
            return nullptr;
        }
        table_[n_++] = Bind{host, dev, bytes, up};
        return dev;
    }

    hipError_t copy(bool up, const hipStream_t* s) {
        const hipMemcpyKind kind = up ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost;
        for (int i = 0; i < n_; ++i) {
            const Bind& b = table_[i];
            if (b.up != up) continue;
            void* dst = up ? b.dev : b.host;
            const void* src = up ? b.host : b.dev;
            const hipError_t e = s ? hipMemcpyAsync(dst, src, b.bytes, kind, *s) : hipMemcpy(dst, src, b.bytes, kind);
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    }

    Arena& arena_;
    Bind table_[MAX_BIND];
    size_t used_ = 0;
    int n_ = 0;
    bool live_ = false, overflow_ = false;
};

}  // namespace staging

#endif
