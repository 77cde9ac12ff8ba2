// The scope arena of every entry point and helper that needs work space on the device: memory from the context's pool that goes
// back when the scope ends, and the host staging of the asynchronous copies issued inside it.  Host only.
#pragma once
#include <algorithm>
#include <cstring>
#include <deque>
#include <vector>

#include "device_ctx.h"

namespace ola {

typedef unsigned long long u64;      // as in gl.cuh, which notes the pair (this header takes nothing from the kernels' side)

// host memory that outlives the asynchronous copies issued from / into it: pinned when the context's arena has room
struct HostSpan {
    u64* p = nullptr; size_t n = 0;
    u64& operator[](size_t i) const { return p[i]; }
    u64* data() const { return p; }
    size_t size() const { return n; }
    u64* begin() const { return p; }
    u64* end() const { return p + n; }
};
struct DevBuf {
    DeviceCtx* ctx;
    std::vector<void*> ptrs;
    // Host staging of asynchronous copies (descriptors, power tables, index lists, read-backs): lives as long as the scope, whose
    // destructor drains the stream first -- so an upload needs no synchronisation of its own (each one stalled the host's
    // run-ahead: 14 of the 22 synchronisations per table were of this kind; the small tables are bound by exactly that latency).
    // Pinned (the context's arena, DeviceCtx::pinned_alloc) while it has room, pageable otherwise.
    std::deque<std::vector<u64>> hosts;
    size_t pinned_mark;
    struct Pending { void* dst; const u64* src; size_t bytes; };
    std::vector<Pending> pending;      // read-backs that landed in pinned memory and still have to reach the caller's buffer
    const bool use_pinned;             // false: a scope that outlives its call (OlaFri) -- the arena is a stack and is left to the calls
    HostSpan host(size_t elems) {
        if (use_pinned)
            if (void* p = ctx->pinned_alloc(std::max<size_t>(1, elems) * 8)) return {(u64*)p, elems};
        hosts.emplace_back(std::max<size_t>(1, elems));
        return {hosts.back().data(), elems};
    }
    u64* upload(const std::vector<u64>& v) {
        HostSpan h = host(v.size());
        std::copy(v.begin(), v.end(), h.begin());
        u64* d = alloc(std::max<size_t>(1, v.size()));
        if (!v.empty()) HIP_CHECK(hipMemcpyAsync(d, h.data(), v.size() * 8, hipMemcpyHostToDevice, ctx->stream));
        return d;
    }
    // device -> the caller's (pageable) buffer, complete after the next synchronisation + collect(): through pinned memory, so
    // that the copy is really asynchronous
    void readback(void* dst, const void* src_dev, size_t bytes) {
        if (!bytes) return;
        if (void* p = use_pinned ? ctx->pinned_alloc(bytes) : nullptr) {
            HIP_CHECK(hipMemcpyAsync(p, src_dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
            pending.push_back({dst, (const u64*)p, bytes});
        } else {
            HIP_CHECK(hipMemcpyAsync(dst, src_dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
        }
    }
    // after a synchronisation of the context's stream
    void collect() {
        for (const Pending& r : pending) memcpy(r.dst, r.src, r.bytes);
        pending.clear();
    }
    void sync_collect() {
        HIP_CHECK(hipStreamSynchronize(ctx->stream));
        collect();
    }
    // The pinned arena is a stack: a scope remembers its top when it opens and puts it back when it closes, so a scope that never
    // stages through pinned memory (the sort / scan scopes of lookup.hip and tablegen.hip) puts back what it found.  That is right
    // as long as scopes of one context nest last-in first-out, which C++ scopes on one thread do: each of those scopes is a local
    // of its function, inside the entry point's DevBuf or the only one of its call.  A scope that is not a local says pinned = false.
    explicit DevBuf(DeviceCtx* c, bool pinned = true) : ctx(c), pinned_mark(c->pinned_top), use_pinned(pinned) {}
    u64* alloc(size_t elems) { return (u64*)alloc_bytes(elems * 8); }
    template <typename T>
    T* alloc(size_t elems) { return (T*)alloc_bytes(elems * sizeof(T)); }
    void* alloc_bytes(size_t bytes) {
        void* p = ctx->alloc(bytes);
        ptrs.push_back(p);
        return p;
    }
    ~DevBuf() {
        (void)hipStreamSynchronize(ctx->stream);
        for (void* p : ptrs) ctx->free(p);
        if (use_pinned) ctx->pinned_top = pinned_mark;
    }
};

}  // namespace ola
