// dbh_owned.h — move-only owners of what the HIP runtime hands out: a device block, a pinned host
// block, a stream, an event.  Whoever holds one as a member frees it by being destroyed; nothing in
// libdeepbinner_hip.so keeps a list of things to free.  Failures come back as the hipError_t of the
// call that failed, for the caller's own status mapping (DBH_HIP / hip_fail: dbh_status.h).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <utility>

#include "dbh_host_layout.h"

// (one definition for every unit - dbh_model.h's objects hold these as members in several units -
// and none of it a symbol of the library)
namespace dbh_owned __attribute__((visibility("hidden"))) {

inline hipError_t device_alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
inline hipError_t pinned_alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }

// a handle of type T, released by Free; moving leaves the source empty
template <typename T, hipError_t (*Free)(T)>
struct Handle {
    T h = nullptr;
    Handle() = default;
    Handle(Handle&& o) noexcept : h(std::exchange(o.h, nullptr)) {}
    Handle& operator=(Handle&& o) noexcept { std::swap(h, o.h); return *this; }
    ~Handle() { if (h) (void)Free(h); }
    operator T() const { return h; }
};
using Stream = Handle<hipStream_t, hipStreamDestroy>;
using Event = Handle<hipEvent_t, hipEventDestroy>;

// a block that only grows
template <hipError_t (*Alloc)(void**, size_t), hipError_t (*Free)(void*)>
struct Block {
    void* ptr = nullptr;
    size_t bytes = 0;
    Block() = default;
    Block(Block&& o) noexcept : ptr(std::exchange(o.ptr, nullptr)), bytes(std::exchange(o.bytes, 0)) {}
    Block& operator=(Block&& o) noexcept { std::swap(ptr, o.ptr); std::swap(bytes, o.bytes); return *this; }
    ~Block() { if (ptr) (void)Free(ptr); }
    // Nothing when the block holds `need` bytes already; otherwise the old block is freed BEFORE
    // the new one is asked for (the two never add up) and its contents are gone.  *fresh: is the
    // block a new one?  After a failure the block is empty.
    hipError_t reserve(size_t need, bool* fresh = nullptr) {
        if (fresh) *fresh = bytes < need;
        if (bytes >= need) return hipSuccess;
        bytes = 0;
        hipError_t e = ptr ? Free(std::exchange(ptr, nullptr)) : hipSuccess;
        if (e == hipSuccess) e = Alloc(&ptr, need);
        if (e == hipSuccess) bytes = need;
        else ptr = nullptr;
        return e;
    }
    // lay_out(Carve&): run over a null base for the size to reserve, then over the block
    template <class LayOut>
    hipError_t carve(LayOut&& lay_out) {
        dbh_host::Carve sizing(nullptr);
        lay_out(sizing);
        const hipError_t e = reserve(sizing.used);
        dbh_host::Carve regions(ptr);
        lay_out(regions);
        return e;
    }
    void* get() const { return ptr; }
    template <typename T> T* as(size_t byte_offset = 0) const { return (T*)((char*)ptr + byte_offset); }
};
using DeviceBlock = Block<device_alloc, hipFree>;
using PinnedBlock = Block<pinned_alloc, hipHostFree>;

}  // namespace dbh_owned
