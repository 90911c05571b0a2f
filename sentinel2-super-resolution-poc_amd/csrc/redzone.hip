// libs2sr red-zone and poison modes (host code only): the device side of csrc/redzone.h -- dev_malloc / dev_free with zones, the zones
// between the workspace planes, the poison fill of fresh allocations and of the scratch slots, and the s2sr_debug_redzone* /
// s2sr_debug_poison* / s2sr_debug_scratch_peek entries of include/s2sr.h.  Both off by default; see s2sr_internal.h.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <string>

#include "engine_internal.h"
#include "redzone.h"

using namespace s2sr;
using namespace s2sr::engine;

std::atomic<size_t> s2sr::g_redzone_bytes{0};
std::atomic<bool> s2sr::g_redzone_ever{false};
std::atomic<int> s2sr::g_poison{0};

namespace {

redzone::Registry& registry() {
    static redzone::Registry* r = new redzone::Registry();   // never destroyed: handles may be closed while the process exits
    return *r;
}

// Fills and read-backs run on a private non-blocking stream per device, never the legacy stream (the device-gate rule of
// s2sr_internal.h).  Every caller holds the device gate.
hipStream_t io_stream() {
    static hipStream_t st[64] = {nullptr};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
    if (!st[dev] && hipStreamCreateWithFlags(&st[dev], hipStreamNonBlocking) != hipSuccess) st[dev] = nullptr;
    return st[dev];
}
bool io_write(void*, void* dst, const uint8_t* src, size_t n) {
    hipStream_t st = io_stream();
    return st && hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess;
}
bool io_read(void*, uint8_t* dst, const void* src, size_t n) {
    hipStream_t st = io_stream();
    return st && hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, st) == hipSuccess && hipStreamSynchronize(st) == hipSuccess;
}
const redzone::DeviceIo kIo{io_write, io_read, nullptr};

bool set_zone(int64_t bytes) {
    if (bytes < 0 || bytes % 4096 != 0) return false;
    if (bytes > 0) g_redzone_ever.store(true);
    g_redzone_bytes.store((size_t)bytes);
    return true;
}

// S2SR_REDZONE=<bytes>, read once when the library is loaded: the initial Z.  With it set, one line at process exit.
struct EnvSwitch {
    bool set = false;
    EnvSwitch() {
        const char* g = getenv("S2SR_REDZONE");
        if (!g || !*g) return;
        set = true;
        char* end = nullptr;
        const long long v = strtoll(g, &end, 10);
        if (end == g || *end || !set_zone(v))
            fprintf(stderr, "s2sr: S2SR_REDZONE=%s is not a number of bytes that is a multiple of 4096: red zones stay off\n", g);
    }
    ~EnvSwitch() {
        if (!set) return;
        size_t n = 0, m = 0;
        registry().totals(&n, &m);
        // what was checked at a free or by s2sr_debug_redzone_check: buffers still live now are not read (the device may be gone)
        fprintf(stderr, "s2sr redzones: %zu allocations checked, %zu damaged\n", n, m);
    }
} g_env_switch;

// pinned host memory is the host's to write: the same fill through a memcpy
bool host_write(void*, void* dst, const uint8_t* src, size_t n) { memcpy(dst, src, n); return true; }
bool host_read(void*, uint8_t* dst, const void* src, size_t n) { memcpy(dst, src, n); return true; }
const redzone::DeviceIo kHostIo{host_write, host_read, nullptr};

// S2SR_POISON=<1|2>, read once when the library is loaded: the initial pattern
struct PoisonEnvSwitch {
    PoisonEnvSwitch() {
        const char* g = getenv("S2SR_POISON");
        if (!g || !*g) return;
        char* end = nullptr;
        const long long v = strtoll(g, &end, 10);
        if (end == g || *end || v < 1 || !poison::valid(v))
            fprintf(stderr, "s2sr: S2SR_POISON=%s is neither 1 nor 2: poison stays off\n", g);
        else
            g_poison.store((int)v);
    }
} g_poison_env_switch;

void sync_handle(s2sr_handle* h) {
    hipSetDevice(h->cfg.device);
    if (h->stream) hipStreamSynchronize(h->stream);
    if (h->copy_stream) hipStreamSynchronize(h->copy_stream);
}

}  // namespace

hipError_t s2sr::redzone_malloc(void** p, size_t bytes, size_t zone) {
    char* base = nullptr;
    const hipError_t e = hipMalloc((void**)&base, bytes + 2 * zone);
    if (e != hipSuccess) return e;
    if (!registry().add(kIo, base + zone, bytes, zone, zone)) {
        (void)hipFree(base);
        return hipErrorUnknown;
    }
    *p = base + zone;
    return hipSuccess;
}

hipError_t s2sr::redzone_free(void* p) {
    redzone::Record r;
    if (!registry().find(p, &r)) return hipFree(p);   // allocated while the mode was off
    (void)hipDeviceSynchronize();                     // hipFree would wait for the device as well: nothing may still be writing
    registry().remove(kIo, p, &r);
    return hipFree(r.base());
}

hipError_t s2sr::redzone_add_plane(void* parent, void* plane, size_t bytes, size_t back) {
    DeviceGate g;
    if (!registry().find(parent)) return hipSuccess;   // the mode went on between the plan and the allocation: no zones to pattern
    return registry().add(kIo, plane, bytes, 0, back, parent) ? hipSuccess : hipErrorUnknown;
}

hipError_t s2sr::poison_device(void* p, size_t bytes, int pat) {
    return poison::fill(kIo, p, bytes, pat) ? hipSuccess : hipErrorUnknown;
}

void s2sr::poison_host(void* p, size_t bytes, int pat) { (void)poison::fill(kHostIo, p, bytes, pat); }

extern "C" {

static_assert(slots::kSlots == S2SR_SCRATCH_SLOTS && kTrashBytes == S2SR_TRASH_BYTES, "include/s2sr.h states both");

int s2sr_debug_poison(int32_t pattern) {
    if (!poison::valid(pattern)) return fail(nullptr, S2SR_E_INVALID, "poison pattern must be 0 (off), 1 (all 0xFF) or 2 (position-dependent)");
    g_poison.store(pattern);
    return S2SR_OK;
}

int32_t s2sr_debug_poison_pattern(void) { return g_poison.load(); }

int s2sr_debug_poison_scratch(s2sr_handle* h, int64_t* slots, int64_t* bytes) {
    if (!h || !slots || !bytes) return fail(h, S2SR_E_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    const int pat = g_poison.load();
    if (pat == poison::kOff) return fail(h, S2SR_E_INVALID, "poison mode is off (s2sr_debug_poison)");
    sync_handle(h);
    DeviceGate g;
    h->scratch.drop(slots::kAllSlots);
    *slots = 0;
    for (int i = 0; i < slots::kSlots; ++i) {
        bytes[i] = 0;
        if (!h->scratch.ptr[i] || !h->scratch.cap[i]) continue;
        if (!poison::fill(kIo, h->scratch.ptr[i], h->scratch.cap[i], pat)) return fail(h, S2SR_E_HIP, "poison fill of a scratch slot failed");
        *slots |= (int64_t)1 << i;
        bytes[i] = (int64_t)h->scratch.cap[i];
    }
    if (h->d_trash && !poison::fill(kIo, h->d_trash, kTrashBytes, pat)) return fail(h, S2SR_E_HIP, "poison fill of the trash page failed");
    return S2SR_OK;
}

int s2sr_debug_scratch_peek(s2sr_handle* h, int32_t slot, int64_t offset, int64_t n, uint8_t* out) {
    if (!h || !out) return fail(h, S2SR_E_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    if (slot < -1 || slot >= slots::kSlots) return fail(h, S2SR_E_INVALID, "scratch slot out of range (-1: the trash page, 0..7)");
    const char* base = slot < 0 ? h->d_trash : (const char*)h->scratch.ptr[slot];
    const size_t cap = slot < 0 ? (h->d_trash ? kTrashBytes : 0) : h->scratch.cap[slot];
    if (!base || offset < 0 || n < 0 || (uint64_t)offset > cap || (uint64_t)n > cap - (uint64_t)offset)
        return fail(h, S2SR_E_INVALID, "the range is not inside this scratch slot");
    if (!n) return S2SR_OK;
    sync_handle(h);
    DeviceGate g;
    if (!io_read(nullptr, out, base + offset, (size_t)n)) return fail(h, S2SR_E_HIP, "scratch read-back failed");
    return S2SR_OK;
}

int s2sr_debug_redzone(int64_t bytes) {
    if (!set_zone(bytes)) return fail(nullptr, S2SR_E_INVALID, "red zone bytes must be 0 or a positive multiple of 4096");
    return S2SR_OK;
}

int64_t s2sr_debug_redzone_bytes(void) { return (int64_t)g_redzone_bytes.load(); }

int s2sr_debug_redzone_check(s2sr_handle* h, int64_t* allocations, int64_t* damaged) {
    if (!h || !allocations || !damaged) return fail(h, S2SR_E_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    sync_handle(h);
    DeviceGate g;
    // this handle's own zoned allocations, the workspace's planes included: what `allocations` counts
    int64_t own = 0;
    for_each_device_buffer(h, [&](const void* p) { if (p && registry().find(p)) own += 1 + (int64_t)registry().planes(p); });
    size_t n = 0, bad = 0;
    redzone::Damage first;
    if (!registry().check_all(kIo, &n, &bad, &first)) return fail(h, S2SR_E_HIP, "red zone read-back failed");
    *allocations = own;
    *damaged = (int64_t)bad;
    if (bad) h->err = first.describe();
    return S2SR_OK;
}

int s2sr_debug_redzone_poke(s2sr_handle* h, int32_t slot, int64_t offset) {
    if (!h) return fail(h, S2SR_E_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    if (slot < 0 || slot >= 6) return fail(h, S2SR_E_INVALID, "scratch slot out of range (0..5)");
    redzone::Record r;
    if (!h->scratch.ptr[slot] || !registry().find(h->scratch.ptr[slot], &r)) return fail(h, S2SR_E_INVALID, "this scratch slot has no red zone");
    const bool back = offset >= 0;
    const uint64_t dist = back ? (uint64_t)offset : (uint64_t)(-(offset + 1));   // bytes from the user range's edge, 0 = the nearest
    if (dist >= (back ? r.back : r.front)) return fail(h, S2SR_E_INVALID, "offset is not inside the red zone");
    const size_t at = back ? (size_t)dist : r.front - 1 - (size_t)dist;          // offset into that zone
    sync_handle(h);
    DeviceGate g;
    const uint8_t v = (uint8_t)~redzone::pattern(back, at);
    if (!io_write(nullptr, back ? r.user + r.bytes + at : r.user - r.front + at, &v, 1)) return fail(h, S2SR_E_HIP, "red zone poke failed");
    return S2SR_OK;
}

}  // extern "C"
