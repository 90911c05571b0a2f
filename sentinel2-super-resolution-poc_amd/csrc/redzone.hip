// libs2sr red-zone mode (host code only): the device side of csrc/redzone.h -- dev_malloc / dev_free with zones, the zones between
// the workspace planes, and the three s2sr_debug_redzone* entries of include/s2sr.h.  Off by default; see s2sr_internal.h.
#include <stdio.h>
#include <stdlib.h>

#include <mutex>
#include <string>

#include "engine_internal.h"
#include "redzone.h"

using namespace s2sr;
using namespace s2sr::engine;

std::atomic<size_t> s2sr::g_redzone_bytes{0};
std::atomic<bool> s2sr::g_redzone_ever{false};

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

extern "C" {

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
    // this handle's own allocations, planes included: what `allocations` counts.  The list follows the device buffers of
    // s2sr_handle (engine_internal.h, which points here): a new one is added in both places.
    int64_t own = 0;
    auto count = [&](const void* p) { if (p && registry().find(p)) ++own; };
    count(h->d_trash); count(h->pool_w); count(h->pool_s); count(h->pool_b); count(h->first16.d_wpack);
    for (const ConvW& c : h->convs) {
        if (!c.pooled) count(c.d_wpack);
        count(c.d_wphase[0]); count(c.d_wphase[1]);
    }
    for (int i = 0; i < s2sr_handle::kScratchSlots; ++i) count(h->d_scratch[i]);
    for (const auto& m : h->stitch_sets) count(m.d);
    if (h->ws.base && registry().find(h->ws.base)) own += 1 + (int64_t)registry().planes(h->ws.base);
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
    if (!h->d_scratch[slot] || !registry().find(h->d_scratch[slot], &r)) return fail(h, S2SR_E_INVALID, "this scratch slot has no red zone");
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
