// libs2sr stall mode: the third diagnostic mode next to red zones and poison (redzone.hip).  A consumer that does
// not wait for its producer on another stream changes no byte while the producer happens to be done in time.  Here a stream is
// held back by a kernel that does nothing but let time pass, at the head of every stream segment, so the producer is provably
// late; and one named wait can be dropped (s2sr_debug_delay_drop), so the tests can show they would notice.  Off by default: the
// wrappers of engine_internal.h and door_enter then cost one relaxed atomic load each and enqueue nothing.
// Also here: door_enter / door_leave, the order between two calls on one handle that run on different streams.
#include "engine_internal.h"

using namespace s2sr;
using namespace s2sr::engine;

std::atomic<int> s2sr::engine::g_delay_mode{0};
std::atomic<int> s2sr::engine::g_delay_drop{-1};

namespace {

std::atomic<int> g_delay_usec{0};
constexpr int kMaxStallUsec = S2SR_DEBUG_STALL_MAX_USEC;

// One wave reads the constant-rate counter until `ticks` have passed, sleeping between reads.  It touches no memory, so there is
// nothing another agent could fail to write; `cap` iterations end it whatever the counter does.
__global__ void __launch_bounds__(64) stall_kernel(unsigned long long ticks, unsigned cap) {
    const unsigned long long t0 = wall_clock64();
    for (unsigned i = 0; i < cap; ++i) {
        if (wall_clock64() - t0 >= ticks) break;
        __builtin_amdgcn_s_sleep(32);            // 32 x 64 clocks: about a microsecond
    }
}

hipError_t launch_stall(hipStream_t st, int usec) {
    if (usec <= 0) return hipSuccess;
    int dev = 0, khz = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess || khz <= 0) {
        (void)hipGetLastError();
        khz = 100000;                            // the constant-rate counter of the CDNA parts: 100 MHz
    }
    const unsigned long long ticks = (unsigned long long)usec * (unsigned long long)khz / 1000ull;
    // a sleep of ~1 us and two counter reads per iteration: 4 iterations per microsecond is never reached, so time ends the stall;
    // were the counter stuck, 4 x 20 000 + 1000 iterations end it after some 0.1 s
    const unsigned cap = 4u * (unsigned)usec + 1000u;
    stall_kernel<<<dim3(1), dim3(64), 0, st>>>(ticks, cap);
    return hipGetLastError();
}

bool capturing(hipStream_t st) {
    if (!st) return false;                       // the legacy stream cannot be captured
    hipStreamCaptureStatus status = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &status) != hipSuccess) {
        (void)hipGetLastError();
        return true;                             // a stream in an unknown state gets no stall
    }
    return status != hipStreamCaptureStatusNone;
}

}  // namespace

hipError_t s2sr::engine::delay_stall(s2sr_handle* h, hipStream_t st) {
    const int mode = g_delay_mode.load(std::memory_order_relaxed);
    if (!(mode & (st == h->copy_stream ? 2 : 1)) || capturing(st)) return hipSuccess;
    return launch_stall(st, g_delay_usec.load(std::memory_order_relaxed));
}

int s2sr::engine::door_enter(s2sr_handle* h, hipStream_t st) {
    if (h->order_pending && h->order_stream != st) {
        HIPCHK(h, ev_stream_wait(h, st, h->order_ev, SITE_HANDLE_ORDER));
        if (st == h->stream) HIPCHK(h, ev_stream_wait(h, h->copy_stream, h->order_ev, SITE_HANDLE_ORDER));
    }
    if (g_delay_mode.load(std::memory_order_relaxed)) {
        HIPCHK(h, delay_stall(h, st));
        HIPCHK(h, delay_stall(h, h->copy_stream));
    }
    return S2SR_OK;
}

int s2sr::engine::door_leave(s2sr_handle* h, hipStream_t st, int rc) {
    if (!h->order_ev && hipEventCreateWithFlags(&h->order_ev, hipEventDisableTiming) != hipSuccess) {
        (void)hipGetLastError();
        h->order_ev = nullptr;
        return rc ? rc : fail(h, S2SR_E_HIP, "hipEventCreate failed (the handle's order event)");
    }
    // also behind a call that failed half way: what it did enqueue still runs
    if (ev_record(h, h->order_ev, st, SITE_HANDLE_ORDER) != hipSuccess) {
        (void)hipGetLastError();
        return rc ? rc : fail(h, S2SR_E_HIP, "hipEventRecord failed (the handle's order event)");
    }
    h->order_stream = st;
    h->order_pending = true;
    return rc;
}

extern "C" {

static_assert(SITE_BATCH_GROUP_D2H == S2SR_SITE_BATCH_GROUP_D2H && SITE_CHUNK_BAND_D2H == S2SR_SITE_CHUNK_BAND_D2H &&
              SITE_DISPLAY_BAND_D2H == S2SR_SITE_DISPLAY_BAND_D2H && SITE_COPY_TO_HOST == S2SR_SITE_COPY_TO_HOST, "include/s2sr.h states the droppable sites");

int s2sr_debug_delay(int32_t mode, int32_t usec) {
    if (mode < 0 || mode > 3 || usec < 0 || usec > kMaxStallUsec || (mode && !usec))
        return fail(nullptr, S2SR_E_INVALID, "stall mode must be 0..3 (bit 1 compute side, bit 2 copy side) with 1..20000 microseconds (0 with mode 0)");
    g_delay_usec.store(usec);
    g_delay_mode.store(mode);
    return S2SR_OK;
}

int32_t s2sr_debug_delay_mode(void) { return g_delay_mode.load(); }
int32_t s2sr_debug_delay_usec(void) { return g_delay_usec.load(); }

int s2sr_debug_delay_drop(int32_t site) {
    bool ok = site == -1;
    for (int s : kDroppableSites) ok = ok || s == site;
    if (!ok) return fail(nullptr, S2SR_E_INVALID, "only a wait whose stream next copies finished pixels to the host can be dropped (-1: none)");
    g_delay_drop.store(site);
    return S2SR_OK;
}

int32_t s2sr_debug_delay_dropped(void) { return g_delay_drop.load(); }

int s2sr_debug_stall(s2sr_handle* h, int32_t which, void* stream, int32_t usec) {
    if (!h) return S2SR_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    if (which < 0 || which > 2 || usec < 1 || usec > kMaxStallUsec)
        return fail(h, S2SR_E_INVALID, "s2sr_debug_stall: which 0 (the handle's stream), 1 (its copy stream) or 2 (the caller's), 1..20000 microseconds");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    hipStream_t st = which == 0 ? h->stream : which == 1 ? h->copy_stream : (hipStream_t)stream;
    if (capturing(st)) return fail(h, S2SR_E_INVALID, "s2sr_debug_stall: the stream is capturing");
    HIPCHK(h, launch_stall(st, usec));
    return S2SR_OK;
}

// The small hook of the independence probe: n bytes of the trash page set to zero on one of the handle's streams (which as above;
// only the epilogues' parked stores ever land there), and optionally the host waits for that stream.
int s2sr_debug_stream_touch(s2sr_handle* h, int32_t which, void* stream, int32_t wait) {
    if (!h) return S2SR_E_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    if (which < 0 || which > 2) return fail(h, S2SR_E_INVALID, "s2sr_debug_stream_touch: which 0, 1 or 2");
    HIPCHK(h, hipSetDevice(h->cfg.device));
    hipStream_t st = which == 0 ? h->stream : which == 1 ? h->copy_stream : (hipStream_t)stream;
    HIPCHK(h, hipMemsetAsync(h->d_trash, 0, 64, st));
    if (wait) HIPCHK(h, hipStreamSynchronize(st));
    return S2SR_OK;
}

}  // extern "C"
