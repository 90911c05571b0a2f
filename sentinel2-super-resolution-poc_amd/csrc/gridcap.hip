// libs2sr grid cap ("Capped grids"): the fourth diagnostic mode next to red zones, poison (redzone.hip) and
// stalled streams (stall.hip).  Every hot kernel is a loop over work items inside a workgroup that stays; at the sizes the tests
// can afford, a 256-CU part gives every workgroup one item, and the second trip through the loop -- where a stale LDS stage, a
// wait that counts the previous epilogue's stores, a missing loop-top barrier or a narrow stride would live -- never runs.  With
// a cap in force the launchers (capped_grid, s2sr_internal.h) take at most that many workgroups, so a small image makes many
// trips.  No kernel knows: the cap changes a launch's grid and nothing else.  Off by default: one relaxed atomic load per launch.
// The cap is read when a launch is enqueued, so a captured graph keeps the grid it was captured with.
#include "engine_internal.h"

using namespace s2sr;
using namespace s2sr::engine;

std::atomic<int> s2sr::g_grid_cap{0};

namespace {

constexpr int kMaxCap = S2SR_DEBUG_GRID_CAP_MAX;

// what the capped launches did, per family: host arithmetic only
std::atomic<long long> g_launches[GF_COUNT];
std::atomic<long long> g_trips[GF_COUNT];

bool set_cap(long long v) {
    if (v < 0 || v > kMaxCap) return false;
    g_grid_cap.store((int)v);
    return true;
}

// S2SR_GRID_CAP=<workgroups>, read once when the library is loaded: the initial cap
struct GridCapEnvSwitch {
    GridCapEnvSwitch() {
        const char* g = getenv("S2SR_GRID_CAP");
        if (!g || !*g) return;
        char* end = nullptr;
        const long long v = strtoll(g, &end, 10);
        if (end == g || *end || !set_cap(v))
            fprintf(stderr, "s2sr: S2SR_GRID_CAP=%s is not a number of workgroups in 0..%d: the grid cap stays off\n", g, kMaxCap);
    }
} g_grid_cap_env_switch;

}  // namespace

void s2sr::grid_cap_note(int fam, long long items, int grid) {
    if (fam < 0 || fam >= GF_COUNT || grid < 1) return;
    const long long trips = (items + grid - 1) / grid;
    g_launches[fam].fetch_add(1, std::memory_order_relaxed);
    long long seen = g_trips[fam].load(std::memory_order_relaxed);
    while (trips > seen && !g_trips[fam].compare_exchange_weak(seen, trips, std::memory_order_relaxed)) {}
}

extern "C" {

static_assert(GF_COUNT == S2SR_GRID_CAP_FAMILIES, "include/s2sr.h states the number of families");

int s2sr_debug_grid_cap(int32_t workgroups) {
    if (!set_cap(workgroups)) return fail(nullptr, S2SR_E_INVALID, "the grid cap must be 0 (off) or 1..1048576 workgroups");
    return S2SR_OK;
}

int32_t s2sr_debug_grid_cap_workgroups(void) { return g_grid_cap.load(); }

int s2sr_debug_grid_cap_stats(int64_t* launches, int64_t* max_trips, int32_t cap, int32_t* n) {
    if (!launches || !max_trips || !n || cap < GF_COUNT) return fail(nullptr, S2SR_E_INVALID, "s2sr_debug_grid_cap_stats: room for S2SR_GRID_CAP_FAMILIES entries");
    for (int i = 0; i < GF_COUNT; ++i) {
        launches[i] = g_launches[i].load();
        max_trips[i] = g_trips[i].load();
    }
    *n = GF_COUNT;
    return S2SR_OK;
}

void s2sr_debug_grid_cap_stats_reset(void) {
    for (int i = 0; i < GF_COUNT; ++i) {
        g_launches[i].store(0);
        g_trips[i].store(0);
    }
}

const char* s2sr_debug_grid_cap_family(int32_t i) { return i >= 0 && i < GF_COUNT ? kGridFamName[i] : nullptr; }

}  // extern "C"
