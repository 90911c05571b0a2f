// The book-keeping of a handle's scratch slots (host-only; no HIP in this file): pointer and capacity per slot, the one record of
// what the last call left on the device for the next one, the guard over the slot a call reads such a result from, and the rule
// for what a scratch request voids.  What the slots hold is the engine's business (the table at enum Slot, engine_internal.h).
// Memory is reached through the two callbacks of DeviceMem only, as csrc/redzone.h reaches the device, so
// tests/native/scratch_main.cpp runs the same code on exact-size heap blocks under ASan / UBSan.
#pragma once
#include <stddef.h>

namespace s2sr::slots {

constexpr int kSlots = 8;
constexpr int kAllSlots = -1;      // Book::drop: every slot at once
constexpr int kTakenRegrow = -1000;   // Book::request: the slot is the one this call took its kept input from and would have to move

// What a call may leave on the device for the next call on the handle: a warped RGBA raster [a, b, 4] (a rows, b columns), a tile
// level of a x b tiles (nx, ny), a uint16 image [a, b, 3].
enum Kind { KEPT_NONE, KEPT_RASTER, KEPT_LEVEL, KEPT_U16 };
struct Kept {
    Kind kind = KEPT_NONE;
    int slot = -1, a = 0, b = 0;
};

struct DeviceMem {
    int (*alloc)(void* ctx, void** p, size_t bytes);   // 0, or the error code request() hands on
    int (*release)(void* ctx, void* p);                // nothing queued reads p any more on return; 0, or the error code
    void* ctx;
};

struct Book {
    void* ptr[kSlots] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    size_t cap[kSlots] = {0, 0, 0, 0, 0, 0, 0, 0};
    Kept kept;                 // at most one result is ever kept: every keep() runs behind its call's own requests, which drop the one before
    int taken = -1;            // the slot the running call reads its kept input from (take .. release)
    bool run_open = false;     // a banded post-process run is open in slot `run_slot`
    int run_slot;
    explicit Book(int run_slot_) : run_slot(run_slot_) {}

    // THE void rule.  Whoever asks for scratch is about to overwrite it: what the last call kept is gone, whichever slot is asked
    // for (the doors that keep something say so again at their end), and a request for the run's slot ends the run.
    void drop(int slot) {
        kept = Kept();
        if (slot == run_slot || slot == kAllSlots) run_open = false;
    }
    // A call's first words about its kept input: the slot that holds a `kind` of a x b, guarded until release(); -1 when the last
    // call left no such thing (the record stays as it is: the caller refuses).
    int take(Kind kind, int a, int b) {
        if (kind == KEPT_NONE || kept.kind != kind || kept.a != a || kept.b != b) return -1;
        return taken = kept.slot;
    }
    void release() { taken = -1; }
    // a door's successful end: this is what it leaves (a consumer that keeps its input intact names it again)
    void keep(Kind kind, int slot, int a, int b) { kept.kind = kind; kept.slot = slot; kept.a = a; kept.b = b; }
    // `bytes` in `slot`.  Within capacity nothing moves; a larger request releases the old block and allocates the new size.
    int request(const DeviceMem& m, int slot, size_t bytes) {
        drop(slot);
        if (cap[slot] >= bytes) return 0;
        if (slot == taken) return kTakenRegrow;
        if (ptr[slot]) {
            if (int rc = m.release(m.ctx, ptr[slot])) return rc;
            ptr[slot] = nullptr;
            cap[slot] = 0;
        }
        if (int rc = m.alloc(m.ctx, &ptr[slot], bytes)) return rc;
        cap[slot] = bytes;
        return 0;
    }
};

}  // namespace s2sr::slots
