// Stand-alone driver of csrc/scratch.h (the book-keeping of a handle's scratch slots: capacity, the kept record, the taken-input
// guard, the void rule), built with -fsanitize=address,undefined by tests/test_scratch_cpu.py.  The "device" is the heap: every
// slot is an exact-size malloc block, so a block freed twice, leaked or used after its release is reported.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <initializer_list>

#include "scratch.h"

using namespace s2sr::slots;

static int failures = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) { printf("line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

static int g_allocs = 0, g_frees = 0, g_fail_alloc = 0, g_fail_free = 0;
static void* g_last_freed = nullptr;
static int mem_alloc(void*, void** p, size_t bytes) {
    if (g_fail_alloc) return g_fail_alloc;
    *p = malloc(bytes);
    memset(*p, 0xAB, bytes);          // every byte of the block is the slot's
    ++g_allocs;
    return 0;
}
static int mem_release(void*, void* p) {
    if (g_fail_free) return g_fail_free;
    g_last_freed = p;
    free(p);
    ++g_frees;
    return 0;
}
static const DeviceMem kMem{mem_alloc, mem_release, nullptr};
constexpr int kRun = 5;               // the slot a banded run lives in, as the engine's SL_PP

static void free_all(Book& b) {
    for (int i = 0; i < kSlots; ++i)
        if (b.ptr[i]) free(b.ptr[i]);
}

static void test_capacity_and_regrow() {
    Book b(kRun);
    g_allocs = g_frees = 0;
    EXPECT(b.request(kMem, 2, 100) == 0 && g_allocs == 1 && g_frees == 0 && b.cap[2] == 100 && b.ptr[2]);
    void* p = b.ptr[2];
    memset(p, 1, 100);
    for (size_t n : {(size_t)100, (size_t)1, (size_t)0, (size_t)99}) {           // within capacity: nothing moves
        EXPECT(b.request(kMem, 2, n) == 0 && b.ptr[2] == p && b.cap[2] == 100);
    }
    EXPECT(g_allocs == 1 && g_frees == 0);
    EXPECT(b.request(kMem, 2, 101) == 0);                                        // larger: the old block goes exactly once
    EXPECT(g_allocs == 2 && g_frees == 1 && g_last_freed == p && b.cap[2] == 101);
    memset(b.ptr[2], 2, 101);
    EXPECT(b.request(kMem, 0, 7) == 0 && g_allocs == 3 && g_frees == 1);         // another slot: this one stays
    EXPECT(b.cap[2] == 101 && b.cap[0] == 7);
    // a failing release keeps the block; a failing allocation leaves the slot empty, and the next request fills it
    void* q = b.ptr[2];
    g_fail_free = -3;
    EXPECT(b.request(kMem, 2, 500) == -3 && b.ptr[2] == q && b.cap[2] == 101 && g_frees == 1);
    g_fail_free = 0;
    g_fail_alloc = -5;
    EXPECT(b.request(kMem, 2, 500) == -5 && b.ptr[2] == nullptr && b.cap[2] == 0 && g_frees == 2);
    g_fail_alloc = 0;
    EXPECT(b.request(kMem, 2, 500) == 0 && b.cap[2] == 500 && g_frees == 2 && g_allocs == 4);
    memset(b.ptr[2], 3, 500);
    free_all(b);
}

static void test_any_request_voids_the_record() {
    for (int slot = 0; slot < kSlots; ++slot) {
        Book b(kRun);
        EXPECT(b.request(kMem, slot, 64) == 0);
        b.keep(KEPT_LEVEL, 1, 3, 2);
        b.run_open = true;
        EXPECT(b.request(kMem, slot, 8) == 0);                                   // within capacity, and still: the record is gone
        EXPECT(b.kept.kind == KEPT_NONE && b.kept.slot == -1);
        EXPECT(b.take(KEPT_LEVEL, 3, 2) == -1);
        EXPECT(b.run_open == (slot != kRun));                                    // only the run's slot ends the run
        free_all(b);
    }
    // a request that fails voids as well: the caller was about to overwrite
    Book b(kRun);
    b.keep(KEPT_U16, 0, 8, 8);
    g_fail_alloc = -5;
    EXPECT(b.request(kMem, 3, 10) == -5 && b.kept.kind == KEPT_NONE);
    g_fail_alloc = 0;
}

static void test_take_and_keep() {
    Book b(kRun);
    EXPECT(b.take(KEPT_NONE, 0, 0) == -1 && b.take(KEPT_RASTER, 0, 0) == -1 && b.taken == -1);   // nothing kept
    EXPECT(b.request(kMem, 0, 64) == 0 && b.request(kMem, 1, 64) == 0);
    b.keep(KEPT_RASTER, 1, 4, 6);
    // the wrong kind, the wrong size, the sizes exchanged: refused, and the record is what it was
    EXPECT(b.take(KEPT_LEVEL, 4, 6) == -1 && b.take(KEPT_U16, 4, 6) == -1 && b.take(KEPT_NONE, 4, 6) == -1);
    EXPECT(b.take(KEPT_RASTER, 4, 5) == -1 && b.take(KEPT_RASTER, 6, 4) == -1);
    EXPECT(b.taken == -1 && b.kept.kind == KEPT_RASTER && b.kept.slot == 1 && b.kept.a == 4 && b.kept.b == 6);
    EXPECT(b.take(KEPT_RASTER, 4, 6) == 1 && b.taken == 1);
    EXPECT(b.kept.kind == KEPT_RASTER);                                          // taking does not consume: the requests do
    // the consumer's own requests drop the record; keep() at its end restores it (the input is intact), or names the result
    EXPECT(b.request(kMem, 0, 32) == 0 && b.request(kMem, 3, 16) == 0 && b.kept.kind == KEPT_NONE);
    b.keep(KEPT_RASTER, 1, 4, 6);
    b.release();
    EXPECT(b.take(KEPT_RASTER, 4, 6) == 1);
    b.release();
    EXPECT(b.request(kMem, 0, 32) == 0);
    b.keep(KEPT_LEVEL, 0, 1, 1);
    EXPECT(b.take(KEPT_RASTER, 4, 6) == -1 && b.take(KEPT_LEVEL, 1, 1) == 0);
    b.release();
    EXPECT(b.taken == -1);
    free_all(b);
}

static void test_taken_slot_does_not_move() {
    Book b(kRun);
    g_allocs = g_frees = 0;
    EXPECT(b.request(kMem, 1, 64) == 0);
    void* p = b.ptr[1];
    b.keep(KEPT_U16, 1, 2, 2);
    EXPECT(b.take(KEPT_U16, 2, 2) == 1);
    EXPECT(b.request(kMem, 1, 64) == 0 && b.ptr[1] == p);                        // within capacity: allowed (and it voids)
    EXPECT(b.request(kMem, 1, 65) == kTakenRegrow);                              // would move what queued work reads: refused
    EXPECT(b.ptr[1] == p && b.cap[1] == 64 && g_frees == 0 && g_allocs == 1);
    memset(p, 7, 64);                                                            // the block is live
    EXPECT(b.request(kMem, 0, 1000) == 0 && g_allocs == 2);                      // the other slots grow as ever
    b.release();                                                                 // the call is over: the slot may move again
    EXPECT(b.request(kMem, 1, 65) == 0 && g_frees == 1 && g_last_freed == p && b.cap[1] == 65);
    free_all(b);
}

static void test_drop_all_slots() {
    Book b(kRun);
    EXPECT(b.request(kMem, 4, 10) == 0);
    void* p = b.ptr[4];
    b.keep(KEPT_LEVEL, 0, 2, 2);
    b.run_open = true;
    b.drop(kAllSlots);                                                           // what s2sr_debug_poison_scratch does
    EXPECT(b.kept.kind == KEPT_NONE && !b.run_open && b.take(KEPT_LEVEL, 2, 2) == -1);
    EXPECT(b.ptr[4] == p && b.cap[4] == 10);                                     // the memory is not its business
    b.keep(KEPT_LEVEL, 0, 2, 2);
    b.run_open = true;
    b.drop(3);
    EXPECT(b.kept.kind == KEPT_NONE && b.run_open);
    b.drop(kRun);
    EXPECT(!b.run_open);
    free_all(b);
}

int main() {
    test_capacity_and_regrow();
    test_any_request_voids_the_record();
    test_take_and_keep();
    test_taken_slot_does_not_move();
    test_drop_all_slots();
    if (failures) { printf("%d failure(s)\n", failures); return 1; }
    printf("ok\n");
    return 0;
}
