// Stand-alone driver of csrc/redzone.h (the registry and pattern logic of the library's red-zone mode), built with
// -fsanitize=address,undefined by tests/test_redzone_cpu.py.  The "device" is the heap: every allocation is an exact-size malloc
// block of front + bytes + back, and the two callbacks are memcpy, so a fill or a read-back one byte past a zone is reported.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "redzone.h"

using namespace s2sr::redzone;

static int failures = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) { printf("line %d: %s\n", __LINE__, #cond); ++failures; } \
    } while (0)

static size_t g_writes = 0, g_reads = 0;
static bool io_write(void*, void* dst, const uint8_t* src, size_t n) { memcpy(dst, src, n); ++g_writes; return true; }
static bool io_read(void*, uint8_t* dst, const void* src, size_t n) { memcpy(dst, src, n); ++g_reads; return true; }
static bool io_fail(void*, void*, const uint8_t*, size_t) { return false; }
static const DeviceIo kIo{io_write, io_read, nullptr};

// what dev_malloc does: base = malloc(bytes + 2 Z), zones patterned, user = base + Z
static char* zoned_malloc(Registry& reg, size_t bytes, size_t Z) {
    char* base = (char*)malloc(bytes + 2 * Z);
    memset(base, 0, bytes + 2 * Z);
    EXPECT(reg.add(kIo, base + Z, bytes, Z, Z));
    return base + Z;
}
// what dev_free does: look up, check, free the base; a pointer that was never registered is freed as it is
static void zoned_free(Registry& reg, char* user) {
    Record r;
    if (!reg.remove(kIo, user, &r)) { free(user); return; }
    EXPECT(r.user == user);
    free(r.base());
}

struct Check { size_t n = 0, bad = 0; Damage d; };
static Check check(Registry& reg) {
    Check c;
    EXPECT(reg.check_all(kIo, &c.n, &c.bad, &c.d));
    return c;
}

static void test_pattern() {
    const size_t Z = 65536;
    bool constant = true;
    for (int back = 0; back < 2; ++back)
        for (size_t i = 0; i < Z; ++i) {
            EXPECT(pattern(back, i) != 0);
            constant = constant && pattern(back, i) == pattern(back, 0);
        }
    EXPECT(!constant);
    // a copy of a zone shifted by k bytes differs from the zone (somewhere in every 4 KiB), and front differs from back
    for (int back = 0; back < 2; ++back)
        for (size_t k : {1, 2, 3, 4, 8, 16, 24, 32, 48, 64, 128, 256, 512, 1024, 2048, 4096, 6144}) {
            size_t diff = 0;
            for (size_t i = 0; i + k < 8192; ++i) diff += pattern(back, i) != pattern(back, i + k);
            EXPECT(diff > 0);
        }
    size_t diff = 0;
    for (size_t i = 0; i < 4096; ++i) diff += pattern(false, i) != pattern(true, i);
    EXPECT(diff > 0);
}

static void test_every_order() {
    const size_t Z = 4096, sizes[3] = {1, 777, 8192};
    int order[3] = {0, 1, 2};
    do {
        Registry reg;
        char* p[3];
        for (int i = 0; i < 3; ++i) {
            p[i] = zoned_malloc(reg, sizes[i], Z);
            memset(p[i], 0xEE, sizes[i]);                      // the user range is the user's: writing all of it damages nothing
            Check c = check(reg);
            EXPECT(c.n == (size_t)i + 1 && c.bad == 0);
        }
        for (int k = 0; k < 3; ++k) {
            Record r;
            EXPECT(reg.find(p[order[k]], &r) && r.bytes == sizes[order[k]] && r.front == Z && r.back == Z);
            zoned_free(reg, p[order[k]]);
            EXPECT(!reg.find(p[order[k]]));
            Check c = check(reg);
            EXPECT(c.n == (size_t)(2 - k) && c.bad == 0);
        }
        EXPECT(reg.live() == 0 && reg.sticky() == 0);
        size_t n = 0, m = 0;
        reg.totals(&n, &m);
        EXPECT(m == 0 && n == 3 + (1 + 2 + 3) + (2 + 1 + 0));
    } while (std::next_permutation(order, order + 3));
}

static void test_damage_edges_and_refill() {
    const size_t Z = 8192, bytes = 1001;
    Registry reg;
    char* a = zoned_malloc(reg, 300, Z);
    char* u = zoned_malloc(reg, bytes, Z);
    struct { bool back; size_t off; } cases[4] = {{false, 0}, {false, Z - 1}, {true, 0}, {true, Z - 1}};
    for (auto& cs : cases) {
        char* at = cs.back ? u + bytes + cs.off : u - Z + cs.off;
        const uint8_t good = (uint8_t)*at;
        EXPECT(good == pattern(cs.back, cs.off));
        *at = (char)(uint8_t)~good;
        Check c = check(reg);
        EXPECT(c.n == 2 && c.bad == 1);
        EXPECT(c.d.user == u && c.d.bytes == bytes && c.d.back == cs.back && c.d.offset == cs.off);
        EXPECT(c.d.found == (uint8_t)~good && c.d.expected == good);
        const std::string s = c.d.describe();
        EXPECT(s.find(cs.back ? "back zone" : "front zone") != std::string::npos);
        EXPECT(s.find("allocation of 1001 bytes") != std::string::npos);
        EXPECT(s.find("offset " + std::to_string(cs.off) + ":") != std::string::npos);
        EXPECT((uint8_t)*at == good);                          // the report re-filled the zone ...
        c = check(reg);
        EXPECT(c.bad == 0);                                    // ... so the next check is clean
    }
    // both zones of one allocation, and a zero written into a zone (zeros are what halos and fresh memory hold)
    u[-1] = 0; u[bytes] = 0;
    Check c = check(reg);
    EXPECT(c.bad == 2 && c.d.back == false && c.d.offset == Z - 1 && c.d.found == 0);
    EXPECT(check(reg).bad == 0);
    // a zone overwritten by a shifted copy of itself, and by the other zone
    memmove(u + bytes + 16, u + bytes, Z - 16);
    EXPECT(check(reg).bad == 1);
    memcpy(u + bytes, u - Z, Z);
    c = check(reg);
    EXPECT(c.bad == 1 && c.d.back);
    EXPECT(check(reg).bad == 0);
    zoned_free(reg, u);
    zoned_free(reg, a);
    EXPECT(reg.sticky() == 0);
}

static void test_sticky_after_free() {
    const size_t Z = 4096;
    Registry reg;
    char* keep = zoned_malloc(reg, 64, Z);
    char* u = zoned_malloc(reg, 500, Z);
    u[500 + 17] ^= 0x40;
    u[-Z] ^= 0x01;
    zoned_free(reg, u);                                        // the damage is found at the free ...
    EXPECT(reg.sticky() == 2 && reg.live() == 1);
    Check c = check(reg);                                      // ... and reported by the next check, once
    EXPECT(c.n == 1 && c.bad == 2 && c.d.bytes == 500 && !c.d.back && c.d.offset == 0);
    c = check(reg);
    EXPECT(c.bad == 0 && reg.sticky() == 0);
    // live damage is described before remembered damage
    char* v = zoned_malloc(reg, 32, Z);
    v[32] = 0;
    zoned_free(reg, v);
    keep[64 + 5] = 0;
    c = check(reg);
    EXPECT(c.bad == 2 && c.d.bytes == 64 && c.d.back && c.d.offset == 5);
    size_t n = 0, m = 0;
    reg.totals(&n, &m);
    EXPECT(m == 4);
    zoned_free(reg, keep);
}

static void test_never_registered_and_zero() {
    Registry reg;
    char* plain = (char*)malloc(100);
    Record r;
    r.bytes = 12345;
    EXPECT(!reg.find(plain) && !reg.find(nullptr));
    EXPECT(!reg.remove(kIo, plain, &r) && r.bytes == 12345);   // untouched
    zoned_free(reg, plain);                                    // freed as it is
    // Z = 0: an exact-size block, no byte outside it is touched, nothing to damage
    const size_t w0 = g_writes, r0 = g_reads;
    char* z = zoned_malloc(reg, 10, 0);
    EXPECT(reg.find(z, &r) && r.front == 0 && r.back == 0 && r.base() == z);
    memset(z, 0xFF, 10);
    Check c = check(reg);
    EXPECT(c.n == 1 && c.bad == 0);
    zoned_free(reg, z);
    EXPECT(g_writes == w0 && g_reads == r0 && reg.live() == 0);
    // a failing device write registers nothing
    const DeviceIo bad{io_fail, io_read, nullptr};
    char* blk = (char*)malloc(4096 * 2 + 8);
    EXPECT(!reg.add(bad, blk + 4096, 8, 4096, 4096));
    EXPECT(!reg.find(blk + 4096) && reg.live() == 0);
    free(blk);
    c = check(reg);
    EXPECT(c.n == 0 && c.bad == 0);
}

// the workspace: one zoned allocation, planes inside it with a zone behind each (the first plane starts at the user pointer)
static void test_planes() {
    const size_t Z = 4096, pb[3] = {1000, 256, 3000};
    auto align256 = [](size_t v) { return (v + 255) & ~(size_t)255; };
    size_t off[3], total = 0;
    for (int i = 0; i < 3; ++i) { off[i] = total; total += align256(pb[i]) + Z; }
    Registry reg;
    char* ws = zoned_malloc(reg, total, Z);
    for (int i = 0; i < 3; ++i) EXPECT(reg.add(kIo, ws + off[i], pb[i], 0, align256(pb[i]) - pb[i] + Z, ws));
    EXPECT(reg.planes(ws) == 3 && reg.live() == 4);
    for (int i = 0; i < 3; ++i) memset(ws + off[i], 0x11, pb[i]);
    EXPECT(check(reg).bad == 0);
    ws[off[0] + pb[0]] = 0x11;                                 // plane 0 runs one byte long: into the round-up slack
    Check c = check(reg);
    EXPECT(c.n == 4 && c.bad == 1 && c.d.bytes == pb[0] && c.d.back && c.d.offset == 0);
    ws[off[1] - 1] = 0;                                        // the byte in front of plane 1: the end of plane 0's zone
    c = check(reg);
    EXPECT(c.bad == 1 && c.d.bytes == pb[0] && c.d.offset == align256(pb[0]) - pb[0] + Z - 1);
    Record r;
    EXPECT(reg.find(ws, &r) && r.bytes == total && !r.parent);  // the plane at the same address does not hide the allocation
    ws[off[2] + pb[2] + 3] = 0;
    zoned_free(reg, ws);                                       // the planes go with their allocation, checked on the way
    EXPECT(reg.live() == 0 && reg.sticky() == 1);
    c = check(reg);
    EXPECT(c.n == 0 && c.bad == 1 && c.d.bytes == pb[2] && c.d.offset == 3);
}

int main() {
    test_pattern();
    test_every_order();
    test_damage_edges_and_refill();
    test_sticky_after_free();
    test_never_registered_and_zero();
    test_planes();
    if (failures) { printf("%d failure(s)\n", failures); return 1; }
    printf("ok\n");
    return 0;
}
