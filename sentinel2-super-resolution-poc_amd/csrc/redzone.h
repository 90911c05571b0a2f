// Red zones around device buffers (host-only; no HIP in this file): the registry of live zoned allocations and the pattern
// logic of the diagnostic mode behind s2sr_debug_redzone (include/s2sr.h).  A zoned allocation is [front zone | user bytes |
// back zone]; a zone holds a position-dependent pattern, and a byte that no longer matches was written by somebody who had no
// business there -- a store a few bytes in front of or behind the buffer it belongs to, which no parity test reads.
// The device is reached through the two callbacks of DeviceIo only, so tests/native/redzone_main.cpp runs the same code on
// malloc'ed blocks under ASan / UBSan.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <mutex>
#include <string>
#include <vector>

namespace s2sr::redzone {

// Byte i of a zone.  Never zero (the halos and the allocation-time memset are zeros), never constant, and different at
// i and i + k for every small shift k (167 is odd; the row term moves every 256 bytes), so a shifted copy of a zone does not pass.
// Front and back zones differ, so one copied over the other does not pass either.
inline uint8_t pattern(bool back, size_t i) {
    return (uint8_t)(((i * 167u + (i >> 8) * 13u + (back ? 0xA7u : 0x5Bu)) & 0xFFu) | 1u);
}

struct DeviceIo {
    bool (*write)(void* ctx, void* dst, const uint8_t* src, size_t n);   // host -> device, complete on return
    bool (*read)(void* ctx, uint8_t* dst, const void* src, size_t n);    // device -> host, complete on return
    void* ctx;
};

// One live allocation: `front` zone bytes end at `user`, `back` zone bytes start at user + bytes.  parent: the user pointer of
// the allocation this record lies inside (a workspace plane and the zone behind it), nullptr for an allocation of its own.
struct Record {
    char* user = nullptr;
    size_t bytes = 0, front = 0, back = 0;
    const void* parent = nullptr;
    char* base() const { return user - front; }
};

struct Damage {
    const void* user = nullptr;
    size_t bytes = 0;       // user bytes of the allocation
    bool back = false;
    size_t offset = 0;      // of the first damaged byte, from the start of that zone
    uint8_t found = 0, expected = 0;
    std::string describe() const {
        char b[200];
        snprintf(b, sizeof b, "redzone: allocation of %zu bytes, %s zone damaged at offset %zu: found 0x%02x, expected 0x%02x",
                 bytes, back ? "back" : "front", offset, (unsigned)found, (unsigned)expected);
        return b;
    }
};

class Registry {
public:
    // pattern both zones of [user - front, user + bytes + back) and record the allocation; false: a callback failed (nothing recorded)
    bool add(const DeviceIo& io, void* user, size_t bytes, size_t front, size_t back, const void* parent = nullptr) {
        Record r;
        r.user = (char*)user; r.bytes = bytes; r.front = front; r.back = back; r.parent = parent;
        if (!fill(io, r, false) || !fill(io, r, true)) return false;
        std::lock_guard<std::mutex> lk(mu_);
        live_.push_back(r);
        return true;
    }
    bool find(const void* user, Record* out = nullptr) const {
        std::lock_guard<std::mutex> lk(mu_);
        for (const Record& r : live_)
            if (r.user == user && !r.parent) {
                if (out) *out = r;
                return true;
            }
        return false;
    }
    // The allocation `user` is about to be freed: check its zones and those of the records inside it, add what is damaged to
    // the sticky record, forget them all.  false: never registered (out untouched).  *io_ok: every read-back worked.
    bool remove(const DeviceIo& io, const void* user, Record* out, bool* io_ok = nullptr) {
        std::vector<Record> gone;
        {
            std::lock_guard<std::mutex> lk(mu_);
            bool found = false;
            for (const Record& r : live_) found = found || (r.user == user && !r.parent);
            if (!found) return false;
            auto mine = [&](const Record& r) { return (r.user == user && !r.parent) || r.parent == user; };
            for (const Record& r : live_)
                if (mine(r)) gone.push_back(r);
            live_.erase(std::remove_if(live_.begin(), live_.end(), mine), live_.end());
        }
        bool ok = true;
        for (const Record& r : gone) {
            if (!r.parent) *out = r;
            Damage d;
            size_t zones = 0;
            ok = check_record(io, r, &zones, &d) && ok;
            std::lock_guard<std::mutex> lk(mu_);
            ++total_checked_;
            if (zones) {
                if (!sticky_zones_) sticky_first_ = d;
                sticky_zones_ += zones;
                total_damaged_ += zones;
            }
        }
        if (io_ok) *io_ok = ok;
        return true;
    }
    // Check every live record.  *allocations: records checked; *damaged: damaged zones among them plus the sticky record (zones
    // found damaged at a free since the last check), which is cleared; *first: the first damage, live records before the sticky
    // one.  Damaged zones are patterned again, so the next check is clean.  false: a callback failed.
    bool check_all(const DeviceIo& io, size_t* allocations, size_t* damaged, Damage* first) {
        std::vector<Record> recs;
        {
            std::lock_guard<std::mutex> lk(mu_);
            recs = live_;
        }
        size_t bad = 0;
        bool ok = true;
        for (const Record& r : recs) {
            Damage d;
            size_t zones = 0;
            ok = check_record(io, r, &zones, &d, true) && ok;
            if (zones && !bad && first) *first = d;
            bad += zones;
        }
        std::lock_guard<std::mutex> lk(mu_);
        total_checked_ += recs.size();
        total_damaged_ += bad;
        if (sticky_zones_ && !bad && first) *first = sticky_first_;
        bad += sticky_zones_;
        sticky_zones_ = 0;
        if (allocations) *allocations = recs.size();
        if (damaged) *damaged = bad;
        return ok;
    }
    size_t planes(const void* parent) const {   // records inside the allocation `parent`
        std::lock_guard<std::mutex> lk(mu_);
        size_t n = 0;
        for (const Record& r : live_) n += r.parent == parent;
        return n;
    }
    size_t live() const { std::lock_guard<std::mutex> lk(mu_); return live_.size(); }
    size_t sticky() const { std::lock_guard<std::mutex> lk(mu_); return sticky_zones_; }
    // since the process started: records checked (at a free or by check_all) and damaged zones found
    void totals(size_t* checked, size_t* damaged) const {
        std::lock_guard<std::mutex> lk(mu_);
        *checked = total_checked_; *damaged = total_damaged_;
    }

private:
    static bool fill(const DeviceIo& io, const Record& r, bool back) {
        const size_t n = back ? r.back : r.front;
        if (!n) return true;
        std::vector<uint8_t> buf(n);
        for (size_t i = 0; i < n; ++i) buf[i] = pattern(back, i);
        return io.write(io.ctx, back ? r.user + r.bytes : r.user - r.front, buf.data(), n);
    }
    // *zones += damaged zones of r (0..2); *first: the first damaged byte (front before back), written when *zones was 0
    static bool check_record(const DeviceIo& io, const Record& r, size_t* zones, Damage* first, bool refill = false) {
        bool ok = true;
        for (int side = 0; side < 2; ++side) {
            const bool back = side == 1;
            const size_t n = back ? r.back : r.front;
            if (!n) continue;
            std::vector<uint8_t> buf(n);
            if (!io.read(io.ctx, buf.data(), back ? r.user + r.bytes : r.user - r.front, n)) { ok = false; continue; }
            for (size_t i = 0; i < n; ++i) {
                if (buf[i] == pattern(back, i)) continue;
                if (!*zones && first) {
                    first->user = r.user; first->bytes = r.bytes; first->back = back; first->offset = i;
                    first->found = buf[i]; first->expected = pattern(back, i);
                }
                ++*zones;
                if (refill) ok = fill(io, r, back) && ok;
                break;
            }
        }
        return ok;
    }

    mutable std::mutex mu_;
    std::vector<Record> live_;
    size_t sticky_zones_ = 0, total_checked_ = 0, total_damaged_ = 0;
    Damage sticky_first_;
};

}  // namespace s2sr::redzone

// Poisoned memory (the diagnostic mode behind s2sr_debug_poison, include/s2sr.h): the bytes an allocation hands out, and the bytes a
// scratch slot keeps between calls, are filled with a pattern that is never the zeros fresh memory reads as, so a kernel that reads
// in-bounds bytes nobody wrote in this call computes something visibly different.  The pattern and the fill live here, host-only and
// reached through the same two callbacks, so tests/native/poison_main.cpp runs them on exact-size heap blocks under ASan / UBSan.
namespace s2sr::poison {

constexpr int kOff = 0, kOnes = 1, kPositional = 2;
inline bool valid(int64_t pat) { return pat >= kOff && pat <= kPositional; }

// Byte i of a poisoned range.  Pattern 1: 0xFF everywhere -- a NaN in fp32 and fp16, the e4m3 NaN code, -1 as an int32 (an index
// that was never uploaded points in front of its table), 255 as a u8.  Pattern 2: the front-zone pattern of the red zones, non-zero
// and different from byte to byte, so a value assembled from stale bytes differs from one position to the next.
inline uint8_t byte_at(int pat, size_t i) { return pat == kOnes ? (uint8_t)0xFF : redzone::pattern(false, i); }

// The fill goes out in chunks of kChunk bytes; pattern 2 repeats every 65536 bytes (167 * 65536 and 13 * 256 are multiples of
// 256), so one chunk's bytes serve every chunk.
constexpr size_t kPeriod = 65536, kChunk = 16 * kPeriod;

// fill [dst, dst + bytes) with pattern `pat` (kOff: nothing is written); false: a callback failed
inline bool fill(const redzone::DeviceIo& io, void* dst, size_t bytes, int pat) {
    if (pat == kOff || !bytes) return true;
    std::vector<uint8_t> buf(std::min(bytes, kChunk));
    for (size_t i = 0; i < buf.size(); ++i) buf[i] = byte_at(pat, i);
    for (size_t o = 0; o < bytes; o += kChunk)
        if (!io.write(io.ctx, (char*)dst + o, buf.data(), std::min(kChunk, bytes - o))) return false;
    return true;
}

// *first: the offset of the first byte of [src, src + bytes) that does not hold pattern `pat`, `bytes` when all do; false: a callback failed
inline bool first_unpoisoned(const redzone::DeviceIo& io, const void* src, size_t bytes, int pat, size_t* first) {
    std::vector<uint8_t> buf(std::min(bytes, kChunk));
    *first = bytes;
    for (size_t o = 0; o < bytes; o += kChunk) {
        const size_t n = std::min(kChunk, bytes - o);
        if (!io.read(io.ctx, buf.data(), (const char*)src + o, n)) return false;
        for (size_t i = 0; i < n; ++i)
            if (buf[i] != byte_at(pat, o + i)) { *first = o + i; return true; }
    }
    return true;
}

}  // namespace s2sr::poison
