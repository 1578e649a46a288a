// rc_stream_slots.h -- the per-stream pool behind the scene's stack spill regions and totals scratch areas (rc_internal.h).  No HIP
// header: a plain host compiler builds it (tests/host/stream_slots_main.cpp).
#pragma once
#include <algorithm>
#include <vector>

// The entry of `pool` that belongs to `stream`: launches on one stream are ordered and share an entry, another stream gets its own, up to
// N.  One stream too many takes over the first entry (index order: oldest first) whose last user is done, else waits for entry 0's.  A
// taken entry moves to the back and is re-keyed; its payload -- a buffer that only grows -- stays with it.  Entry: `.stream`, and `.last`
// with idle() (never blocks) and wait().  *fresh: the entry was appended by this call.
template <int N, class Entry>
Entry& rc_stream_slot(std::vector<Entry>& pool, decltype(Entry::stream) stream, bool* fresh = nullptr) {
    if (fresh) *fresh = false;
    for (Entry& e : pool)
        if (e.stream == stream) return e;
    if (pool.size() < (size_t)N) {
        pool.emplace_back();
        if (fresh) *fresh = true;
    } else {
        size_t victim = 0;
        while (victim < pool.size() && !pool[victim].last.idle()) ++victim;
        if (victim == pool.size()) { victim = 0; pool[0].last.wait(); }
        std::rotate(pool.begin() + victim, pool.begin() + victim + 1, pool.end());
    }
    pool.back().stream = stream;
    return pool.back();
}
