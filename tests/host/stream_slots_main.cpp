// Stand-alone check of rc_stream_slot (raycore.jl_amd/csrc/rc_stream_slots.h), the per-stream pool behind the scene's stack spill regions
// and totals scratch areas, on a fake entry whose `last` is scripted.  Built and run by tests/test_stream_slots.py; no HIP, no GPU.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "rc_stream_slots.h"

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } } while (0)

namespace {
struct FakeLast {
    bool is_idle = false;
    mutable int waits = 0;
    bool idle() const { return is_idle; }
    void wait() const { ++waits; }
};
struct Entry {
    int stream = 0;
    int payload = 0;  // stands for the entry's buffer
    FakeLast last;
};
constexpr int N = 3;
using Pool = std::vector<Entry>;

// streams 1, 2, 3 with payloads 101, 102, 103, all busy
Pool full_pool() {
    Pool pool;
    for (int st = 1; st <= N; ++st) {
        bool fresh = false;
        Entry& e = rc_stream_slot<N>(pool, st, &fresh);
        CHECK(fresh && e.stream == st && &e == &pool.back());
        e.payload = 100 + st;
    }
    CHECK(pool.size() == (size_t)N);
    return pool;
}
int total_waits(const Pool& pool) { int w = 0; for (const Entry& e : pool) w += e.last.waits; return w; }
}  // namespace

int main() {
    {   // the same stream twice: the same entry, the pool does not grow
        Pool pool;
        pool.reserve(N);  // (as the scene does: entries never move while the pool fills)
        bool fresh = false;
        Entry* a = &rc_stream_slot<N>(pool, 7, &fresh);
        CHECK(fresh && pool.size() == 1);
        Entry* b = &rc_stream_slot<N>(pool, 7, &fresh);
        CHECK(a == b && !fresh && pool.size() == 1);
        Entry* c = &rc_stream_slot<N>(pool, 8);
        CHECK(c != a && pool.size() == 2 && &rc_stream_slot<N>(pool, 7) == a && &rc_stream_slot<N>(pool, 8) == c && pool.size() == 2);
        CHECK(total_waits(pool) == 0);
    }
    {   // a fourth stream with only entry 1 idle takes entry 1 without waiting: old 0, old 2, the new one
        Pool pool = full_pool();
        pool[1].last.is_idle = true;
        bool fresh = true;
        Entry& e = rc_stream_slot<N>(pool, 4, &fresh);
        CHECK(!fresh && pool.size() == (size_t)N && &e == &pool[2]);
        CHECK(pool[0].stream == 1 && pool[1].stream == 3 && pool[2].stream == 4);
        CHECK(pool[0].payload == 101 && pool[1].payload == 103 && pool[2].payload == 102);  // a taken entry keeps its payload
        CHECK(total_waits(pool) == 0);
        // the evicted stream is a miss: it takes over an entry (nothing idle but the one just taken: that one), it does not find its old one
        Entry& back = rc_stream_slot<N>(pool, 2);
        CHECK(pool.size() == (size_t)N && &back == &pool[2] && back.stream == 2 && back.payload == 102 && total_waits(pool) == 0);
        CHECK(pool[0].stream == 1 && pool[1].stream == 3);
    }
    {   // the first idle entry in index order wins
        Pool pool = full_pool();
        pool[1].last.is_idle = pool[2].last.is_idle = true;
        Entry& e = rc_stream_slot<N>(pool, 4);
        CHECK(e.payload == 102 && pool[0].stream == 1 && pool[1].stream == 3 && pool[2].stream == 4 && total_waits(pool) == 0);
    }
    {   // a fourth stream with nothing idle waits exactly once, on entry 0, and takes it
        Pool pool = full_pool();
        Entry& e = rc_stream_slot<N>(pool, 4);
        CHECK(pool.size() == (size_t)N && &e == &pool[2] && e.stream == 4 && e.payload == 101 && e.last.waits == 1);
        CHECK(pool[0].stream == 2 && pool[1].stream == 3 && pool[0].last.waits == 0 && pool[1].last.waits == 0);
        // the evicted stream comes back: a miss again, the oldest entry (stream 2's) goes after one more wait
        Entry& back = rc_stream_slot<N>(pool, 1);
        CHECK(&back == &pool[2] && back.stream == 1 && back.payload == 102 && back.last.waits == 1 && total_waits(pool) == 2);
        CHECK(pool[0].stream == 3 && pool[1].stream == 4 && pool[1].payload == 101);
        // streams that own an entry are still hits and wait for nothing
        CHECK(&rc_stream_slot<N>(pool, 3) == &pool[0] && &rc_stream_slot<N>(pool, 4) == &pool[1] && total_waits(pool) == 2);
    }
    std::puts("stream slots ok");
    return 0;
}
