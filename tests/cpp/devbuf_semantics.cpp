// devbuf_semantics.cpp -- DevBuf (the owning device allocation), Carver (the build arena's slicer) and PinnedReadback (a page-locked block
// + the event of the copy into it) of csrc/rt_internal.h on the host,
// under AddressSanitizer + UndefinedBehaviorSanitizer (tests/test_devbuf_semantics.py).  The header is the product's own; the HIP
// allocator behind it is restated here over malloc, with a count of live blocks and a refusal that can be armed, so that every path
// of reserve / release / adopt / move runs without a device and a block freed twice or never is a sanitizer report or a wrong count.
#include <sanitizer/asan_interface.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>

#include <set>
#include <utility>
#include <vector>

#include "../../dxrexperiments_amd/csrc/rt_internal.h"

static std::set<void *> g_live;          // blocks handed out and not freed yet
static int g_fail_next = 0;              // the next so many hipMalloc calls report an exhausted device
static int g_frees = 0;
static size_t g_limit = ~(size_t)0;
static int g_failures = 0;

extern "C" hipError_t hipMalloc(void **ptr, size_t size)
{
    if (g_fail_next > 0) { g_fail_next--; *ptr = nullptr; return hipErrorOutOfMemory; }
    *ptr = malloc(size);
    g_live.insert(*ptr);
    return hipSuccess;
}
extern "C" hipError_t hipFree(void *ptr)
{
    if (!ptr) return hipSuccess;
    if (!g_live.erase(ptr)) { fprintf(stderr, "hipFree of a block that is not live: %p\n", ptr); g_failures++; return hipErrorInvalidValue; }
    g_frees++;
    free(ptr);
    return hipSuccess;
}
extern "C" hipError_t hipGetLastError(void) { return hipSuccess; }
extern "C" const char *hipGetErrorString(hipError_t e) { return e == hipErrorOutOfMemory ? "out of memory" : "error"; }
void rt_set_error(const char *, ...) {}
size_t &rt_alloc_limit_ref() { return g_limit; }

// ... and the page-locked allocator, events and the asynchronous copy behind PinnedReadback: live counts, a refusal that can be armed on
// each of the two creations, on the copy and on the record; a copy is carried out when a query first finds its event complete
static std::set<void *> g_host, g_events;
static int g_fail_host = 0, g_fail_event = 0, g_fail_copy = 0, g_fail_record = 0;
static int g_host_frees = 0, g_event_destroys = 0;
static bool g_event_complete = false;
static struct { void *dst; const void *src; size_t bytes; } g_copy = {nullptr, nullptr, 0};

extern "C" hipError_t hipHostMalloc(void **ptr, size_t size, unsigned int)
{
    if (g_fail_host > 0) { g_fail_host--; *ptr = nullptr; return hipErrorOutOfMemory; }
    *ptr = malloc(size);
    g_host.insert(*ptr);
    return hipSuccess;
}
extern "C" hipError_t hipHostFree(void *ptr)
{
    if (!g_host.erase(ptr)) { fprintf(stderr, "hipHostFree of a block that is not live: %p\n", ptr); g_failures++; return hipErrorInvalidValue; }
    g_host_frees++;
    if (g_copy.dst == ptr) g_copy.dst = nullptr;       // (the owner has joined the stream: nothing lands any more)
    ASAN_UNPOISON_MEMORY_REGION(ptr, 64);
    free(ptr);
    return hipSuccess;
}
extern "C" hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned flags)
{
    if (flags != hipEventDisableTiming) { fprintf(stderr, "an event that keeps time\n"); g_failures++; }
    if (g_fail_event > 0) { g_fail_event--; *e = nullptr; return hipErrorOutOfMemory; }
    *e = (hipEvent_t)malloc(1);
    g_events.insert(*e);
    return hipSuccess;
}
extern "C" hipError_t hipEventDestroy(hipEvent_t e)
{
    if (!g_events.erase(e)) { fprintf(stderr, "hipEventDestroy of an event that is not live: %p\n", (void *)e); g_failures++; return hipErrorInvalidValue; }
    g_event_destroys++;
    free(e);
    return hipSuccess;
}
extern "C" hipError_t hipMemcpyAsync(void *dst, const void *src, size_t bytes, hipMemcpyKind kind, hipStream_t)
{
    if (g_fail_copy > 0) { g_fail_copy--; return hipErrorInvalidValue; }
    if (kind != hipMemcpyDeviceToHost || !g_host.count(dst)) { fprintf(stderr, "a copy that is no read-back into a live block\n"); g_failures++; }
    g_copy = {dst, src, bytes};
    return hipSuccess;
}
extern "C" hipError_t hipEventRecord(hipEvent_t e, hipStream_t)
{
    if (g_fail_record > 0) { g_fail_record--; return hipErrorInvalidValue; }
    if (!g_events.count(e)) { fprintf(stderr, "record of an event that is not live\n"); g_failures++; }
    g_event_complete = false;
    return hipSuccess;
}
extern "C" hipError_t hipEventQuery(hipEvent_t e)
{
    if (!g_events.count(e)) { fprintf(stderr, "query of an event that is not live\n"); g_failures++; return hipErrorInvalidValue; }
    if (!g_event_complete) return hipErrorNotReady;
    if (g_copy.dst) { memcpy(g_copy.dst, g_copy.src, g_copy.bytes); g_copy.dst = nullptr; }
    return hipSuccess;
}

#define CHECK(cond)                                                             \
    do {                                                                        \
        if (!(cond)) { fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); g_failures++; } \
    } while (0)

static void scope_exit_frees()
{
    {
        DevBuf b;
        CHECK(b.reserve(1000) == RT_OK && b.p && b.bytes == 1000 && !b.borrowed);
        CHECK(g_live.size() == 1);
        CHECK(b.reserve(10) == RT_OK && b.bytes == 1000);          // never shrinks
        DevBuf z;
        CHECK(z.reserve(0) == RT_OK && z.p == nullptr);            // nothing asked, nothing held
    }
    CHECK(g_live.empty());
}

static void move_leaves_the_source_empty()
{
    const int frees = g_frees;
    {
        DevBuf a;
        CHECK(a.reserve(64) == RT_OK);
        void *const block = a.p;
        DevBuf b(std::move(a));
        CHECK(a.p == nullptr && a.bytes == 0 && !a.borrowed);
        CHECK(b.p == block && b.bytes == 64);
        CHECK(g_live.size() == 1);
        DevBuf &same = b;
        b = std::move(same);                                       // self-assignment keeps the block
        CHECK(b.p == block && g_live.size() == 1);
    }
    CHECK(g_live.empty() && g_frees == frees + 1);                 // freed exactly once
}

static void move_assignment_frees_the_old_block()
{
    const int frees = g_frees;
    {
        DevBuf a, b;
        CHECK(a.reserve(64) == RT_OK && b.reserve(128) == RT_OK);
        void *const kept = b.p;
        a = std::move(b);
        CHECK(g_frees == frees + 1 && g_live.size() == 1 && g_live.count(kept));
        CHECK(a.p == kept && a.bytes == 128 && b.p == nullptr && b.bytes == 0);
        std::vector<DevBuf> v;                                     // (what a container does when it grows)
        v.push_back(std::move(a));
        v.emplace_back();
        v.resize(16);
        CHECK(v[0].p == kept && g_live.size() == 1);
    }
    CHECK(g_live.empty() && g_frees == frees + 2);
}

static void an_adopted_slice_is_never_freed()
{
    static char arena[4096];
    const int frees = g_frees;
    {
        DevBuf s;
        s.adopt(arena + 256, 512);
        CHECK(s.p == arena + 256 && s.bytes == 512 && s.borrowed);
        CHECK(s.reserve(512) == RT_OK && s.p == arena + 256);      // fits: stays in the arena
        DevBuf t(std::move(s));                                    // `borrowed` travels with the pointer
        CHECK(t.borrowed && t.p == arena + 256 && !s.borrowed && s.p == nullptr);
        t.release();
        CHECK(t.p == nullptr && !t.borrowed && g_frees == frees);
        t.adopt(arena, 256);
        CHECK(t.reserve(1024) == RT_OK);                           // beyond the slice: a block of its own
        CHECK(!t.borrowed && t.p != arena && t.bytes == 1024 && g_live.size() == 1 && g_frees == frees);
        DevBuf u;
        u.adopt(arena, 128);
        g_fail_next = 2;                                           // the device is full: the slice is NOT given up for a second try
        CHECK(u.reserve(4096) == RT_ERR_OOM && u.p == arena && u.bytes == 128 && u.borrowed);
        CHECK(g_fail_next == 1);
        g_fail_next = 0;
        DevBuf own;
        CHECK(own.reserve(32) == RT_OK);
        own.adopt(arena, 64);                                      // adopting lets go of what it owned
        CHECK(g_live.size() == 1 && g_frees == frees + 1);
    }
    CHECK(g_live.empty() && g_frees == frees + 2);                 // the two own blocks, never the arena (free() of it would be an ASan report)
}

static void a_failed_growth_keeps_the_buffer()
{
    {
        DevBuf b;
        CHECK(b.reserve(100) == RT_OK);
        void *const block = b.p;
        g_limit = 1000;                                            // refused by the limit: the old block is not even touched
        CHECK(b.reserve(2000) == RT_ERR_OOM && b.p == block && b.bytes == 100 && g_live.count(block));
        CHECK(b.reserve(1000) == RT_OK && b.bytes == 1000);        // at the limit is allowed
        g_limit = ~(size_t)0;
    }
    CHECK(g_live.empty());
}

static void out_of_memory_then_retry()
{
    {
        DevBuf b;
        CHECK(b.reserve(100) == RT_OK);
        void *const old = b.p;
        g_fail_next = 1;                                           // old + new do not fit together: the old block goes, the second try succeeds
        CHECK(b.reserve(200) == RT_OK && b.bytes == 200 && b.p && !g_live.count(old) && g_live.count(b.p) && g_live.size() == 1);
        void *const second = b.p;
        g_fail_next = 2;                                           // ... and when that fails too: an EMPTY buffer, never a stale pointer
        CHECK(b.reserve(400) == RT_ERR_OOM && b.p == nullptr && b.bytes == 0 && !g_live.count(second) && g_live.empty());
        CHECK(b.reserve(50) == RT_OK && b.bytes == 50);            // and it is usable again
        DevBuf fresh;
        g_fail_next = 1;                                           // nothing to give up: one try, empty as before
        CHECK(fresh.reserve(8) == RT_ERR_OOM && fresh.p == nullptr && fresh.bytes == 0 && g_fail_next == 0);
    }
    CHECK(g_live.empty());
}

static void the_alloc_limit_is_honoured()
{
    g_limit = 4096;
    {
        DevBuf b;
        const int before = (int)g_live.size();
        CHECK(b.reserve(4097) == RT_ERR_OOM && b.p == nullptr && (int)g_live.size() == before);
        CHECK(b.reserve(4096) == RT_OK);
    }
    g_limit = ~(size_t)0;
    CHECK(g_live.empty());
}

struct Slices { char *a; double *b; uint32_t *c; char *none; uint64_t *d; };
static void carve(Carver &c, size_t n, Slices &s)
{
    s.a = c.take<char>(1);
    s.b = c.take<double>(n);
    s.c = c.take<uint32_t>(2 * n - 1);
    s.none = c.take<char>(0);
    s.d = c.take<uint64_t>(64);
}
static void carver_slices()
{
    for (size_t n : {(size_t)1, (size_t)31, (size_t)32, (size_t)33, (size_t)1000}) {
        Carver sizing(nullptr);
        Slices none;
        carve(sizing, n, none);
        CHECK(none.a == nullptr && none.b == nullptr && none.d == nullptr);
        void *raw = aligned_alloc(256, sizing.offset);
        Carver c(raw);
        Slices s;
        carve(c, n, s);
        CHECK(c.offset == sizing.offset);                          // the null-base run adds up exactly what the real one takes
        const std::pair<char *, size_t> got[] = {{s.a, 1}, {(char *)s.b, 8 * n}, {(char *)s.c, 4 * (2 * n - 1)}, {(char *)s.d, 8 * 64}};
        char *end = (char *)raw;
        for (const auto &g : got) {
            CHECK(((uintptr_t)g.first & 255u) == 0);               // aligned
            CHECK(g.first >= end);                                 // disjoint, in order
            end = g.first + g.second;
            for (size_t k = 0; k < g.second; k++) g.first[k] = (char)k;      // and inside the allocation (ASan)
        }
        CHECK(end <= (char *)raw + c.offset);
        CHECK(s.none == (char *)s.d);                              // an empty slice takes no room
        free(raw);
    }
}

static void readback_creation_is_all_or_nothing()
{
    {
        PinnedReadback r;
        g_fail_event = 1;                                          // the block is there, the event is refused: the block goes back
        CHECK(!r.ready() && r.block == nullptr && r.event == nullptr && g_host.empty() && g_events.empty() && g_host_frees == 1);
        g_fail_host = 1;
        CHECK(!r.ready() && r.block == nullptr && g_host.empty() && g_events.empty() && g_fail_event == 0);
        uint32_t word = 7;
        g_fail_host = 1;                                           // send() creates as well, and a refusal leaves nothing in flight
        CHECK(!r.send(&word, 4, nullptr) && !r.in_flight && g_host.empty() && g_events.empty());
        CHECK(r.ready() && r.block && r.event && g_host.size() == 1 && g_events.size() == 1);      // a later call tries again
        void *const block = r.block;
        CHECK(r.ready() && r.block == block && g_host.size() == 1 && g_events.size() == 1);        // and only once
    }
    CHECK(g_host.empty() && g_events.empty() && g_host_frees == 2 && g_event_destroys == 1);
}

static void readback_send_and_landed()
{
    PinnedReadback r;
    uint32_t word = 0x12345678u;
    CHECK(!r.landed());                                            // nothing made, nothing sent: no query of a null event
    g_fail_copy = 1;
    CHECK(!r.send(&word, 4, nullptr) && !r.in_flight && g_fail_copy == 0);
    g_fail_record = 1;
    CHECK(!r.send(&word, 4, nullptr) && !r.in_flight && g_fail_record == 0);
    g_event_complete = true;
    CHECK(!r.landed());                                            // ... whatever the event says
    g_copy.dst = nullptr;
    CHECK(r.send(&word, 4, nullptr) && r.in_flight);
    CHECK(!r.landed() && !r.landed() && r.in_flight);              // not ready: false, as often as it is asked
    g_event_complete = true;
    CHECK(r.landed() && !r.in_flight && r.read<uint32_t>() == 0x12345678u);
    CHECK(!r.landed() && !r.landed());                             // true once per flight
    float f = 2.5f;
    CHECK(r.send(&f, 4, nullptr) && !r.landed());
    r.in_flight = false;                                           // a flight nobody asks about any more
    g_event_complete = true;
    CHECK(!r.in_flight && !r.landed());
    CHECK(!r.send(&word, 65, nullptr) && !r.in_flight);            // the block holds 64 bytes
}

static void readback_moves_and_frees_once()
{
    const int frees = g_host_frees, destroys = g_event_destroys;
    {
        PinnedReadback a;
        uint32_t word = 3;
        CHECK(a.send(&word, 4, nullptr));
        void *const block = a.block;
        const hipEvent_t event = a.event;
        PinnedReadback b(std::move(a));
        CHECK(a.block == nullptr && a.event == nullptr && !a.in_flight);
        CHECK(b.block == block && b.event == event && b.in_flight && g_host.size() == 1 && g_events.size() == 1);
        PinnedReadback c;
        CHECK(c.ready() && g_host.size() == 2);
        c = std::move(b);                                          // move-assignment lets go of what it had
        CHECK(g_host_frees == frees + 1 && g_event_destroys == destroys + 1 && c.block == block && c.in_flight && b.block == nullptr);
        PinnedReadback &same = c;
        c = std::move(same);
        CHECK(c.block == block && g_host.size() == 1);
        g_event_complete = true;
        CHECK(!a.landed() && !b.landed() && c.landed() && c.read<uint32_t>() == 3);
    }
    CHECK(g_host.empty() && g_events.empty() && g_host_frees == frees + 2 && g_event_destroys == destroys + 2);
}

static void readback_dies_with_a_copy_in_flight()
{
    const int frees = g_host_frees;
    {
        PinnedReadback r;
        uint32_t word = 9;
        CHECK(r.send(&word, 4, nullptr) && !r.landed() && r.in_flight);
        ASAN_POISON_MEMORY_REGION(r.block, 64);                    // a destructor that reads or writes the block is a sanitizer report
    }
    CHECK(g_host.empty() && g_events.empty() && g_host_frees == frees + 1);
}

int main()
{
    scope_exit_frees();
    move_leaves_the_source_empty();
    move_assignment_frees_the_old_block();
    an_adopted_slice_is_never_freed();
    a_failed_growth_keeps_the_buffer();
    out_of_memory_then_retry();
    the_alloc_limit_is_honoured();
    carver_slices();
    readback_creation_is_all_or_nothing();
    readback_send_and_landed();
    readback_moves_and_frees_once();
    readback_dies_with_a_copy_in_flight();
    const size_t live = g_live.size() + g_host.size() + g_events.size();
    CHECK(live == 0);
    printf("%d failures, %zu live allocations\n", g_failures, live);
    return g_failures == 0 && live == 0 ? 0 : 1;
}
