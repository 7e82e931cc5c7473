// handle_semantics.cpp -- rt_handle (the base of every host object but the context), rt_retain / rt_release, rt_make and the context's own
// count of csrc/rt_internal.h on the host, under AddressSanitizer + UndefinedBehaviorSanitizer (tests/test_handle_semantics.py).  The
// header is the product's own; the few HIP calls behind it are restated here, each writing one line to an event log, and ~rt_context
// (rt_api.hip in the product) is a stand-in that logs.  A toy type that owns two DevBufs then shows the rule the base states once: the
// device is selected (and, for a type that says so, the stream joined) before an object's buffers go, and the context goes after them.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>

#include <set>
#include <string>
#include <vector>

#include "../../dxrexperiments_amd/csrc/rt_internal.h"

static std::vector<std::string> g_log;
static std::set<void *> g_live;          // blocks handed out and not freed yet
static int g_allow = -1;                 // so many more hipMalloc calls succeed, then the device is full (-1: always)
static size_t g_limit = ~(size_t)0;
static int g_failures = 0;

extern "C" hipError_t hipSetDevice(int device) { g_log.push_back("select " + std::to_string(device)); return hipSuccess; }
extern "C" hipError_t hipStreamSynchronize(hipStream_t) { g_log.push_back("join"); return hipSuccess; }
extern "C" hipError_t hipMalloc(void **ptr, size_t size)
{
    if (g_allow == 0) { *ptr = nullptr; g_log.push_back("refused"); return hipErrorOutOfMemory; }
    if (g_allow > 0) g_allow--;
    *ptr = malloc(size);
    g_live.insert(*ptr);
    g_log.push_back("malloc");
    return hipSuccess;
}
extern "C" hipError_t hipFree(void *ptr)
{
    if (!ptr) return hipSuccess;
    if (!g_live.erase(ptr)) { fprintf(stderr, "hipFree of a block that is not live: %p\n", ptr); g_failures++; return hipErrorInvalidValue; }
    free(ptr);
    g_log.push_back("free");
    return hipSuccess;
}
extern "C" hipError_t hipGetLastError(void) { return hipSuccess; }
extern "C" const char *hipGetErrorString(hipError_t e) { return e == hipErrorOutOfMemory ? "out of memory" : "error"; }
void rt_set_error(const char *, ...) {}
size_t &rt_alloc_limit_ref() { return g_limit; }
rt_context::~rt_context() { g_log.push_back("context gone"); }

#define CHECK(cond)                                                             \
    do {                                                                        \
        if (!(cond)) { fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); g_failures++; } \
    } while (0)

typedef std::vector<std::string> Log;

template <bool JOINS> struct Toy : rt_handle {
    using rt_handle::rt_handle;
    static constexpr bool joins_stream = JOINS;
    DevBuf a, b;
};

// a *_create as the library writes them: one way out between the object's creation and *out
template <class T> static int toy_create(rt_context *ctx, T **out)
{
    rt_made<T> x;
    RT_TRY(rt_make(ctx, x));
    RT_TRY(x->a.reserve(100));
    RT_TRY(x->b.reserve(200));
    *out = x.release();
    return RT_OK;
}

static rt_context *context_on(int device)
{
    rt_context *ctx = new rt_context();
    ctx->device = device;
    return ctx;
}

template <bool JOINS> static void destroy_order()
{
    rt_context *ctx = context_on(3);
    Toy<JOINS> *t = nullptr;
    CHECK(toy_create(ctx, &t) == RT_OK && t && t->ctx == ctx && t->refs == 1 && ctx->refs == 2 && g_live.size() == 2);
    g_log.clear();
    rt_context_release(ctx);                                       // the context's own handle goes first: the object keeps it alive
    CHECK(g_log.empty() && ctx->refs == 1);
    CHECK(rt_release(t) == RT_OK);
    CHECK(g_log == (JOINS ? Log{"select 3", "join", "free", "free", "context gone"} : Log{"select 3", "free", "free", "context gone"}));
    CHECK(g_live.empty());
}

static void last_reference()
{
    rt_context *ctx = context_on(0);
    Toy<true> *t = nullptr;
    CHECK(toy_create(ctx, &t) == RT_OK);
    rt_retain(t);
    rt_retain(t);
    CHECK(t->refs == 3 && ctx->refs == 2);                         // the object holds the context once, however often it is held itself
    g_log.clear();
    CHECK(rt_release(t) == RT_OK && rt_release(t) == RT_OK);
    CHECK(g_log.empty() && g_live.size() == 2 && t->refs == 1);
    CHECK(rt_release(t) == RT_OK);                                 // exactly the third
    CHECK(g_log == (Log{"select 0", "join", "free", "free"}) && g_live.empty() && ctx->refs == 1);
    g_log.clear();
    CHECK(rt_release((Toy<true> *)nullptr) == RT_OK && rt_release((Toy<false> *)nullptr) == RT_OK);
    rt_context_release(nullptr);
    CHECK(g_log.empty());
    rt_context_release(ctx);
    CHECK(g_log == Log{"context gone"});
}

template <bool JOINS> static void failed_creation()
{
    rt_context *ctx = context_on(1);
    alignas(Toy<JOINS>) static char somewhere[sizeof(Toy<JOINS>)];
    Toy<JOINS> *const untouched = (Toy<JOINS> *)somewhere, *out = untouched;
    const int before = ctx->refs;
    g_allow = 1;                                                   // the second buffer is refused: the object exists, and holds the first
    g_log.clear();
    CHECK(toy_create(ctx, &out) == RT_ERR_OOM);
    g_allow = -1;
    CHECK(ctx->refs == before && g_live.empty() && out == untouched);
    CHECK(g_log == (JOINS ? Log{"malloc", "refused", "select 1", "join", "free"} : Log{"malloc", "refused", "select 1", "free"}));
    g_log.clear();
    rt_context_release(ctx);
    CHECK(g_log == Log{"context gone"});
}

// two objects on one context whose handle goes first: the context dies with the second of them, whichever that is
static void last_object_standing(bool a_first)
{
    rt_context *ctx = context_on(2);
    Toy<true> *a = nullptr;
    Toy<false> *b = nullptr;
    CHECK(toy_create(ctx, &a) == RT_OK && toy_create(ctx, &b) == RT_OK && ctx->refs == 3);
    rt_context_release(ctx);
    g_log.clear();
    CHECK((a_first ? rt_release(a) : rt_release(b)) == RT_OK);
    CHECK(g_log == (a_first ? Log{"select 2", "join", "free", "free"} : Log{"select 2", "free", "free"}) && ctx->refs == 1 && g_live.size() == 2);
    g_log.clear();
    CHECK((a_first ? rt_release(b) : rt_release(a)) == RT_OK);
    CHECK(g_log == (a_first ? Log{"select 2", "free", "free", "context gone"} : Log{"select 2", "join", "free", "free", "context gone"}));
    CHECK(g_live.empty());
}

int main()
{
    destroy_order<true>();
    destroy_order<false>();
    last_reference();
    failed_creation<true>();
    failed_creation<false>();
    last_object_standing(true);
    last_object_standing(false);
    const size_t live = g_live.size();
    CHECK(live == 0);
    printf("%d failures, %zu live allocations\n", g_failures, live);
    return g_failures == 0 && live == 0 ? 0 : 1;
}
