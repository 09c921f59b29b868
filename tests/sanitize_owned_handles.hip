// Stand-alone host program for AddressSanitizer / UndefinedBehaviorSanitizer over the owner of the library's HIP handles (csrc/pt_owned.h:
// Owned, which Stream, Event and HostBuf instantiate): host code only, no device, nothing loaded into an interpreter.
// tests/run_owned_handles_sanitizer.sh compiles it with -fsanitize=address,undefined and runs it.
// The template is instantiated over a plain integer handle -- and, for the form with arguments behind the handle that HostBuf takes, over
// a heap array -- with create and destroy functions that keep books: every handle made is destroyed exactly once, none twice, and the null
// handle never.  The cases are the ways the library treats its owners: move construction and move assignment, self-move-assignment,
// release and double release, a create over a held handle, a create that fails, two vectors of owners that grow, hand their elements to
// each other and shrink (the timing events' pool: State::evBounce / evFree), and an aggregate with array and vector members assigned from a
// default-constructed one (free_renderer's R() = State()).  Exit status 0 and "sanitizer run finished" when the books balance.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "../include/pt_amd.h"

#define PT_TEST_API 1      // (the owners' own count, as the test library carries it)

namespace {
std::string g_err;
int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
#define HIPCHECK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return fail(PT_ERR_HIP, "HIP error: %s: %d", #expr, (int)e_); } while (0)
#define PTCHECK(expr) do { int rc_ = (expr); if (rc_) return rc_; } while (0)
#include "../project3-cuda-path-tracer_amd/csrc/pt_owned.h"

int g_bad = 0, g_checks = 0;
void expect(bool ok, const char *what) {
    ++g_checks;
    if (!ok) { fprintf(stderr, "unexpected: %s\n", what); ++g_bad; }
}

// the books: handles 1, 2, ... as they are made; `live` holds those not yet destroyed
int g_next = 0, g_made = 0, g_destroyed = 0;
std::set<int> g_live;
constexpr unsigned kRefuse = 99;      // the flags `make` answers an error to, touching nothing
hipError_t make(int *h, unsigned flags) {
    if (flags == kRefuse) return hipErrorOutOfMemory;
    *h = ++g_next;
    g_live.insert(*h);
    ++g_made;
    return hipSuccess;
}
hipError_t unmake(int h) {
    expect(h != 0, "the null handle is never destroyed");
    expect(g_live.erase(h) == 1, "a handle is destroyed once, and only one that was made");
    ++g_destroyed;
    return hipSuccess;
}
constexpr char kMake[] = "make", kMakeArray[] = "make_array";
using Handle = Owned<int, make, unmake, kMake>;

// ... and the form HostBuf takes: a pointer for a handle, arguments behind it (the leak check is the sanitizer's)
int g_arrays = 0;
hipError_t make_array(int **p, size_t n, unsigned) { *p = new int[n](); ++g_arrays; return hipSuccess; }
hipError_t unmake_array(void *p) { delete[] static_cast<int *>(p); --g_arrays; return hipSuccess; }
struct Array : Owned<int *, make_array, unmake_array, kMakeArray> {
    int alloc(size_t n, unsigned flags) { return this->create(n, flags); }
};

// free_renderer's shape: array members, vectors, owners beside plain data
struct Slotlike { Handle stream; int parity = 0; Handle evDone, evCommitted; };
struct Statelike {
    bool init = false;
    Slotlike slot[4];
    Array noiseHost;
    Handle noiseEv[2];
    std::vector<Handle> evBounce, evFree;
    Array hostFault;
    Handle camStream;
};

bool balanced() { return g_live.empty() && g_made == g_destroyed && g_liveHandles.load() == 0 && g_arrays == 0; }
}  // namespace

int main() {
    {   // empty owners: nothing to destroy, however they go
        Handle a, b;
        Handle c(std::move(a));
        b = std::move(c);
        b.release();
        expect(!a && !b && !c, "empty owners stay empty");
    }
    expect(g_made == 0 && g_destroyed == 0, "no call for an empty owner");
    {   // move construction and move assignment
        Handle a;
        expect(a.create(0u) == PT_OK && a == 1 && g_liveHandles.load() == 1, "create");
        Handle b(std::move(a));
        expect(!a && b == 1 && g_destroyed == 0, "move construction hands the handle over");
        Handle c;
        expect(c.create(0u) == PT_OK && c == 2, "a second handle");
        c = std::move(b);
        expect(!b && c == 1 && g_destroyed == 1 && !g_live.count(2), "move assignment lets the held handle go, once");
        Handle &self = c;
        c = std::move(self);
        expect(c == 1 && g_destroyed == 1, "self-move-assignment keeps the handle");
        // release and double release
        c.release();
        expect(!c && g_destroyed == 2, "release");
        c.release();
        expect(!c && g_destroyed == 2, "double release");
        // create over a held handle, and a create that fails
        expect(c.create(0u) == PT_OK && c == 3 && c.create(0u) == PT_OK && c == 4 && g_destroyed == 3, "create over a held handle lets it go first");
        Handle d;
        expect(d.create(kRefuse) == PT_ERR_HIP && !d && g_liveHandles.load() == 1, "a create that fails leaves the owner empty and uncounted");
        expect(c.create(kRefuse) == PT_ERR_HIP && !c && g_destroyed == 4, "... and a held handle released");
    }
    expect(balanced(), "balanced after the moves");
    {   // the timing events' pool: pairs pushed onto one vector as launches are timed, moved to the other when resolved, taken back from it
        std::vector<Handle> bounce, pool;
        for (int round = 0; round < 5; ++round) {
            for (int launch = 0; launch < 300; ++launch) {
                Handle e0, e1;
                for (Handle *e : {&e0, &e1}) {
                    if (!pool.empty()) { *e = std::move(pool.back()); pool.pop_back(); }
                    else expect(e->create(0u) == PT_OK, "a pool event");
                }
                bounce.push_back(std::move(e0));
                bounce.push_back(std::move(e1));
            }
            expect(bounce.size() == 600 && std::all_of(bounce.begin(), bounce.end(), [](const Handle &e) { return e != 0; }), "every timed launch holds its pair");
            if (round == 2) bounce.resize(100);      // (a shrink that destroys)
            for (Handle &e : bounce) pool.push_back(std::move(e));
            bounce.clear();
            bounce.shrink_to_fit();
        }
        expect(g_destroyed == g_made - (int)pool.size(), "growing, shrinking and handing over destroy nothing but what the resize cut off");
        expect((long long)pool.size() == g_liveHandles.load(), "the owners' count is the pool's size");
    }
    expect(balanced(), "balanced after the vectors");
    {   // R() = State(): array members and vectors assigned from a default-constructed aggregate
        Statelike s;
        s.init = true;
        for (Slotlike &sl : s.slot) {
            expect(sl.stream.create(0u) == PT_OK && sl.evDone.create(0u) == PT_OK && sl.evCommitted.create(0u) == PT_OK, "a slot's handles");
            sl.parity = 1;
        }
        expect(s.noiseHost.alloc(4, 0u) == PT_OK && s.hostFault.alloc(1, 0u) == PT_OK && s.noiseEv[1].create(0u) == PT_OK, "the lazily made ones, one left empty");
        s.noiseHost[3] = 7;
        *s.hostFault = 1;
        for (int i = 0; i < 6; ++i) { s.evBounce.emplace_back(); expect(s.evBounce.back().create(0u) == PT_OK, "a pending event"); }
        const int before = g_destroyed;
        s = Statelike();
        expect(g_destroyed - before == 12 + 1 + 6 && g_arrays == 0 && !s.init && !s.slot[3].stream && s.slot[0].parity == 0 && !s.hostFault && s.evBounce.empty(),
               "the assignment released everything, once");
        s = Statelike();      // (an empty one again: nothing to do)
        expect(g_destroyed - before == 19, "nothing is released twice");
    }
    expect(balanced(), "balanced at the end");
    printf("%d handles made, %d destroyed, %d checks, %d with an unexpected answer\n", g_made, g_destroyed, g_checks, g_bad);
    if (g_bad) return 1;
    printf("sanitizer run finished\n");
    return 0;
}
