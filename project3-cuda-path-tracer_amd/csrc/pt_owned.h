// pt_owned.h -- the owners of what the library holds on the device side: DevBuf (device memory), Stream and Event (HIP handles), HostBuf
// (page-locked host memory).  Whatever a renderer (State, Slot, History), a group (PtGroup, GroupDevice), the scan library's workspaces or a
// temporary of pt_api.hip holds is held by one of them, so "what does the library hold" is answered by the types: no teardown list names a
// handle.  Each is move-only and empty by default, and an empty owner -- never filled, released, or moved from -- makes no HIP call in its
// destructor.  Borrowed handles (the caller's stream, accumulator and pinned buffer, a group's snapshot and event inside a member) stay raw.
//
// THE RULE FOR PROCESS EXIT.  Objects in static storage -- the default context, the scan workspaces, thread-local state -- are destroyed
// AFTER the HIP runtime's own exit handlers, when no HIP call may be made any more.  An owner is safe there only because exit_handler()
// (pt_api.hip), registered behind the library's first HIP call and so run before the runtime's handlers, has emptied everything first.  So
// every code path that can fill an owner has called register_exit_handler() before (pt_init's device half, both scan entry points,
// group_build), or its owner is not in static storage (a call's temporaries; a group and its contexts, on the heap).  State::pinnedHost is a
// raw pointer for exactly this reason: pt_pin_host may run before any of those.  No HIP call in a static destructor, no leak-on-exit flag.
//
// Included by pt_api.hip inside its anonymous namespace, behind fail(), HIPCHECK and PTCHECK.
#pragma once

#ifdef PT_TEST_API      // what the owners hold right now (pt_test_live_device_buffers, pt_test_live_handles); the product carries no counter
std::atomic<long long> g_liveDevBufs{0}, g_liveHandles{0};
inline void count_devbuf(int d) { g_liveDevBufs += d; }
inline void count_handle(int d) { g_liveHandles += d; }
#else
inline void count_devbuf(int) {}
inline void count_handle(int) {}
#endif

// The owner of one device allocation: every table of a renderer and every temporary of pt_api.hip.
template <typename T>
struct DevBuf {
    T *p = nullptr;
    size_t cap = 0;                 // elements allocated (the camera move refreshes a table in place where it fits)
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept { if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; } return *this; }
    ~DevBuf() { release(); }
    void release() {
        if (!p) return;
        (void)hipFree(p);
        p = nullptr;
        cap = 0;
        count_devbuf(-1);
    }
    // n elements (at least one: a kernel may be handed the pointer of an empty table), uninitialised / zeroed / copied from the host
    // (`slack`: elements behind the copied ones, left uninitialised)
    int alloc(size_t n) {
        release();
        HIPCHECK(hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(T)));
        cap = std::max<size_t>(n, 1);
        count_devbuf(1);
        return PT_OK;
    }
    int alloc_zeroed(size_t n) {
        PTCHECK(alloc(n));
        HIPCHECK(hipMemset(p, 0, std::max<size_t>(n, 1) * sizeof(T)));
        return PT_OK;
    }
    int upload(const T *src, size_t n, size_t slack = 0) {
        PTCHECK(alloc(n + slack));
        if (n) HIPCHECK(hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice));
        return PT_OK;
    }
    int upload(const std::vector<T> &v) { return upload(v.data(), v.size()); }
};

// The owner of one handle H that Create(&h, ...) -- the HIP call What names in a failure's message -- makes and Destroy(h) lets go.  It converts
// to the handle, so a HIP call takes the owner where it took the handle; an empty one is the null handle (for a stream: the NULL stream).
constexpr char kStreamCreate[] = "hipStreamCreateWithFlags", kEventCreate[] = "hipEventCreateWithFlags", kHostAlloc[] = "hipHostMalloc";
template <class H, auto Create, auto Destroy, const char *What>
struct Owned {
    H h{};
    Owned() = default;
    Owned(const Owned &) = delete;
    Owned &operator=(const Owned &) = delete;
    Owned(Owned &&o) noexcept : h(o.h) { o.h = H{}; }
    Owned &operator=(Owned &&o) noexcept { if (this != &o) { release(); h = o.h; o.h = H{}; } return *this; }
    ~Owned() { release(); }
    operator H() const { return h; }
    void release() {
        if (!h) return;
        (void)Destroy(h);
        h = H{};
        count_handle(-1);
    }
    template <class... A>
    int create(A... a) {            // (the arguments of Create behind the handle: a stream's or an event's flags)
        release();
        if (const hipError_t e = Create(&h, a...)) return fail(PT_ERR_HIP, "HIP error (%s:%d): %s: %s", "pt_owned.h", __LINE__, What, hipGetErrorString(e));
        count_handle(1);
        return PT_OK;
    }
};
using Stream = Owned<hipStream_t, hipStreamCreateWithFlags, hipStreamDestroy, kStreamCreate>;
using Event = Owned<hipEvent_t, hipEventCreateWithFlags, hipEventDestroy, kEventCreate>;      // (hipEventDefault: what hipEventCreate makes)

template <typename T>      // ... and of n elements of page-locked host memory (hipHostMalloc's flags)
inline hipError_t host_alloc(T **p, size_t n, unsigned flags) { return hipHostMalloc((void **)p, n * sizeof(T), flags); }
template <typename T>
struct HostBuf : Owned<T *, host_alloc<T>, hipHostFree, kHostAlloc> {
    int alloc(size_t n, unsigned flags) { return this->create(n, flags); }
};
