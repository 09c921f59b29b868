// pt_group.h -- renderer contexts and device groups of the C ABI (include/pt_amd.h: pt_ctx_*, pt_group_*).
//
// A CONTEXT is one renderer instance (State): the C ABI's functions act on the calling thread's current one.  A GROUP is N contexts that
// render the row shards y % N of ONE frame -- one context per device of a node (the north star's tile-sharded 8 x MI355X), or
// several on one device -- behind one call each: the native multi-device host path the reference's own C++ host can sit on
// (host/pathtrace_shim.cpp honours PT_AMD_DEVICES; the reference is hard-wired to device 0, src/preview.cpp:107, src/pathtrace.cu:70-71).
// Pixels are independent and seeded by their GLOBAL index, so the shards' rows, put together, are the one-device frame bit for bit.
//
// Round 6 -- how a group is laid out and driven:
//   * ONE zero-padded full-frame accumulator per DISTINCT device (GroupDevice::full).  The members on a device commit their own rows in
//     place into it (k_commit indexes by the global pixel; rows are disjoint), so members that share a device need no collective at all.
//   * ONE issuing THREAD per member (Worker): a member's launches are enqueued by its own host thread, so eight devices are fed side by
//     side instead of one after the other (a C2 shard of 1/8 is ~0.24 ms of GPU time per batch of 64 -- less than one thread needs to
//     enqueue eight members' launches).  PT_AMD_GROUP_THREADS=0: the calling thread issues everything (experiments).
//   * The frame is ASSEMBLED asynchronously (assemble(); pt_group_iterate / pt_group_reduce / the first pt_group_readback after a batch):
//       "rccl reduce"         distinct devices, librccl.so loaded (dlopen; single process, ncclCommInitAll): every member's commit
//                             ALSO writes its rows' new values into one of two SNAPSHOT frames of its device (k_commit's `snap`: the
//                             accumulator is read once, for the addition and the copy), then ONE ncclReduce(sum, float32, 3 W H, root =
//                             member 0's device) of the snapshots on the device's collective stream behind the members' commit events --
//                             x + 0 is exact: disjoint rows.  Across devices the root receives into a RESULT frame of its own
//                             (PtGroup::reduced); a one-rank communicator, where the reduce is the identity, reduces the snapshot onto
//                             itself.  Nothing waits on the host: the reduce of iteration i runs while iteration i + 1 is committed
//                             into the OTHER snapshot and the batches traced ahead keep tracing; a snapshot is written again two calls
//                             later, behind its reduce's event.  pt_group_readback = one D2H copy of the latest assembled frame on the
//                             root's collective stream + a wait for THAT stream only.
//       "shared accumulator"  every member on ONE device: the accumulator is the frame; readback copies it behind the members' commit events.
//       "host gather"         several devices without RCCL (PT_AMD_COLLECTIVE=host, no librccl.so): every device's frame is copied to the host
//                             and the rows are taken from their owners' (synchronous; a fallback).
//   * ncclGroupStart / ncclGroupEnd are balanced on EVERY path: the loop between them records the first error and goes on to GroupEnd.
// Across DISTINCT devices the RCCL leg is UNMEASURED: no multi-GPU node was available to any build round (pt_group_collective() says so);
// what has run is the same pipeline in a one-rank communicator (PT_AMD_COLLECTIVE=rccl), bit-identical after every call, and -- in the test
// library only -- the multi-device PROTOCOL on VIRTUAL devices: pt_test_group_create_virtual (include/pt_amd_test.h) gives every member a
// virtual device index, each distinct index a GroupDevice of its own on the one HIP device (its own accumulator, snapshots, collective stream,
// events), and an emulated reduce with ncclReduce's semantics (EmulatedReduce below) or the host gather in RCCL's place.  Everything after
// group_build is the product's code.  That proves the snapshot / event protocol, not RCCL or the links between devices.
//
// The stale-row bug the virtual devices found (tests/test_gpu_group_devices.py).  Until then the root reduced IN PLACE: the sum landed in the
// root's own snapshot k.  A commit writes only its member's rows into a snapshot, so the other devices' rows of the root's snapshot -- zero
// before the first reduce, which is all "x + 0" needs -- held the frame of that reduce ever after: the third assembly (snapshot 0 again) summed
// {A3 | B1 stale} and {0 | B3} to {A3 | B1 + B3}.  A one-rank communicator never shows it (the root's members write every row there is).  The
// fix: with two or more GroupDevices the root receives into PtGroup::reduced, which no commit writes, and every snapshot keeps zeros in the
// rows its device does not own.
// Included by pt_api.hip inside its extern "C" block.
#pragma once
#include <dlfcn.h>      // (the C++ headers this file needs -- <atomic>, <condition_variable>, <functional>, <thread> -- are included by pt_api.hip)

struct PtContext {
    State st;                       // (first: pt_ctx_current hands &st out as the context)
    std::atomic<int> users{0};      // threads this context is current on (pt_ctx_make_current)
};

namespace {
// the context pt_ctx_make_current bound to this thread: released when the thread rebinds or ends, so that pt_ctx_destroy can tell
// whether ANOTHER thread still acts on the context (its t_ctx would dangle)
struct CurrentRef {
    PtContext *held = nullptr;
    ~CurrentRef() {
        if (held) held->users.fetch_sub(1);
    }
};
thread_local CurrentRef t_ref;
}  // namespace

PtContext *pt_ctx_create(void) {
    PtContext *c = new (std::nothrow) PtContext();
    if (!c) { fail(PT_ERR_INVALID, "pt_ctx_create: out of memory"); return nullptr; }
    std::lock_guard<std::mutex> lock(g_ctxMutex);
    g_contexts.push_back(&c->st);
    return c;
}
PtContext *pt_ctx_current(void) { return t_ctx == &g_default ? nullptr : reinterpret_cast<PtContext *>(t_ctx); }
int pt_ctx_make_current(PtContext *ctx) {
    {
        std::lock_guard<std::mutex> lock(g_ctxMutex);
        if (ctx && std::find(g_contexts.begin(), g_contexts.end(), &ctx->st) == g_contexts.end()) return fail(PT_ERR_INVALID, "pt_ctx_make_current: not a live context");
        if (t_ref.held != ctx) {
            if (t_ref.held) t_ref.held->users.fetch_sub(1);
            t_ref.held = ctx;
            if (ctx) ctx->users.fetch_add(1);
        }
    }
    t_ctx = ctx ? &ctx->st : &g_default;
    // an initialised renderer lives on ONE device: its calls allocate, launch and copy there
    if (R().init || R().nslots > 0) HIPCHECK(hipSetDevice(R().device));
    return PT_OK;
}
int pt_ctx_destroy(PtContext *ctx) {
    if (!ctx) return PT_OK;
    {
        std::lock_guard<std::mutex> lock(g_ctxMutex);
        auto it = std::find(g_contexts.begin(), g_contexts.end(), &ctx->st);
        if (it == g_contexts.end()) return fail(PT_ERR_INVALID, "pt_ctx_destroy: not a live context");
        // current on ANOTHER thread: that thread's next pt_* call would act on freed memory
        if (ctx->users.load() > (t_ref.held == ctx ? 1 : 0))
            return fail(PT_ERR_INVALID, "pt_ctx_destroy: the context is current on another thread (pt_ctx_make_current(NULL) there first)");
        g_contexts.erase(it);
        if (t_ref.held == ctx) { t_ref.held = nullptr; ctx->users.fetch_sub(1); }
    }
    int dev = -1;
    (void)hipGetDevice(&dev);
    State *const prev = t_ctx;
    t_ctx = &ctx->st;
    free_renderer();
    t_ctx = prev == &ctx->st ? &g_default : prev;
    if (dev >= 0) (void)hipSetDevice(dev);          // (free_renderer switched to the renderer's device)
    delete ctx;
    return PT_OK;
}

// ---- groups ---------------------------------------------------------------------------------------------------------------------------
namespace {
// the collective's function table: librccl.so's entry points -- or, for the test library's virtual devices, the emulation's (EmulatedReduce).
// A group calls its collective through PtGroup::api only.
struct Rccl {
    void *lib = nullptr;
    int (*CommInitAll)(void **, int, const int *) = nullptr;
    int (*CommDestroy)(void *) = nullptr;
    int (*Reduce)(const void *, void *, size_t, int, int, int, void *, hipStream_t) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
    bool load() {
        if (lib) return true;
        for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"})
            if ((lib = dlopen(name, RTLD_NOW | RTLD_LOCAL))) break;
        if (!lib) return false;
        CommInitAll = (decltype(CommInitAll))dlsym(lib, "ncclCommInitAll");
        CommDestroy = (decltype(CommDestroy))dlsym(lib, "ncclCommDestroy");
        Reduce = (decltype(Reduce))dlsym(lib, "ncclReduce");
        GroupStart = (decltype(GroupStart))dlsym(lib, "ncclGroupStart");
        GroupEnd = (decltype(GroupEnd))dlsym(lib, "ncclGroupEnd");
        GetErrorString = (decltype(GetErrorString))dlsym(lib, "ncclGetErrorString");
        if (CommInitAll && CommDestroy && Reduce && GroupStart && GroupEnd && GetErrorString) return true;
        dlclose(lib);
        lib = nullptr;
        return false;
    }
};
Rccl *rcclPtr() {
    static Rccl r;
    return &r;
}
#define rccl() (*rcclPtr())
std::mutex g_rcclMutex;                          // (loading; the calls themselves go through one group's host thread)
constexpr int kNcclFloat = 7, kNcclSum = 0;      // rccl.h: ncclFloat32, ncclSum

#ifdef PT_TEST_API
// ---- the emulated reduce: a second table of the Rccl shape, for the virtual devices of the test library --------------------------------
// Semantics: ncclReduce's in one process.  Between GroupStart and GroupEnd every rank of a communicator posts (sendbuf, recvbuf, count, root,
// comm, stream); at GroupEnd the root's recvbuf[i] = sendbuf_0[i] + sendbuf_1[i] + ... in ASCENDING RANK order, fp32, one IEEE addition each.
// recvbuf may be the root's own sendbuf (in place); the other ranks' recvbuf is ignored.  A NULL communicator answers ncclInvalidArgument and
// posts nothing; GroupEnd closes the group whatever was refused (a group that ends with no post enqueues nothing and succeeds, as RCCL's does).
// A group that ends with posts from only SOME ranks, or with ranks that disagree on count or root, would hang real RCCL; here it is refused
// with ncclInvalidUsage and nothing is enqueued.  float32 and sum only; at most kEmuMaxRanks (8) ranks, every one on the current HIP device.
//
// Stream order -- what makes the call behave on each rank's stream as the real one does.  GroupEnd enqueues everything from the host and
// waits for nothing:
//   1. a "posted" event is recorded on every non-root rank's stream;
//   2. the root's stream waits for all of them;
//   3. ONE kernel (k_emulated_reduce, pt_test_kernels.h) on the root's stream adds the send buffers into the root's recvbuf;
//   4. a "done" event is recorded on the root's stream;
//   5. every non-root rank's stream waits for it.
// So a rank's operation is complete on its stream only when its send buffer has been read -- which is what a group's evRed[k] records and
// what the next commit into snapshot k waits for.  Every wait is for an event recorded EARLIER in the same GroupEnd: the dependencies are
// acyclic in enqueue order, and nothing can wait for work that is not yet enqueued.
struct EmulatedReduce {
    enum { kSuccess = 0, kUnhandledHipError = 1, kInvalidArgument = 4, kInvalidUsage = 5 };      // rccl.h: ncclResult_t
    struct World {                     // what CommInitAll makes: the ranks of one communicator
        int n = 0, live = 0;
        Event posted[kEmuMaxRanks];
        Event done;
    };
    struct Comm { World *w; int rank; };
    struct Post { const float *send; float *recv; size_t count; int root; Comm *comm; hipStream_t stream; };
    struct Calls { int depth = 0; std::vector<Post> posts; };      // the calling thread's open group (RCCL's group state is per thread too)
    static Calls &calls() {
        thread_local Calls c;
        return c;
    }
    static int CommInitAll(void **comms, int n, const int *) {
        if (!comms || n < 1 || n > kEmuMaxRanks) return kInvalidArgument;
        World *w = new World();
        w->n = w->live = n;
        bool ok = w->done.create(hipEventDisableTiming) == PT_OK;
        for (int r = 0; r < n && ok; ++r) ok = w->posted[r].create(hipEventDisableTiming) == PT_OK;
        if (!ok) { delete w; return kUnhandledHipError; }
        for (int r = 0; r < n; ++r) comms[r] = new Comm{w, r};
        return kSuccess;
    }
    static int CommDestroy(void *comm) {
        Comm *c = static_cast<Comm *>(comm);
        if (!c) return kInvalidArgument;
        World *w = c->w;
        delete c;
        if (--w->live == 0) delete w;
        return kSuccess;
    }
    static int GroupStart() {
        ++calls().depth;
        return kSuccess;
    }
    static int Reduce(const void *send, void *recv, size_t count, int dtype, int op, int root, void *comm, hipStream_t stream) {
        if (!comm || !send || dtype != kNcclFloat || op != kNcclSum) return kInvalidArgument;
        const bool alone = calls().depth == 0;        // outside a group: a group of this one call
        if (alone) GroupStart();
        calls().posts.push_back(Post{static_cast<const float *>(send), static_cast<float *>(recv), count, root, static_cast<Comm *>(comm), stream});
        return alone ? GroupEnd() : (int)kSuccess;
    }
    static int GroupEnd() {
        Calls &c = calls();
        if (c.depth <= 0) return kInvalidUsage;
        if (--c.depth > 0) return kSuccess;
        std::vector<Post> posts;
        posts.swap(c.posts);
        if (posts.empty()) return kSuccess;
        // one post per rank of ONE communicator, all of one count and root
        World *w = posts[0].comm->w;
        const int root = posts[0].root;
        const size_t count = posts[0].count;
        if ((int)posts.size() != w->n || root < 0 || root >= w->n) return kInvalidUsage;
        const Post *byRank[kEmuMaxRanks] = {};
        for (const Post &p : posts) {
            if (p.comm->w != w || p.root != root || p.count != count || byRank[p.comm->rank]) return kInvalidUsage;
            byRank[p.comm->rank] = &p;
        }
        const Post &rp = *byRank[root];
        if (!rp.recv) return kInvalidArgument;
        if (count == 0) return kSuccess;
        ptk::EmuSources src{};
        bool aligned = (reinterpret_cast<uintptr_t>(rp.recv) & 15u) == 0;
        for (int r = 0; r < w->n; ++r) {
            src.p[r] = byRank[r]->send;
            aligned = aligned && (reinterpret_cast<uintptr_t>(src.p[r]) & 15u) == 0;
        }
        const long long nvec4 = aligned ? (long long)(count / 4) : 0;
        const long long lanes = nvec4 + ((long long)count - 4 * nvec4);
        bool ok = true;
        for (int r = 0; r < w->n && ok; ++r)
            if (r != root) ok = hipEventRecord(w->posted[r], byRank[r]->stream) == hipSuccess;
        for (int r = 0; r < w->n && ok; ++r)
            if (r != root) ok = hipStreamWaitEvent(rp.stream, w->posted[r], 0) == hipSuccess;
        if (ok) {
            hipLaunchKernelGGL(ptk::k_emulated_reduce, dim3((unsigned)((lanes + kBlock - 1) / kBlock)), dim3(kBlock), 0, rp.stream, src, w->n, rp.recv, nvec4,
                               (long long)count);
            ok = hipGetLastError() == hipSuccess && hipEventRecord(w->done, rp.stream) == hipSuccess;
        }
        for (int r = 0; r < w->n && ok; ++r)
            if (r != root) ok = hipStreamWaitEvent(byRank[r]->stream, w->done, 0) == hipSuccess;
        return ok ? kSuccess : kUnhandledHipError;
    }
    static const char *GetErrorString(int r) {
        switch (r) {
            case kSuccess: return "no error";
            case kUnhandledHipError: return "unhandled HIP error (emulated reduce)";
            case kInvalidArgument: return "invalid argument (emulated reduce)";
            case kInvalidUsage: return "invalid usage (emulated reduce)";
        }
        return "unknown result code (emulated reduce)";
    }
    static const Rccl *table() {
        static const Rccl t = [] {
            Rccl r;
            r.CommInitAll = CommInitAll;
            r.CommDestroy = CommDestroy;
            r.Reduce = Reduce;
            r.GroupStart = GroupStart;
            r.GroupEnd = GroupEnd;
            r.GetErrorString = GetErrorString;
            return r;
        }();
        return &t;
    }
};
#endif  // PT_TEST_API
// the calling thread's current context and device, put back when a group call returns
struct CurrentGuard {
    State *saved = t_ctx;
    int dev = -1;
    CurrentGuard() { (void)hipGetDevice(&dev); }
    ~CurrentGuard() {
        t_ctx = saved;
        if (dev >= 0) (void)hipSetDevice(dev);
    }
};

// One host thread per member: it owns the member's context (t_ctx) and device for its lifetime and enqueues what the group's calls post.
// (Spinning on an atomic word before sleeping on the condition variable was tried for the per-iteration protocol and measured no
// different -- 0.097 ms per pt_group_iterate with 8 members on one device either way: the members' commits, not the wake-ups, bound it.)
struct Worker {
    std::thread th;
    std::mutex m;
    std::condition_variable cv;
    std::function<int()> job;
    bool pending = false, quit = false;
    int rc = PT_OK;
    std::string err;
    void loop(State *st) {
        t_ctx = st;
        for (;;) {
            std::function<int()> f;
            {
                std::unique_lock<std::mutex> lk(m);
                cv.wait(lk, [&] { return pending || quit; });
                if (!pending && quit) return;
                f = job;
            }
            g_err.clear();
            const int r = f();
            {
                std::lock_guard<std::mutex> lk(m);
                rc = r;
                err = g_err;
                pending = false;
            }
            cv.notify_all();
        }
    }
    void post(std::function<int()> f) {
        {
            std::lock_guard<std::mutex> lk(m);
            job = std::move(f);
            pending = true;
        }
        cv.notify_all();
    }
    int wait(std::string *e) {
        std::unique_lock<std::mutex> lk(m);
        cv.wait(lk, [&] { return !pending; });
        if (rc != PT_OK && e) *e = err;
        return rc;
    }
    void stop() {
        {
            std::lock_guard<std::mutex> lk(m);
            quit = true;
        }
        cv.notify_all();
        if (th.joinable()) th.join();
    }
};

// what a group holds per DISTINCT device.  `id` is the device's identity -- what members are grouped by -- and `device` the HIP ordinal its
// buffers, streams and events live on: the same number in a product group, the virtual index and the one real device in a virtual group
// (pt_test_group_create_virtual).  Members of different GroupDevices share nothing below, whatever their HIP ordinals.
struct GroupDevice {
    int id = 0;
    int device = 0;
    std::vector<int> members;              // indices into PtGroup::ctx
    DevBuf<float> full;                    // the zero-padded full-frame accumulator the members on this device commit into
    DevBuf<float> snap[2];                 // rccl: the members' commits copy their rows here (k_commit's `snap`), every other row stays zero; the reduce's send buffer
    Stream coll;                           // the collective's stream (and the read-back's)
    Event evRed[2];                        // the reduce that read snapshot k is through (collective stream)
    void *comm = nullptr;                  // ncclComm_t: the function table's (PtGroup::api), destroyed through it
};
}  // namespace

struct PtGroup {
    std::vector<PtContext *> ctx;
    std::vector<int> device;               // [n] member -> HIP device
    std::vector<int> devIndex;             // [n] member -> index into dev
    std::vector<Stream> stream;            // [n] the member's own "caller's stream": commits, in call order (empty: the NULL stream)
    std::vector<Event> evCommit;           // [n] the member's commits so far (recorded behind every call's enqueue)
    std::vector<std::unique_ptr<Worker>> worker;   // [n] or empty (PT_AMD_GROUP_THREADS=0, one member)
    std::vector<GroupDevice> dev;          // distinct devices, dev[0] = member 0's = the reduce's root
    bool rccl = false;                     // the frame is assembled by ncclReduce (else: shared accumulator / on the host)
    const Rccl *api = nullptr;             // ... through this table: librccl.so's, or the emulated reduce of a virtual group (test library)
    DevBuf<float> reduced;                 // rccl, two or more devices: the frame the root (dev[0]) receives the reduce into.  No commit writes it.  ONE
                                           // buffer: the reduce that writes it and the read-back that copies it are both on dev[0].coll, in call order
    std::vector<char> waitRed;            // [n] rccl: the member's next commit writes a snapshot a reduce may still be reading: wait for evRed first
    int W = 0, H = 0;
    bool inited = false;
    bool dirty = false;                    // commits were enqueued since the frame was last assembled
    int k = 0;                             // the snapshot the NEXT assembly takes
    int last = -1;                         // ... and the one that holds the latest assembled frame
    int failReduces = 0;                   // tests (pt_test_group_fail_next_reduce): the next reduces are issued with a null communicator
    std::vector<float> stage;              // host gather: one device's frame
    std::string how = "shared accumulator";
};

namespace {
// runs f(i) for every member -- on the members' own threads when the group has them, else on the calling thread, member by member --
// and returns the first failure (its message becomes the calling thread's pt_last_error)
int for_members(PtGroup *g, const std::function<int(int)> &f) {
    const int n = (int)g->ctx.size();
    int first = PT_OK;
    if (!g->worker.empty()) {
        for (int i = 0; i < n; ++i) g->worker[i]->post([&f, i] { return f(i); });
        for (int i = 0; i < n; ++i) {
            std::string e;
            const int rc = g->worker[i]->wait(&e);
            if (rc != PT_OK && first == PT_OK) { first = rc; g_err = e; }
        }
        return first;
    }
    for (int i = 0; i < n; ++i) {
        t_ctx = &g->ctx[i]->st;
        (void)hipSetDevice(g->device[i]);
        const int rc = f(i);
        if (rc != PT_OK) return rc;
    }
    return PT_OK;
}

void group_release_buffers(PtGroup *g) {
    for (GroupDevice &d : g->dev) {
        (void)hipSetDevice(d.device);
        if (d.coll) (void)hipStreamSynchronize(d.coll);
        d.full.release();
        for (DevBuf<float> &s : d.snap) s.release();
    }
    if (g->reduced.p) {     // (on the root's device)
        (void)hipSetDevice(g->dev[0].device);
        g->reduced.release();
    }
    g->inited = false;
    g->dirty = false;
    g->last = -1;
}

// Assemble the frame from what the members have committed so far -- asynchronously: nothing here waits on the host.
int assemble(PtGroup *g) {
    const int k = g->k;
    if (!g->rccl) {
        // shared accumulator / host gather: the accumulators ARE the frame's parts, and the collective streams -- which the read-back copies
        // on -- already wait for the members' commits (pt_group_iterate_batch)
        g->dirty = false;
        return PT_OK;
    }
    if (!g->dirty && g->last >= 0) return PT_OK;                 // nothing was committed since the last assembly: its frame stands
    // 1. (per device, the collective stream already waits for the commits that wrote snapshot k: every member's last call wrote its rows
    //    there and queued the wait -- pt_group_iterate_batch)
    // 2. ONE ncclReduce(sum) of the snapshots to dev[0] -- into g->reduced where there are other devices: the root's own snapshot
    //    must keep zeros in their rows for the reduce after next (a commit rewrites its member's rows only); a one-rank reduce is the
    //    identity and stays in place.  No early return between GroupStart and GroupEnd: the first error is kept, the group is always
    //    closed, then the call fails -- an open RCCL group would swallow every later collective of the process.
    const Rccl &rc_ = *g->api;
    int r = rc_.GroupStart(), rHip = 0;
    if (r == 0) {
        for (size_t di = 0; di < g->dev.size(); ++di) {
            GroupDevice &d = g->dev[di];
            if (hipSetDevice(d.device) != hipSuccess) { rHip = 1; continue; }
            void *comm = g->failReduces > 0 ? nullptr : d.comm;
            float *const recv = di != 0 ? nullptr : g->reduced.p ? g->reduced.p : d.snap[k].p;
            const int ri = rc_.Reduce(d.snap[k].p, recv, (size_t)g->W * g->H * 3, kNcclFloat, kNcclSum, 0, comm, d.coll);
            if (ri != 0 && r == 0) r = ri;
        }
        const int r2 = rc_.GroupEnd();
        if (r == 0) r = r2;
    }
    if (g->failReduces > 0) --g->failReduces;
    // (an error leaves the snapshot as the commits wrote it and nothing but waits on the collective streams: the next call tries again)
    if (r != 0 || rHip) return fail(PT_ERR_HIP, "pt_group: ncclReduce failed: %s", rHip ? "hipSetDevice" : rc_.GetErrorString(r));
    for (GroupDevice &d : g->dev) {
        HIPCHECK(hipSetDevice(d.device));
        HIPCHECK(hipEventRecord(d.evRed[k], d.coll));
    }
    g->last = k;
    g->k = k ^ 1;
    g->dirty = false;
    std::fill(g->waitRed.begin(), g->waitRed.end(), 1);      // snapshot k ^ 1 was last read by the reduce before this one
    return PT_OK;
}
}  // namespace

namespace {
// the collective's streams, events and RCCL's communicator: once per group, behind the members' first pt_init (see pt_group_create)
int ensure_collective(PtGroup *g) {
    for (GroupDevice &d : g->dev) {
        HIPCHECK(hipSetDevice(d.device));      // (each member by itself: a call that failed half-way is made up for by the next)
        if (!d.coll) PTCHECK(d.coll.create(hipStreamNonBlocking));
        for (Event &e : d.evRed)
            if (!e) PTCHECK(e.create(hipEventDisableTiming));
    }
    if (g->rccl && !g->dev[0].comm) {
        const int nd = (int)g->dev.size();
        std::vector<void *> comms(nd, nullptr);
        std::vector<int> devs;
        for (const GroupDevice &d : g->dev) devs.push_back(d.device);
        std::lock_guard<std::mutex> lock(g_rcclMutex);
        const int r = g->api->CommInitAll(comms.data(), nd, devs.data());
        if (r != 0) {
            fprintf(stderr, "pt_group_init: ncclCommInitAll failed (%s): the frame is assembled %s\n", g->api->GetErrorString(r), nd > 1 ? "on the host" : "in place");
            g->rccl = false;
            g->how = nd > 1 ? "host gather" : "shared accumulator";
        } else {
            for (int q = 0; q < nd; ++q) g->dev[q].comm = comms[q];
        }
    }
    return PT_OK;
}
}  // namespace

namespace {
// Creating a group, first half: WHERE its members sit.  Member g->device.size() joins the GroupDevice of identity `id` -- a new one, on
// HIP device `hip`, when it is the first member there.  (pt_group_create: id = the HIP ordinal; pt_test_group_create_virtual: id = the
// virtual index, every one on the current HIP device.)
void group_place(PtGroup *g, int id, int hip) {
    const int i = (int)g->device.size();
    g->device.push_back(hip);
    int di = -1;
    for (size_t q = 0; q < g->dev.size(); ++q)
        if (g->dev[q].id == id) di = (int)q;
    if (di < 0) {
        GroupDevice gd;
        gd.id = id;
        gd.device = hip;
        g->dev.push_back(std::move(gd));
        di = (int)g->dev.size() - 1;
    }
    g->dev[di].members.push_back(i);
    g->devIndex.push_back(di);
}

// ... second half: the group from that map -- contexts, commit streams, the collective, the issuing threads.  `emulated` (test library): a
// VIRTUAL group, assembled by that table's reduce (collective 1) or on the host (0); null: the product's choice -- RCCL where there is
// something to reduce and librccl.so loads, PT_AMD_COLLECTIVE permitting.  Takes `g` over: destroyed on failure.
int group_build(PtGroup **out, PtGroup *g, const Rccl *emulated, int collective, const char *fn) {
    register_exit_handler();
    CurrentGuard guard;
    const int n = (int)g->device.size();
    for (int i = 0; i < n; ++i) {
        PtContext *c = pt_ctx_create();
        if (!c) { pt_group_destroy(g); return PT_ERR_INVALID; }
        g->ctx.push_back(c);
    }
    // Streams.  A process gets FOUR hardware queues per device by default (GPU_MAX_HW_QUEUES), handed to streams as they are created; a
    // fifth stream shares a queue with an earlier one, and work that shares a queue runs in queue order whatever the streams say: commits
    // that land behind a tracing stream's bounce launches wait for whole launches (config C3 as written, one member: 0.046 against 0.040 ms
    // per iteration; 0.053 against 0.0445 with the collective -- profiles/r06_group_experiments.txt).  So: a member that has its device to
    // itself commits on that device's NULL stream (the renderer's other streams are non-blocking: nothing synchronises with it implicitly),
    // and everything the collective needs -- its stream, RCCL's communicator with the streams IT creates -- is made AFTER the members'
    // first pt_init has created their tracing streams (ensure_collective, from pt_group_init): null, two tracing streams, collective.
    // Members that share a device (the one-GPU rehearsal) get a commit stream each -- "alone" means alone on the HIP device: the members of a
    // virtual group sit on GroupDevices of their own and on ONE null stream all the same.
    g->stream = std::vector<Stream>(n);
    g->evCommit = std::vector<Event>(n);
    bool ok = true;
    const char *ownStreams = getenv("PT_AMD_GROUP_OWN_STREAMS");      // experiments only
    for (int i = 0; i < n && ok; ++i) {
        const bool alone = std::count(g->device.begin(), g->device.end(), g->device[i]) == 1 && !(ownStreams && atoi(ownStreams));
        ok = hipSetDevice(g->device[i]) == hipSuccess && (alone || g->stream[i].create(hipStreamNonBlocking) == PT_OK) &&
             g->evCommit[i].create(hipEventDisableTiming) == PT_OK;
    }
    if (!ok) {
        pt_group_destroy(g);
        return fail(PT_ERR_HIP, "%s: no stream / event on a member's device", fn);
    }
    // RCCL: one rank per DISTINCT device, one process (ncclCommInitAll).  Members that all share one device need no collective
    // (PT_AMD_COLLECTIVE=rccl sends their frame through a one-rank communicator all the same: the call path on a one-GPU box).
    // The library is loaded here -- pt_group_collective() answers from now on --, the communicator is made by the first pt_group_init.
    // A virtual group takes what its creator named and reads no environment.
    const char *want = emulated ? nullptr : getenv("PT_AMD_COLLECTIVE");
    const bool forbid = want && !strcmp(want, "host");
    const bool force = want && !strcmp(want, "rccl");
    const int nd = (int)g->dev.size();
    if (nd > 1) g->how = "host gather";
    if (emulated) {
        if (collective == 1) {
            g->api = emulated;
            g->rccl = true;
            g->how = "emulated reduce (virtual devices: test library)";
        }
    } else if (!forbid && (nd > 1 || force)) {
        std::lock_guard<std::mutex> lock(g_rcclMutex);
        if (rccl().load()) {
            g->api = &rccl();
            g->rccl = true;
            g->how = nd > 1 ? "rccl reduce (unmeasured across devices: no multi-GPU node was available to the build)" : "rccl reduce (one-rank communicator)";
        }
    }
    // the members' issuing threads
    const char *thr = getenv("PT_AMD_GROUP_THREADS");
    if (n > 1 && !(thr && atoi(thr) == 0)) {
        for (int i = 0; i < n; ++i) {
            g->worker.emplace_back(new Worker());
            Worker *w = g->worker.back().get();
            State *st = &g->ctx[i]->st;
            const int d = g->device[i];
            w->th = std::thread([w, st, d] {
                (void)hipSetDevice(d);
                w->loop(st);
            });
        }
    }
    {
        std::lock_guard<std::mutex> lock(g_groupMutex);      // (a group the host forgets is destroyed by the process's exit handler)
        g_groups.push_back(g);
    }
    *out = g;
    return PT_OK;
}
}  // namespace

int pt_group_create(PtGroup **out, int n, const int32_t *devices) {
    if (!out || n < 1 || n > 64) return fail(PT_ERR_INVALID, "pt_group_create: 1..64 members");
    const int ndev = count_devices();
    if (ndev < 1) return fail(PT_ERR_NO_GPU, "pt_group_create: no HIP device (this library has no CPU fallback)");
    PtGroup *g = new (std::nothrow) PtGroup();
    if (!g) return fail(PT_ERR_INVALID, "pt_group_create: out of memory");
    for (int i = 0; i < n; ++i) {
        const int d = devices ? devices[i] : i % ndev;
        if (d < 0 || d >= ndev) { delete g; return fail(PT_ERR_INVALID, "pt_group_create: device %d of %d", d, ndev); }
        group_place(g, d, d);
    }
    return group_build(out, g, nullptr, -1, "pt_group_create");
}

void pt_group_destroy(PtGroup *g) {
    if (!g) return;
    CurrentGuard guard;
    // the members' renderers first (they synchronise their own streams), on their own threads' behalf; then the threads
    for (size_t i = 0; i < g->ctx.size(); ++i) {
        t_ctx = &g->ctx[i]->st;
        free_renderer();
    }
    t_ctx = guard.saved;
    for (auto &w : g->worker) w->stop();
    g->worker.clear();
    for (PtContext *c : g->ctx) (void)pt_ctx_destroy(c);
    group_release_buffers(g);
    for (size_t i = 0; i < g->stream.size(); ++i) {
        (void)hipSetDevice(g->device[i]);
        g->evCommit[i].release();
        (void)hipStreamSynchronize(g->stream[i]);
        g->stream[i].release();
    }
    for (GroupDevice &d : g->dev) {
        (void)hipSetDevice(d.device);
        for (Event &e : d.evRed) e.release();
        d.coll.release();
        if (d.comm) (void)g->api->CommDestroy(d.comm);
    }
    {
        std::lock_guard<std::mutex> lock(g_groupMutex);
        g_groups.erase(std::remove(g_groups.begin(), g_groups.end(), g), g_groups.end());
    }
    delete g;
}

int pt_group_size(const PtGroup *g) { return g ? (int)g->ctx.size() : 0; }
const char *pt_group_collective(const PtGroup *g) { return g ? g->how.c_str() : ""; }

int pt_group_set_meshes(PtGroup *g, const PtMesh *meshes, int nmeshes) {
    if (!g) return fail(PT_ERR_INVALID, "pt_group_set_meshes: null group");
    CurrentGuard guard;
    for (PtContext *c : g->ctx) {
        t_ctx = &c->st;
        int rc = pt_set_meshes(meshes, nmeshes);
        if (rc) return rc;
    }
    return PT_OK;
}

int pt_group_set_bump_maps(PtGroup *g, const PtBumpBinding *bindings, int nbindings, size_t binding_struct_bytes) {
    if (!g) return fail(PT_ERR_INVALID, "pt_group_set_bump_maps: null group");
    CurrentGuard guard;
    for (PtContext *c : g->ctx) {
        t_ctx = &c->st;
        int rc = pt_set_bump_maps(bindings, nbindings, binding_struct_bytes);
        if (rc) return rc;
    }
    return PT_OK;
}

int pt_group_set_textures(PtGroup *g, const PtTexture *textures, int ntextures, size_t texture_struct_bytes, const PtTexBinding *bindings,
                          int nbindings, size_t binding_struct_bytes) {
    if (!g) return fail(PT_ERR_INVALID, "pt_group_set_textures: null group");
    CurrentGuard guard;
    for (PtContext *c : g->ctx) {
        t_ctx = &c->st;
        int rc = pt_set_textures(textures, ntextures, texture_struct_bytes, bindings, nbindings, binding_struct_bytes);
        if (rc) return rc;
    }
    return PT_OK;
}

int pt_group_init(PtGroup *g, const PtCamera *cam, const PtGeom *geoms, int ngeoms, const PtMaterial *mats, int nmats, int traceDepth,
                  const PtOptions *opts) {
    if (!g || !cam) return fail(PT_ERR_INVALID, "pt_group_init: null argument");
    if (cam->resolution[0] <= 0 || cam->resolution[1] <= 0) return fail(PT_ERR_INVALID, "pt_group_init: bad resolution");
    if (opts && (opts->flags & PT_FLAG_MOMENTS)) return fail(PT_ERR_INVALID, "pt_group_init: PT_FLAG_MOMENTS is not for groups (their members hold row shards)");
    if (opts && (opts->flags & PT_FLAG_KEEP_RENDERER))
        return fail(PT_ERR_INVALID, "pt_group_init: PT_FLAG_KEEP_RENDERER is not for groups (a group re-initialises its members in place already)");
    if (opts && (opts->flags & PT_FLAG_OBJECT_HISTORY))
        return fail(PT_ERR_INVALID, "pt_group_init: PT_FLAG_OBJECT_HISTORY is not for groups (their members keep no history)");
    if (opts && (opts->flags & PT_FLAG_MOTION))
        return fail(PT_ERR_INVALID, "pt_group_init: PT_FLAG_MOTION is not for groups (pt_group_init takes one pose of the scene)");
    CurrentGuard guard;
    const int n = (int)g->ctx.size();
    {   // a re-init (the reference's Free -> Init restart): the old renderers go first, then the buffers they accumulate into
        int rc = for_members(g, [](int) -> int { free_renderer(); return PT_OK; });
        if (rc) return rc;
    }
    group_release_buffers(g);
    g->W = cam->resolution[0];
    g->H = cam->resolution[1];
    const size_t frameFloats = (size_t)g->W * (size_t)g->H * 3;
    const auto frames = [&]() -> int {
        for (GroupDevice &d : g->dev) {
            HIPCHECK(hipSetDevice(d.device));
            PTCHECK(d.full.alloc_zeroed(frameFloats));
            if (g->rccl)      // (zeroed: the rows of the OTHER devices' members stay zero for good -- no commit and no reduce writes them --,
                              // which is what the sum needs)
                for (DevBuf<float> &s : d.snap) PTCHECK(s.alloc_zeroed(frameFloats));
            if (g->rccl && g->dev.size() > 1 && &d == &g->dev[0]) PTCHECK(g->reduced.alloc_zeroed(frameFloats));      // the root's result frame (see assemble)
            HIPCHECK(hipDeviceSynchronize());
        }
        return PT_OK;
    };
    if (const int rc = frames()) { group_release_buffers(g); return rc; }      // (a failure between two allocations leaves none behind)
    g->waitRed.assign(n, 0);
    PtOptions base;
    memset(&base, 0, sizeof base);
    if (opts) base = *opts;
    int rc = for_members(g, [&](int i) -> int {
        PtOptions o = base;
        o.shard_rank = i;
        o.shard_count = n;
        o.device = g->device[i];
        o.stream = g->stream[i];
        o.flags &= ~PT_FLAG_ACCUM_SHARD_ROWS;
        o.accum_dev = g->dev[g->devIndex[i]].full.p;        // own rows in place, the co-members' beside them, zeros for the other devices' rows
        return pt_init(cam, geoms, ngeoms, mats, nmats, traceDepth, &o);
    });
    if (rc) return rc;
    if ((rc = ensure_collective(g))) return rc;      // (behind the members' tracing streams: see pt_group_create)
    g->inited = true;
    g->dirty = false;
    g->k = 0;
    g->last = -1;
    return PT_OK;
}

// every member enqueues its shard's wavefront batch (asynchronous: the devices run side by side, fed by a host thread each)
int pt_group_iterate_batch(PtGroup *g, int frame, int first_iter, int count) {
    if (!g) return fail(PT_ERR_INVALID, "pt_group_iterate_batch: null group");
    if (!g->inited) return fail(PT_ERR_NOT_INIT, "pt_group_iterate_batch before pt_group_init");
    CurrentGuard guard;
    int rc = for_members(g, [&](int i) -> int {
        if (g->rccl) {      // this call's commit copies the member's rows into snapshot k as well
            GroupDevice &d = g->dev[g->devIndex[i]];
            R().snapTarget = d.snap[g->k].p;
            R().snapWait = g->waitRed[i] ? d.evRed[g->k].h : nullptr;
            g->waitRed[i] = 0;
        }
        int r = pt_iterate_batch(frame, first_iter, count, nullptr);
        if (r) return r;
        // the member's commits so far, and the device's collective stream behind them (whatever reads the frame next -- a reduce, a read-back --
        // is enqueued there after every member is through with this: the members' threads do it side by side)
        HIPCHECK(hipEventRecord(g->evCommit[i], g->stream[i]));
        HIPCHECK(hipStreamWaitEvent(g->dev[g->devIndex[i]].coll, g->evCommit[i], 0));
        return PT_OK;
    });
    if (rc) return rc;
    g->dirty = true;
    return PT_OK;
}

// config C3 as written: one iteration on every member (a commit out of the batches traced ahead with PT_FLAG_TRACE_AHEAD), then the
// frame's assembly -- the reference's per-iteration full-frame transfer (src/pathtrace.cu:170-171) with the reduce in its place
int pt_group_iterate(PtGroup *g, int frame, int iter) {
    int rc = pt_group_iterate_batch(g, frame, iter, 1);
    if (rc) return rc;
    return pt_group_reduce(g);
}

int pt_group_reduce(PtGroup *g) {
    if (!g) return fail(PT_ERR_INVALID, "pt_group_reduce: null group");
    if (!g->inited) return fail(PT_ERR_NOT_INIT, "pt_group_reduce before pt_group_init");
    CurrentGuard guard;
    return assemble(g);
}

int pt_group_sync(PtGroup *g) {
    if (!g) return fail(PT_ERR_INVALID, "pt_group_sync: null group");
    if (!g->inited) return fail(PT_ERR_NOT_INIT, "pt_group_sync before pt_group_init");
    CurrentGuard guard;
    int rc = for_members(g, [](int) -> int { return pt_sync(); });      // (reports a member's device fault)
    if (rc) return rc;
    for (GroupDevice &d : g->dev) {
        HIPCHECK(hipSetDevice(d.device));
        HIPCHECK(hipStreamSynchronize(d.coll));
    }
    return PT_OK;
}

// the whole frame's un-normalised running sum (W * H * 3 floats), as pt_readback delivers it for one device.  Waits for the frame's
// assembly and the copy only -- not for the batches the members trace ahead.
int pt_group_readback(PtGroup *g, float *rgb_sum_host) {
    if (!g || !rgb_sum_host) return fail(PT_ERR_INVALID, "pt_group_readback: null argument");
    if (!g->inited) return fail(PT_ERR_NOT_INIT, "pt_group_readback before pt_group_init");
    CurrentGuard guard;
    const size_t frameFloats = (size_t)g->W * g->H * 3;
    int rc;
    if (g->dirty || (g->rccl && g->last < 0)) {
        if ((rc = assemble(g))) return rc;
    }
    if (g->rccl) {
        HIPCHECK(hipSetDevice(g->dev[0].device));
        const float *const frame = g->reduced.p ? g->reduced.p : g->dev[0].snap[g->last].p;
        HIPCHECK(hipMemcpyAsync(rgb_sum_host, frame, frameFloats * sizeof(float), hipMemcpyDeviceToHost, g->dev[0].coll));
        HIPCHECK(hipStreamSynchronize(g->dev[0].coll));
    } else if (g->dev.size() == 1) {
        HIPCHECK(hipSetDevice(g->dev[0].device));
        HIPCHECK(hipMemcpyAsync(rgb_sum_host, g->dev[0].full.p, frameFloats * sizeof(float), hipMemcpyDeviceToHost, g->dev[0].coll));
        HIPCHECK(hipStreamSynchronize(g->dev[0].coll));
    } else {
        // host gather: row y belongs to member y % n, i.e. to that member's device
        g->stage.resize(frameFloats);
        const size_t rowFloats = (size_t)g->W * 3;
        const int n = (int)g->ctx.size();
        for (size_t di = 0; di < g->dev.size(); ++di) {
            GroupDevice &d = g->dev[di];
            HIPCHECK(hipSetDevice(d.device));
            HIPCHECK(hipMemcpyAsync(g->stage.data(), d.full.p, frameFloats * sizeof(float), hipMemcpyDeviceToHost, d.coll));
            HIPCHECK(hipStreamSynchronize(d.coll));
            for (int y = 0; y < g->H; ++y)
                if (g->devIndex[y % n] == (int)di) memcpy(rgb_sum_host + (size_t)y * rowFloats, g->stage.data() + (size_t)y * rowFloats, rowFloats * sizeof(float));
        }
    }
    // a member's device fault: the kernels write the sticky fault word to page-locked host memory too (readback_fault), so the good path
    // costs no copy and no wait for the members' streams
    for (PtContext *c : g->ctx) {
        t_ctx = &c->st;
        if (R().hostFault && *(volatile uint32_t *)R().hostFault != 0u) {
            (void)hipSetDevice(R().device);
            if ((rc = readback_fault())) return rc;
        }
    }
    return PT_OK;
}

// the members' tallies, summed (every member counts the paths of its own rows)
int pt_group_counters(PtGroup *g, PtCounters *out) {
    if (!g || !out) return fail(PT_ERR_INVALID, "pt_group_counters: null argument");
    if (!g->inited) return fail(PT_ERR_NOT_INIT, "pt_group_counters before pt_group_init");
    CurrentGuard guard;
    memset(out, 0, sizeof *out);
    std::vector<PtCounters> cs(g->ctx.size());
    int rc = for_members(g, [&](int i) -> int { return pt_counters(&cs[i]); });
    if (rc) return rc;
    for (size_t i = 0; i < cs.size(); ++i) {
        const PtCounters &c = cs[i];
        for (int d = 0; d < PT_MAX_DEPTH + 2; ++d) { out->live[d] += c.live[d]; out->ended_early[d] += c.ended_early[d]; }
        out->light_hits += c.light_hits;
        out->misses += c.misses;
        out->iterations = i == 0 ? c.iterations : std::min(out->iterations, c.iterations);
        out->bounce_launches += c.bounce_launches;
        out->bounce_kernel_ms += c.bounce_kernel_ms;
    }
    return PT_OK;
}
